"""The walks' lower bounds and the resident tree against an f64 model (tests/bounds_model.py).

Every distance the library returns is claimed to be the exact minimum, bit for bit; that rests on the walks skipping a subtree or a leaf
triangle only when its lower bound is conservative.  Here the bound itself is tested, element by element: a point p, a triangle T and a
node N above T.  The device evaluates the library's own inline functions (walk.hip.h, through the test hook m2s_debug_eval) on the records
downloaded from a resident mesh (m2s_debug_mesh_arrays); the model decodes the tree, makes the points and knows the true distance.  No
kernel walks anything here, and no check needs a subtree minimum.

  a. structure: the arrays are the tree they claim to be, for every leaf size a grid call marks it with
  b. the stored oriented bounds and pre-test planes contain the geometry, in f64, zero tolerance
  c. the walks' own comparison never prunes T, or a node above T, while T's computed distance is the best one or ties with it
  d. what margin the bounds would need against the TRUE distance: measured and printed, asserted against nothing taken from the run
  e. the checks fail on records shrunk by 1e-4"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bounds_model as bm  # noqa: E402
import oracle as orc  # noqa: E402
import sample_model  # noqa: E402
from mesh_to_sdf_amd import Grid, Mesh, Topology, _lib, meshes  # noqa: E402
from test_gpu_closest import _sliver_meshes  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
MAX_TRIS = 512          # triangles per mesh that get points (all of them below that)
N_ON = 9                # bounds_model.triangle_points: the first nine points lie on the triangle


def _offset(v, d):
    return (v + np.asarray(d, F)).astype(F)


def _nan_inf_blob():
    v, idx = meshes.blob(24, 13)
    v = v.copy()
    v[17, 1] = np.nan
    v[140, 0] = np.inf
    return v, idx


def _random_triangles(n):
    return np.random.default_rng(40 + n).uniform(-1, 1, (3 * n, 3)).astype(F), np.arange(3 * n, dtype=np.uint32)


def _sliver(k):
    return list(_sliver_meshes())[k][1:]


# name -> (maker, has planted non-finite or overflowing vertices)
MESHES = {
    "blob-6k": (lambda: meshes.named("blob-6k"), False),            # all three NodeExt builder forms: thread, wave, cylinder
    "blob": (lambda: meshes.blob(24, 13), False),
    "blob x 1e-3": (lambda: ((meshes.blob(24, 13)[0] * F(1e-3)).astype(F), meshes.blob(24, 13)[1]), False),
    "blob x 1e3": (lambda: ((meshes.blob(24, 13)[0] * F(1e3)).astype(F), meshes.blob(24, 13)[1]), False),
    "blob at (1000, -2000, 500)": (lambda: (_offset(meshes.blob(24, 13)[0], [1000, -2000, 500]), meshes.blob(24, 13)[1]), False),
    "blob at 1e4 (1, -1, 1)": (lambda: (_offset(meshes.blob(24, 13)[0], [1e4, -1e4, 1e4]), meshes.blob(24, 13)[1]), False),
    "sheet": (lambda: meshes.sheet(20, 20, rotate=False), False),   # thin slabs
    "sheet rotated": (lambda: meshes.sheet(20, 20), False),
    "random slivers": (lambda: _sliver(0), False),
    "blob with slivers": (lambda: _sliver(1), False),
    "with degenerates": (lambda: sample_model.with_degenerates(*meshes.blob(12, 9)), True),
    "one huge": (lambda: sample_model.one_huge(*meshes.blob(12, 9)), False),
    "NaN and inf vertex": (_nan_inf_blob, True),
    "1 triangle": (lambda: _random_triangles(1), False),
    "2 triangles": (lambda: _random_triangles(2), False),
    "3 triangles": (lambda: _random_triangles(3), False),
}


def _records(arr):
    return arr["tris"], arr["planes"], arr["nodes"], arr["ext"]


def device_values(pts, pt_tri, el_pt, el_node, tris, planes, ext, scale):
    """The device's values for the points pts (triangle slot pt_tri each) and the elements (point el_pt, node el_node): the bounds P
    (planes_dist2) and B (ext_dist2), the exact evaluation's d2, the slacks and the two pruning thresholds."""
    n = len(pts)
    out = {}
    out["P"] = _lib.debug_eval(_lib.EVAL_PLANES, pts, planes[pt_tri])
    out["d2"] = _lib.debug_eval(_lib.EVAL_DIST2, pts, tris[pt_tri])
    for k, fold in (("s0", 0.0), ("s1", 1.0)):
        out[k] = _lib.debug_eval(_lib.EVAL_SLACK, pts, None, np.stack([np.full(n, scale, F), np.full(n, fold, F)], 1))
    out["thr"] = _lib.debug_eval(_lib.EVAL_PRUNE, None, None, np.stack([out["d2"], out["s0"]], 1))
    out["thr_n"] = _lib.debug_eval(_lib.EVAL_PRUNE, None, None, np.stack([bm.lowered_d2(out["d2"]), out["s1"]], 1))
    out["B"] = _lib.debug_eval(_lib.EVAL_EXT, pts[el_pt], ext[el_node])
    return out


def pruning_failures(dev, el_pt):
    """Elements (and points) the walks' comparison would drop although T's own computed distance is the best so far."""
    bad_B = bm.pruned(dev["B"], dev["thr"][el_pt]) | bm.pruned(dev["B"], dev["thr_n"][el_pt])
    bad_P = bm.pruned(dev["P"], dev["thr"]) | bm.pruned(dev["P"], dev["thr_n"])
    return np.flatnonzero(bad_B), np.flatnonzero(bad_P)


class Case:
    def __init__(self, name):
        make, self.planted = MESHES[name]
        self.name = name
        self.v, self.idx = make()
        self.v = np.ascontiguousarray(self.v, F).reshape(-1, 3)
        self.idx = np.ascontiguousarray(self.idx, np.uint32).reshape(-1)
        self.n = self.idx.size // 3
        with Mesh(self.v, Topology.TriangleList(self.idx)) as m:
            self.arr = m.debug_arrays(bm.DTYPES)
        tris, planes, nodes, ext = _records(self.arr)
        self.scale = bm.mesh_scale(self.arr["scene"])
        self.skip, self.first = nodes["skip"].astype(np.int64), self.arr["slot_first"].astype(np.int64)
        tree_bad = bm.tree_errors(self.skip, self.first, self.n)
        assert not tree_bad, f"{name}: the skip links are no pre-order tree: {tree_bad}"
        # every (triangle, node above it) pair of the whole tree: what the containment checks run over
        self.all_k, self.all_node = bm.ancestors(self.skip, self.first, np.arange(self.n))
        rng = np.random.default_rng(20261019)
        self.picks = np.arange(self.n) if self.n <= MAX_TRIS else np.sort(rng.choice(self.n, MAX_TRIS, replace=False))
        t = tris[self.picks]
        tp = bm.round_points(bm.triangle_points(t["a"], t["b"], t["c"], self.scale, rng))
        P = tp.shape[1]
        k, node = bm.ancestors(self.skip, self.first, self.picks)
        dp = bm.round_points(bm.disc_points(ext[node])).reshape(-1, 3)
        D = dp.shape[0] // len(node)
        pts = np.concatenate([tp.reshape(-1, 3), dp])
        pt_tri = np.concatenate([np.repeat(self.picks, P), np.repeat(self.picks[k], D)])
        pt_on = np.concatenate([np.tile(np.arange(P) < N_ON, len(self.picks)), np.zeros(len(dp), bool)])
        el_pt = np.concatenate([(k[:, None] * P + np.arange(P)[None, :]).reshape(-1), len(self.picks) * P + np.arange(len(dp))])
        el_node = np.concatenate([np.repeat(node, P), np.repeat(node, D)])
        tv, tfin = bm.tri_vertices(tris)
        keep = np.isfinite(pts).all(1) & tfin.all(1)[pt_tri]
        self.left_out = int((~keep).sum())
        renum = np.cumsum(keep) - 1
        ek = keep[el_pt]
        self.pts, self.pt_tri, self.pt_on = np.ascontiguousarray(pts[keep]), pt_tri[keep], pt_on[keep]
        self.el_pt, self.el_node = renum[el_pt[ek]], el_node[ek]
        self.dev = device_values(self.pts, self.pt_tri, self.el_pt, self.el_node, tris, planes, ext, self.scale)
        t = tris[self.pt_tri]
        self.delta = bm.point_triangle_distance(self.pts, t["a"], t["b"], t["c"])

    def describe(self, e=None, p=None):
        """One failing element (or point) by name: the point, the triangle record, the node record and the device's values."""
        tris, planes, nodes, ext = _records(self.arr)
        p = self.el_pt[e] if e is not None else p
        T = self.pt_tri[p]
        s = (f"{self.name}: p = {self.pts[p].tolist()} (bits {self.pts[p].view(np.uint32).tolist()}), triangle slot {T} (input {tris['index'][T]}): "
             f"a {tris['a'][T].tolist()} b {tris['b'][T].tolist()} c {tris['c'][T].tolist()}, planes {planes[T].tolist()}; "
             f"d2 {self.dev['d2'][p]!r} thr {self.dev['thr'][p]!r} thr_n {self.dev['thr_n'][p]!r} P {self.dev['P'][p]!r} true distance {self.delta[p]!r}")
        if e is not None:
            N = self.el_node[e]
            s += f"; node slot {N} ({bm.subtree_counts(self.skip)[N]} triangles): {ext[N].tolist()}, B {self.dev['B'][e]!r}"
        return s


@pytest.fixture(scope="module", params=list(MESHES))
def case(request):
    """One mesh at a time: built, downloaded, its points made, the device's values and the model's distances computed once, shared by
    the tests below and left unchanged by them."""
    return Case(request.param)


def _structure_errors(arr, v, idx):
    """(a) on one download: everything the walks assume about the arrays, exact."""
    tris, planes, nodes, ext = _records(arr)
    n = idx.size // 3
    bad = []
    assert len(tris) == n == len(planes) == len(arr["slot_of"]) and len(nodes) == len(ext) == len(arr["slot_first"]) == (2 * n - 1 if n else 0)
    slot_of = arr["slot_of"].astype(np.int64)
    if not np.array_equal(np.sort(slot_of), np.arange(n)):
        return ["slot_of is no permutation"]
    if not np.array_equal(tris["index"][slot_of], np.arange(n)):
        bad.append("tris[slot_of[i]].index != i")
    want = v[idx.reshape(-1, 3).astype(np.int64)]                                   # [n, 3, 3], input order
    got = np.stack([tris["a"], tris["b"], tris["c"]], 1)[slot_of]
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        bad.append("a record's vertices are not the input's bits")
    skip, first = nodes["skip"].astype(np.int64), arr["slot_first"].astype(np.int64)
    bad += bm.tree_errors(skip, first, n)
    if bad:
        return bad
    if not np.array_equal(ext["skip"].astype(np.int64), 48 * skip):
        bad.append("ext.skip != 48 nodes.skip")
    if not np.array_equal(ext["tri"], nodes["tri"]):
        bad.append("ext.tri != nodes.tri")
    cnt, leaf_max = bm.subtree_counts(skip), arr["leaf_max"]
    if not np.array_equal(nodes["tri"], np.where(cnt <= leaf_max, first, -1)):
        bad.append(f"tri marks do not follow leaf_max = {leaf_max}")
    return bad


def test_structure(case):
    assert _structure_errors(case.arr, case.v, case.idx) == []
    assert case.arr["leaf_max"] >= 1
    # every box contains every finite vertex of its subtree
    out = bm.box_violations(case.arr["nodes"], case.arr["tris"], case.all_k, case.all_node)
    assert len(out) == 0, f"{case.name}: {len(out)} vertices outside a box above them, first (pair, vertex) {out[0]}: triangle slot {case.all_k[out[0][0]]}, node {case.all_node[out[0][0]]}"


def test_structure_holds_for_every_leaf_size():
    """Grid calls re-mark the leaves of a resident tree (set_leaf_size): the grid sizes of test_persistent_mesh_leaf_size_follows_the_grid,
    which ask for leaves of 2, 4, 8 and 16 triangles (the library's own rule through m2s_debug_leaf_sizes)."""
    v, idx = meshes.named("blob-6k")
    L = _lib.lib()
    L.m2s_debug_leaf_sizes.restype = C.c_int
    L.m2s_debug_leaf_sizes.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    seen = []
    with Mesh(v, Topology.TriangleList(idx)) as m:
        first = m.debug_arrays(bm.DTYPES)
        for n in (96, 24, 12, 48, 64, 12, 96):
            g = Grid.from_bounding_box(*meshes.extended_bbox(v, 0.1), [n, n, n])
            out3 = (C.c_uint32 * 3)()
            assert L.m2s_debug_leaf_sizes(C.byref(g._g), idx.size // 3, 0, out3) == 0
            m.generate_grid_sdf(g)
            arr = m.debug_arrays(bm.DTYPES)
            assert arr["leaf_max"] == out3[0], (n, arr["leaf_max"], out3[0])
            assert _structure_errors(arr, v, idx) == [], n
            seen.append(arr["leaf_max"])
            for k in ("tris", "planes", "slot_of", "slot_first", "scene"):           # nothing else of the tree depends on the leaf size
                assert arr[k].tobytes() == first[k].tobytes(), (n, k)
            for k, fields in (("nodes", ("mn", "skip", "mx")), ("ext", ("c", "R", "n", "mid", "half", "skip"))):
                for f in fields:
                    assert arr[k][f].tobytes() == first[k][f].tobytes(), (n, k, f)
    assert seen == [2, 8, 16, 8, 4, 16, 2]


def test_hook_argument_checks_with_a_mesh():
    """Wrong `which` and a short capacity fail with M2S_ERR_BAD_ARG, and the size query needs no buffer."""
    v, idx = meshes.blob(12, 9)
    L = _lib.lib()
    with Mesh(v, Topology.TriangleList(idx)) as m:
        m.debug_arrays()
        fn = L.m2s_debug_mesh_arrays
        nbytes = C.c_size_t(0)
        n = idx.size // 3
        for which, size in enumerate((96 * n, 64 * n, 32 * (2 * n - 1), 48 * (2 * n - 1), 4 * n, 4 * (2 * n - 1), 36, 4)):
            assert fn(m._h, which, None, 0, C.byref(nbytes)) == 0 and nbytes.value == size, which
            buf = np.full(size // 4, 0xDEADBEEF, np.uint32)
            assert fn(m._h, which, buf.ctypes.data, size - 1, None) == _lib.ERR_BAD_ARG
            assert (buf == 0xDEADBEEF).all()
            assert fn(m._h, which, buf.ctypes.data, size, None) == 0
        for which in (-1, 8, 100):
            assert fn(m._h, which, None, 0, C.byref(nbytes)) == _lib.ERR_BAD_ARG
        assert fn(m._h, 0, None, 0, None) == _lib.ERR_BAD_ARG


def _units(reserve, size):
    """Smallest reserve in units of 2^-24 x the quantity's size (finite entries with a size only)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        r = np.asarray(reserve, np.float64) / (bm.U * np.asarray(size, np.float64))
    r = r[np.isfinite(r)]
    return float(r.min()) if r.size else float("nan")


def stored_bound_failures(tris, planes, ext, all_k, all_node, name=""):
    """(b): the (triangle, node) pairs with a finite vertex outside the node's slab or disc, and the triangles whose pre-test planes do
    not hold their own vertices or are no unit vectors."""
    slab, rad, size = bm.ext_reserves(ext, tris, all_k, all_node)
    has, edge, face, unit, vmax = bm.plane_reserves(planes, tris)
    if name:
        print(f"\n[reserves] {name}: slab {_units(slab, size):.3g}  radius^2 {_units(rad, size * size):.3g}  plane edges {_units(edge[has], vmax[has]):.3g}  "
              f"face {_units(face[has], vmax[has]):.3g}  unit length {_units(unit[has], np.ones(int(has.sum()))):.3g}   (units of 2^-24 x size; smallest)")
    bad_pair = np.flatnonzero(bm.outside(slab).any(1) | bm.outside(rad).any(1))
    with np.errstate(invalid="ignore"):
        bad_tri = np.flatnonzero(has & ~((edge >= 0) & (face >= 0) & (unit >= 0)))
    return bad_pair, bad_tri, has


def test_stored_bounds_contain_the_geometry(case):
    tris, planes, nodes, ext = _records(case.arr)
    bad_pair, bad_tri, has = stored_bound_failures(tris, planes, ext, case.all_k, case.all_node, case.name)
    assert not (has & (tris["cls"] != bm.TRI_REGULAR)).any(), "a degenerate triangle carries pre-test planes"
    msg = ""
    if len(bad_pair):
        k, N = case.all_k[bad_pair[0]], case.all_node[bad_pair[0]]
        msg += f"{len(bad_pair)} (triangle, node) pairs stick out; first: triangle slot {k} a {tris['a'][k].tolist()} b {tris['b'][k].tolist()} c {tris['c'][k].tolist()} node slot {N} {ext[N].tolist()}. "
    if len(bad_tri):
        k = bad_tri[0]
        _, edge, face, unit, vmax = bm.plane_reserves(planes[k:k + 1], tris[k:k + 1])
        msg += (f"{len(bad_tri)} pre-test records fail; first: triangle slot {k} a {tris['a'][k].tolist()} b {tris['b'][k].tolist()} c {tris['c'][k].tolist()} "
                f"planes {planes[k].tolist()}: edge reserve {edge[0]!r}, face reserve {face[0]!r} (vmax {vmax[0]!r}), unit reserve {unit[0]!r}")
    assert not msg, f"{case.name}: {msg}"


def test_no_walk_prunes_the_best_triangle(case):
    """(c).  For every element (p, T, N): B = ext_dist2(p, ext[N]), P = planes_dist2(p, planes[T]), d2 = the exact evaluation's value for T,
    thr = prune_bound(d2, slack) and thr_n = prune_bound(d2 lowered by the Normal fold's tie window, slack with the fold's term) — all of
    them the device's values.  Neither bound may exceed either threshold: that is the comparison the walks make."""
    if not case.planted:
        assert case.left_out == 0, f"{case.name}: {case.left_out} points are not finite"
    assert len(case.pts) and len(case.el_pt)
    bad_B, bad_P = pruning_failures(case.dev, case.el_pt)
    print(f"\n[elements] {case.name}: {len(case.picks)} triangles, {len(case.pts)} points, {len(case.el_pt)} elements, {case.left_out} points left out")
    msg = ""
    if len(bad_B):
        msg += f"{len(bad_B)} elements whose node would be pruned; first: {case.describe(e=bad_B[0])}. "
    if len(bad_P):
        msg += f"{len(bad_P)} points whose triangle would be pruned by its pre-test; first: {case.describe(p=bad_P[0])}"
    assert not msg, msg


def test_margin_needed_against_the_true_distance(case):
    """(d).  The margin each bound would need if the comparison were made against the TRUE distance delta of T (f64 model): printed per
    mesh and bound, recorded in DESIGN.md section 4; nothing is asserted against a figure of this run.  What is asserted: the probe's d2
    is the oracle's, bit for bit, on a seeded subsample."""
    d = case.dev
    scale = np.maximum(case.scale, np.abs(case.pts).max(1)).astype(np.float64)
    for what, bound, slack, delta, sc in (("planes", d["P"], d["s0"], case.delta, scale),
                                          ("ext", d["B"], d["s0"][case.el_pt], case.delta[case.el_pt], scale[case.el_pt])):
        rel, ab = bm.needed_margin(bound, slack.astype(np.float64), delta, sc)
        rel, ab = rel[np.isfinite(rel)], ab[np.isfinite(ab)]
        print(f"\n[margin] {case.name}: {what}: rel_needed max {rel.max() if rel.size else float('nan'):.3g} ({rel.max() / bm.U if rel.size else float('nan'):.3g} u)  "
              f"abs_needed max {ab.max() if ab.size else float('nan'):.3g} x scale ({ab.max() / bm.U if ab.size else float('nan'):.3g} u)")
    tris = case.arr["tris"]
    rng = np.random.default_rng(7)
    sub = rng.choice(len(case.pts), min(2000, len(case.pts)), replace=False)
    for p in sub:
        T = case.pt_tri[p]
        want = orc.point_triangle_distance2(case.pts[p], tris["a"][T], tris["b"][T], tris["c"][T])
        got = d["d2"][p]
        if np.isnan(want):
            assert got == np.inf, case.describe(p=p)        # eval_triangle: f32::min drops a NaN operand, a fresh Best holds +inf
        else:
            assert got.view(np.uint32) == want.view(np.uint32), (case.describe(p=p), got, want)


def test_the_checks_have_teeth():
    """(e).  Copies of the blob's records with every half and R shrunk by 1e-4 relative and every o_k moved inwards by 1e-4 vmax: (b) must
    find a node and a triangle, (c) an element; on the unmutated copies both find nothing."""
    c = Case("blob")
    tris, planes, nodes, ext = (x.copy() for x in _records(c.arr))
    on = np.flatnonzero(c.pt_on)                                                     # the points on T, with every node above T
    renum = np.full(len(c.pts), -1)
    renum[on] = np.arange(len(on))
    ek = c.pt_on[c.el_pt]
    pts, pt_tri, el_pt, el_node = c.pts[on], c.pt_tri[on], renum[c.el_pt[ek]], c.el_node[ek]

    def failures(planes_, ext_):
        bad_pair, bad_tri, _ = stored_bound_failures(tris, planes_, ext_, c.all_k, c.all_node)
        bad_B, bad_P = pruning_failures(device_values(pts, pt_tri, el_pt, el_node, tris, planes_, ext_, c.scale), el_pt)
        return len(bad_pair), len(bad_tri), len(bad_B), len(bad_P)

    assert failures(planes, ext) == (0, 0, 0, 0)
    small_ext, small_planes = ext.copy(), planes.copy()
    small_ext["half"] = small_ext["half"] * F(1 - 1e-4)
    small_ext["R"] = small_ext["R"] * F(1 - 1e-4)
    has, _, _, _, vmax = bm.plane_reserves(planes, tris)
    for o in ("o0", "o1", "o2"):
        small_planes[o] = np.where(has, small_planes[o] - (1e-4 * vmax).astype(F), small_planes[o])
    n_pair, n_tri, n_B, n_P = failures(small_planes, small_ext)
    print(f"\n[teeth] shrunk records: {n_pair} (triangle, node) pairs and {n_tri} triangles fail (b), {n_B} elements and {n_P} points fail (c)")
    assert n_pair >= 1 and n_tri >= 1
    assert n_B >= 1 and n_P >= 1
