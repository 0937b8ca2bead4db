"""Voxelization without a GPU: the host build of csrc/voxel.hip.h against the numpy model of the contract (tests/voxel_model.py) bit
for bit, the interval searches against trying every index, an exactly representable case with a closed-form count, the conservative /
tight property against float64, the exports, and the argument checks that happen before any device work."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_model as vm  # noqa: E402
from mesh_to_sdf_amd import Grid, M2SError, M2SPanic, Topology, _lib, meshes, voxelize  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(os.path.dirname(_lib.SO_PATH), "libm2s_probe.so")
FAR = np.array([1.0e4, -1.0e4, 1.0e4], F)


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        _lib.build()
    L = C.CDLL(PROBE)
    L.probe_vox_overlap.argtypes = [C.c_uint64] + [C.c_void_p] * 4
    L.probe_vox_centre.restype = C.c_float
    L.probe_vox_centre.argtypes = [C.c_float, C.c_float, C.c_uint32]
    L.probe_vox_interval.argtypes = [C.c_float] * 5 + [C.c_uint32, C.c_void_p]
    L.probe_vox_raster.argtypes = [C.c_void_p] * 5
    return L


def _probe_overlap(probe, tris, q, h):
    tris, q, h = (np.ascontiguousarray(np.broadcast_to(x, s), F) for x, s in ((tris, (len(q), 3, 3)), (q, (len(q), 3)), (h, (len(q), 3))))
    out = np.zeros(len(q), np.uint8)
    probe.probe_vox_overlap(len(q), tris.ctypes.data, q.ctypes.data, h.ctypes.data, out.ctypes.data)
    return out.astype(bool)


def _probe_surface(probe, tris, first, size, count):
    occ = np.zeros(count, np.uint8)
    first, size, n = np.ascontiguousarray(first, F), np.ascontiguousarray(size, F), np.asarray(count, np.uint32)
    for t in np.ascontiguousarray(tris, F):
        probe.probe_vox_raster(t.ctypes.data, first.ctypes.data, size.ctypes.data, n.ctypes.data, occ.ctypes.data)
    return occ


def _padded_grid(v, count, frac=0.05):
    lo, hi = meshes.extended_bbox(v, frac)
    return meshes.grid_from_bounding_box(lo, hi, count)


# ---- 1. the predicate -----------------------------------------------------------------------------------------------------------------
def test_probe_matches_model_on_random_pairs(probe):
    rng = np.random.default_rng(7)
    n = 200_000
    tris = rng.uniform(-1, 1, (n, 3, 3)).astype(F)
    tris[n // 2:] = (tris[n // 2:, :1] + F(0.15) * tris[n // 2:]).astype(F)      # the second half small: cell-sized triangles
    q = rng.uniform(-1, 1, (n, 3)).astype(F)
    q[n // 2:] = (tris[n // 2:, 0] + rng.uniform(-0.3, 0.3, (n - n // 2, 3)).astype(F)).astype(F)   # ... with a cell near each
    h = rng.uniform(0.02, 0.3, (n, 3)).astype(F)
    want = vm.overlap(tris, q, h)
    assert 0.05 < want.mean() < 0.95
    got = _probe_overlap(probe, tris, q, h)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]


def _adversarial():
    """(tris [n, 3, 3], q [n, 3], h [n, 3], expected or None) on the grid of cell size 2^-2 with centres at odd multiples of 2^-3: every
    coordinate, difference and product below is exactly representable, so `expected` is geometry, not rounding."""
    H = F(0.125)
    rows = []

    def add(tri, q, expected, h=(H, H, H)):
        rows.append((np.array(tri, F), np.array(q, F), np.array(h, F), expected))

    cell = (0.125, 0.125, 0.125)                                                  # the box [0, 0.25]^3
    add([[0.25, 0, 0], [0.25, 0.25, 0], [0.25, 0, 0.25]], cell, True)             # lies in the face x = 0.25
    add([[0.25, 0, 0], [0.5, 0.25, 0], [0.5, 0, 0.25]], cell, True)               # touches the face at an edge of the cell's
    add([[0.25, 0.25, 0.1], [0.5, 0.5, 0.1], [0.5, 0.25, 0.2]], cell, True)       # touches the edge x = y = 0.25 in a point
    add([[0.25, 0.25, 0.25], [0.5, 0.5, 0.5], [0.5, 0.25, 0.5]], cell, True)      # a vertex exactly at the corner
    add([[0.25, 0.25, 0.25], [0.5, 0.5, 0.5], [0.5, 0.25, 0.5]], (0.375, 0.375, 0.375), True)     # ... the neighbour across it
    add([[0.25, 0.25, 0.25], [0.5, 0.5, 0.5], [0.5, 0.25, 0.5]], (-0.125, 0.125, 0.125), False)   # ... one cell away
    add([[0.2500001, 0, 0], [0.5, 0.25, 0], [0.5, 0, 0.25]], cell, False)         # one ulp off the face
    add([[0.375, -0.125, 0.0], [-0.125, 0.375, 0.0], [0.375, 0.375, 0.0]], cell, True)   # the diagonal x + y = 0.25 cuts the corner's square
    add([[0.625, -0.125, 0.0], [-0.125, 0.625, 0.0], [0.625, 0.625, 0.0]], cell, True)   # x + y = 0.5 touches the corner (0.25, 0.25)
    add([[0.75, -0.125, 0.0], [-0.125, 0.75, 0.0], [0.75, 0.75, 0.0]], cell, False)      # x + y = 0.625: only a cross axis separates
    add([[-1, -1, 0.5], [1, -1, 0.5], [0, 1, 0.5]], cell, False)                  # only the plane separates
    add([[-1, -1, 0.25], [1, -1, 0.25], [0, 1, 0.25]], cell, True)                # the plane z = 0.25 through the top face
    # slivers
    add([[0, 0, 0.1], [1, 1.0e-7, 0.1], [2, 0, 0.1]], cell, None)
    add([[-3, 0.125, 0.125], [3, 0.125, 0.125], [0, 0.125 + 1.0e-6, 0.125]], cell, True)
    # zero area: segments and points
    add([[0, 0, 0], [0.25, 0.25, 0.25], [0.125, 0.125, 0.125]], cell, True)       # a diagonal of the cell
    add([[0.25, 0.25, 0], [0.25, 0.25, 1], [0.25, 0.25, 0.5]], cell, True)        # a segment along the cell's edge
    add([[0.5, 0.5, 0], [0.5, 0.5, 1], [0.5, 0.5, 0.5]], cell, False)
    add([[0.25, 0.25, 0.25]] * 3, cell, True)                                     # a point at the corner
    add([[0.125, 0.125, 0.125]] * 3, cell, True)                                  # a point at the centre
    add([[0.26, 0.125, 0.125]] * 3, cell, False)
    add([[0.3, 0.1, 0.1], [0.5, 0.1, 0.1], [0.3, 0.1, 0.1]], cell, False)         # a repeated vertex
    # not finite: overlaps nothing, wherever the rest lies
    add([[np.nan, 0.1, 0.1], [0.1, 0.1, 0.1], [0.1, 0.2, 0.1]], cell, False)
    add([[np.inf, 0.1, 0.1], [-1, 0.1, 0.1], [0.1, 0.2, 0.1]], cell, False)
    # finite vertices whose edges overflow: the cross axes and the plane are NaN and never miss
    add([[3.0e38, 0, 0.1], [0, 3.0e38, 0.1], [-3.0e38, -3.0e38, 0.1]], cell, True)
    add([[3.0e38, 0, 0.5], [0, 3.0e38, 0.5], [-3.0e38, -3.0e38, 0.5]], cell, False)      # ... but the z box clause does
    # offset by 1e4: spacing of f32 there is 2^-10
    o = 1.0e4
    add([[o + 0.25, o, o], [o + 0.25, o + 0.25, o], [o + 0.25, o, o + 0.25]], (o + 0.125, o + 0.125, o + 0.125), True)
    add([[o + 0.5, o, o], [o + 0.5, o + 0.25, o], [o + 0.5, o, o + 0.25]], (o + 0.125, o + 0.125, o + 0.125), False)
    t, q, h, e = zip(*rows)
    return np.stack(t), np.stack(q), np.stack(h), list(e)


def test_probe_matches_model_on_adversarial_pairs(probe):
    tris, q, h, expected = _adversarial()
    want = vm.overlap(tris, q, h)
    for i, e in enumerate(expected):
        assert e is None or bool(want[i]) == e, f"model, case {i}: {tris[i].tolist()} vs {q[i].tolist()}"
    got = _probe_overlap(probe, tris, q, h)
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    # every case again with the vertices rotated and reversed: the clauses name a, b, c, the answer on exact inputs does not depend on them
    for perm in ([1, 2, 0], [2, 0, 1], [0, 2, 1]):
        w2 = vm.overlap(tris[:, perm], q, h)
        assert np.array_equal(_probe_overlap(probe, tris[:, perm], q, h), w2)
        for i, e in enumerate(expected):
            assert e is None or bool(w2[i]) == e, (perm, i)


def test_probe_centres_match_model_and_do_not_decrease(probe):
    for first, size, n in ((-1.1, 0.1375, 16), (1.0e4 - 1.2, 2.4 / 32, 32), (-3.0e38, 1.0e37, 64), (0.0, 1.0e-3, 70000), (5.0, 2.0 ** -22, 4096)):
        q = vm.centres(first, size, n)
        got = np.array([probe.probe_vox_centre(F(first), F(size), i) for i in range(0, n, max(1, n // 512))], F)
        assert np.array_equal(got.view(np.uint32), q[::max(1, n // 512)].view(np.uint32))
        assert (q[1:] >= q[:-1]).all()
    assert np.unique(vm.centres(5.0, 2.0 ** -22, 4096)).size < 0.6 * 4096          # (centres do collapse there)


# ---- 2. the interval searches -------------------------------------------------------------------------------------------------------------
def _interval_cases():
    b = meshes.blob(12, 9)
    t_near = vm.triangles_of(*b)
    t_far = vm.triangles_of((b[0] + FAR).astype(F), b[1])
    near = _padded_grid(b[0], (32, 20, 33))
    far = _padded_grid((b[0] + FAR).astype(F), (32, 32, 32))
    inner = meshes.grid_from_bounding_box([-0.5, -0.4, -0.3], [0.45, 0.5, 0.2], (16, 7, 40))   # triangles partly and wholly outside
    one = meshes.grid_from_bounding_box([-0.3, -0.3, -0.3], [0.9, 0.9, 0.9], (1, 1, 1))
    collapsed = (np.array([5.0, 5.0, 5.0], F), np.array([2.0 ** -22] * 3, F), (4096, 8, 8))     # many indices share a centre
    big = np.array([[[-50, -60, -9], [80, -10, 7], [-20, 90, 6]]], F)
    return [("near", t_near, near), ("far", t_far, far), ("partly outside", t_near, inner), ("one cell", t_near, one),
            ("larger than the grid", big, near), ("collapsed centres", (t_near * F(1.0e-3) + F(5.0)).astype(F), collapsed)]


def test_interval_searches_return_exactly_the_passing_indices(probe):
    out = np.zeros(2, np.uint32)
    empties = 0
    for name, tris, (first, size, count) in _interval_cases():
        for tri in tris:
            for m in range(3):
                ok = vm.box_pass(tri[0, m], tri[1, m], tri[2, m], vm.centres(first[m], size[m], count[m]), F(size[m]) * F(0.5))
                probe.probe_vox_interval(tri[0, m], tri[1, m], tri[2, m], F(first[m]), F(size[m]), count[m], out.ctypes.data)
                lo, hi = int(out[0]), int(out[1])
                got = np.zeros(count[m], bool)
                got[lo:max(lo, hi)] = True
                assert hi <= count[m] and np.array_equal(got, ok), (name, tri.tolist(), m, lo, hi, np.flatnonzero(ok))
                empties += not ok.any()
    assert empties > 50                                                           # wholly outside along some axis: covered


def test_probe_raster_matches_model_on_whole_grids(probe):
    """intervals + column clauses + cell clauses, the way the kernel strings them together, against the model's plain evaluation"""
    for name, tris, (first, size, count) in _interval_cases():
        want, _ = vm.surface(tris, first, size, count)
        assert np.array_equal(_probe_surface(probe, tris, first, size, count), want), name
    b = meshes.blob(12, 9)
    first, size, count = _padded_grid(b[0], (9, 8, 7))
    tris = vm.triangles_of(*b)
    assert np.array_equal(vm.surface(tris, first, size, count)[0], vm.surface_all_pairs(tris, first, size, count))


# ---- 3. an exact case -------------------------------------------------------------------------------------------------------------------------
def test_square_between_two_layers_sets_both_and_nothing_else(probe):
    # cells of size 2^-3 from 0 on; the square [0.25, 0.75]^2 in the plane z = 0.5, the boundary between layers 3 and 4
    first, size, count = np.full(3, 0.0625, F), np.full(3, 0.125, F), (8, 8, 8)
    sq = np.array([[[0.25, 0.25, 0.5], [0.75, 0.25, 0.5], [0.75, 0.75, 0.5]], [[0.25, 0.25, 0.5], [0.75, 0.75, 0.5], [0.25, 0.75, 0.5]]], F)
    occ, _ = vm.surface(sq, first, size, count)
    want = np.zeros(count, np.uint8)
    want[1:7, 1:7, 3:5] = 1            # closed boxes: the cells [0.125, 0.25] and [0.75, 0.875] touch the square's border
    assert np.array_equal(occ, want) and occ.sum() == 6 * 6 * 2
    assert np.array_equal(_probe_surface(probe, sq, first, size, count), want)


# ---- 4. conservative and tight against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube 16", "cube odd", "blob-192", "blob-6144"])
def test_conservative_and_tight_against_f64(probe, name):
    v, idx, count = {"cube 16": (*meshes.cube(), (16, 16, 16)), "cube odd": (*meshes.cube(), (17, 13, 33)),
                     "blob-192": (*meshes.blob(12, 9), (32, 32, 32)), "blob-6144": (*meshes.blob(48, 65), (40, 24, 33))}[name]
    first, size, count = _padded_grid(v, count)
    tris = vm.triangles_of(v, idx)
    occ = _probe_surface(probe, tris, first, size, count)
    assert np.array_equal(occ, vm.surface(tris, first, size, count)[0])
    sure_in, sure_out = vm.classify64(tris, first, size, count)
    assert not (sure_in & sure_out).any()
    assert occ[sure_in].all(), f"{(occ[sure_in] == 0).sum()} cells that pass every clause by the margin are clear"
    assert not occ[sure_out].any(), f"{occ[sure_out].sum()} cells that miss a clause by the margin are set"
    unclassified = int((~sure_in & ~sure_out).sum())
    assert unclassified <= 0.005 * occ.sum(), (unclassified, int(occ.sum()))


def test_layouts_of_the_model():
    occ = (np.arange(3 * 2 * 65).reshape(3, 2, 65) % 7 == 0).astype(np.uint8)
    bits = vm.pack_bits(occ)
    assert bits.shape == (3, 2, 3) and np.array_equal(vm.unpack_bits(bits, 65), occ)
    assert (bits[:, :, 2] >> 1 == 0).all()                                        # one live bit in the last word
    assert bits[0, 0, 0] & 1 == 1 and (bits[0, 0, 0] >> 7) & 1 == 1


# ---- 5. the library: exports and argument checks that need no device ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


def test_new_entry_points_are_exported(lib):
    for name in ("m2s_voxelize", "m2s_mesh_voxelize"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    hdr = open(os.path.join(ROOT, "include", "m2s.h")).read()
    assert "typedef struct m2s_voxelize_opts" in hdr and "M2S_VOXELIZE_SOLID = 1" in hdr
    assert "#define M2S_VERSION_MINOR 5" in hdr
    assert C.sizeof(_lib.M2SVoxelizeOpts) == 8
    assert lib.m2s_version() == 5


def _opts(**kw):
    o = _lib.M2SOpts()
    o.struct_size = C.sizeof(_lib.M2SOpts)
    o.device = -1
    o.synchronous = 1
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _grid(first=(0.125,) * 3, size=(0.25,) * 3, count=(4, 4, 4)):
    g = _lib.M2SGrid()
    for k in range(3):
        g.first_cell[k], g.cell_size[k], g.cell_count[k] = first[k], size[k], count[k]
    return g


def test_bad_arguments_fail_before_the_device(lib):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    idx = np.array([0, 1, 2, 0, 2, 3], np.uint32)
    bits, occ, cells = np.zeros(16, np.uint32), np.zeros(64, np.uint8), np.zeros(64, np.uint64)
    count = C.c_uint64(77)
    V, I = v.ctypes.data, idx.ctypes.data
    outs = [bits.ctypes.data, occ.ctypes.data, cells.ctypes.data, 64, C.byref(count)]
    BAD = _lib.ERR_BAD_ARG
    vx, mvx = lib.m2s_voxelize, lib.m2s_mesh_voxelize
    g = _grid()
    G = C.byref(g)
    vo = lambda size=8, mode=0: C.byref(_lib.M2SVoxelizeOpts(size, mode))        # noqa: E731
    assert vx(V, 4, I, 6, 4, 0, G, None, None, None, None, 0, None, None) == BAD                     # all four outputs NULL
    assert "NULL" in _lib.last_error()
    assert vx(V, 4, I, 6, 4, 0, None, None, *outs, None) == BAD                                      # NULL grid
    assert mvx(None, G, None, *outs, None) == BAD                                                    # NULL mesh
    for bad in (_grid(count=(0, 4, 4)), _grid(count=(4, 4, 0)), _grid(count=(2 ** 31, 1, 1)), _grid(count=(2 ** 17, 2 ** 17, 1)),
                _grid(count=(2 ** 13, 2 ** 13, 2 ** 13)),
                _grid(size=(0.25, 0.0, 0.25)), _grid(size=(-0.25, 0.25, 0.25)), _grid(size=(0.25, 0.25, float("inf"))),
                _grid(size=(float("nan"), 0.25, 0.25)), _grid(first=(0, float("nan"), 0)), _grid(first=(float("-inf"), 0, 0))):
        assert vx(V, 4, I, 6, 4, 0, C.byref(bad), None, *outs, None) == BAD, (list(bad.cell_count), list(bad.cell_size), list(bad.first_cell))
    for o in (vo(mode=2), vo(mode=0xFFFFFFFF), vo(size=4), vo(size=16), vo(size=0)):
        assert vx(V, 4, I, 6, 4, 0, G, o, *outs, None) == BAD
    for field, value in (("x_begin", 1), ("x_end", 2), ("x_period", 4), ("n_peer_out", 1), ("mem_kind", 5), ("algorithm", 2)):
        assert vx(V, 4, I, 6, 4, 0, G, None, *outs, C.byref(_opts(**{field: value}))) == BAD, field
    assert vx(V, 4, I, 6, 3, 0, G, None, *outs, None) == BAD                                         # index_bytes
    assert vx(V, 4, I, 6, 4, 7, G, None, *outs, None) == BAD                                         # topology
    assert vx(None, 4, I, 6, 4, 0, G, None, *outs, None) == BAD                                      # NULL vertices
    bad_idx = np.array([0, 1, 2, 0, 2, 4], np.uint32)
    assert vx(V, 4, bad_idx.ctypes.data, 6, 4, 0, G, None, *outs, None) == BAD                       # vertex index out of range
    assert "out of range" in _lib.last_error()
    assert count.value == 77                                                                          # no failed check writes *n_set_out
    with pytest.raises(M2SPanic):
        voxelize(v, Topology.TriangleList(idx), Grid([0, 0, 0], [0.25, 0.25, 0.25], [4, 0, 4]))
    with pytest.raises(M2SPanic):
        voxelize(v, Topology.TriangleList(bad_idx), Grid([0, 0, 0], [0.25, 0.25, 0.25], [4, 4, 4]))


def test_an_empty_mesh_needs_a_device_like_its_siblings(lib):
    """Nothing is decided early for a mesh without triangles: the outputs still have to be cleared on the device's side.  Where there is
    no device the call fails with M2S_ERR_HIP; where there is one it sets nothing."""
    import torch

    v = np.zeros((2, 3), F)
    occ, count = np.ones(64, np.uint8), C.c_uint64(77)
    g = _grid()
    rc = lib.m2s_voxelize(v.ctypes.data, 2, None, 0, 4, 0, C.byref(g), None, None, occ.ctypes.data, None, 0, C.byref(count), None)
    if torch.cuda.is_available():
        assert rc == _lib.M2S_OK and count.value == 0 and not occ.any()
    else:
        assert rc == _lib.ERR_HIP
        with pytest.raises(M2SError):
            voxelize(v, Topology.TriangleList(), Grid([0, 0, 0], [0.25, 0.25, 0.25], [4, 4, 4]))


def _compile(tmp_path, cc, std, src, extra=()):
    exe = str(tmp_path / os.path.basename(src).split(".")[0])
    subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                           os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", *extra, "-o", exe])
    return exe


@pytest.mark.parametrize("cc,std,src", [("gcc", "-std=c99", "tests/c/voxelize_smoke.c"), ("g++", "-std=c++17", "tests/cpp/voxelize_tests.cpp")])
def test_headers_compile_and_the_early_answers_hold(lib, tmp_path, cc, std, src):
    """The C and C++ headers with the new declarations, from consumers of their own; run without arguments the programs ask only what is
    decided before any device work."""
    if not shutil.which(cc):
        pytest.skip("no " + cc)
    exe = _compile(tmp_path, cc, std, src, ["-lm"] if cc == "gcc" else [])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
