"""m2s_grid_isosurface without a GPU: the generated table (tools/gen_isosurface_table.py) against its committed header and its rule on
all 256 cases, including the crack-free proof across shared faces; the test oracle tests/isosurface_model.py on analytic fields;
the exported symbol and the argument checks that fail before any device work; the new C and C++ programs compile."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import isosurface_model as im
from isosurface_model import gen
from mesh_to_sdf_amd import _lib
from mesh_to_sdf_amd.api import Grid, M2SPanic, grid_isosurface

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the table -------------------------------------------------------------------------------------------------------------------
def test_regenerating_the_table_reproduces_the_header():
    with open(gen.HEADER) as f:
        assert f.read() == gen.render()


def _crossing_edges(case):
    ins = lambda c: (case >> c) & 1
    return {e for e in range(12) if ins(gen.edge_corners(e)[0]) != ins(gen.edge_corners(e)[1])}


@pytest.mark.parametrize("case", range(256))
def test_every_crossing_edge_is_on_exactly_one_loop(case):
    loops = gen.loops(case)
    used = [e for lp in loops for e in lp]
    assert sorted(used) == sorted(_crossing_edges(case))
    assert [lp[0] for lp in loops] == sorted(lp[0] for lp in loops) and all(lp[0] == min(lp) for lp in loops)
    tris = gen.TABLE[case]
    assert len(tris) == sum(len(lp) - 2 for lp in loops) <= gen.MAX_TRIS
    # the fan: the triangles' boundary (directed edges used once) is exactly the loops' segments
    seg = {(lp[i], lp[(i + 1) % len(lp)]) for lp in loops for i in range(len(lp))}
    dir_edges = [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]
    boundary = {e for e in dir_edges if (e[1], e[0]) not in dir_edges}
    assert boundary == seg


@pytest.mark.parametrize("case", range(256))
def test_face_segments_follow_the_face_rule(case):
    ins = lambda c: (case >> c) & 1
    for face in gen.FACES:
        segs = gen.face_segments(case, face)
        crossing = [e for e in gen.face_edges(face) if e in _crossing_edges(case)]
        assert sorted(e for s in segs for e in s) == sorted(crossing)
        inside = [c for c in gen.face_corners(face) if ins(c)]
        if len(crossing) == 4:
            # ambiguous: the two inside corners are on a diagonal and each is cut off on its own
            assert len(inside) == 2 and len(segs) == 2
            for a, b in segs:
                shared = set(gen.edge_corners(a)) & set(gen.edge_corners(b))
                assert len(shared) == 1 and ins(shared.pop())
        for a, b in segs:   # inside corners on the right, seen from outside
            f, s = face
            n = [0, 0, 0]
            n[f] = 1 if s else -1
            ma, mb = np.array(gen.edge_mid(a)), np.array(gen.edge_mid(b))
            for c in gen.face_corners(face):
                side = np.dot(np.cross(n, mb - ma), np.array(gen.corner_pos(c)) - ma)
                near = c in gen.edge_corners(a) or c in gen.edge_corners(b)
                if near and side != 0:
                    assert (side < 0) == bool(ins(c)), (case, face, a, b, c)


def _face_signature(case, face):
    """The face's four signs, keyed by the in-plane corner position."""
    f, _ = face
    out = {}
    for c in gen.face_corners(face):
        p = list(gen.corner_pos(c))
        p.pop(f)
        out[tuple(p)] = (case >> c) & 1
    return out


def _segment_coords(segs, face):
    """Segments as pairs of in-plane edge midpoints (the face's coordinate dropped)."""
    f, _ = face
    drop = lambda m: tuple(v for k, v in enumerate(m) if k != f)
    return {(drop(gen.edge_mid(a)), drop(gen.edge_mid(b))) for a, b in segs}


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_shared_faces_agree_in_opposite_directions(axis):
    # cell A's upper face on `axis` is cell B's lower face: for every pair of cases that agree on it, the segments are the same
    # in opposite directions, so the mesh has no crack there
    up, low = (axis, 1), (axis, 0)
    for a in range(256):
        sig = _face_signature(a, up)
        sa = _segment_coords(gen.face_segments(a, up), up)
        for b in range(256):
            if _face_signature(b, low) != sig:
                continue
            sb = _segment_coords(gen.face_segments(b, low), low)
            assert sa == {(q, p) for p, q in sb}, (axis, a, b)


# ---- the model on analytic fields ------------------------------------------------------------------------------------------------
def _field(g, fn):
    x, y, z = (g.coord(a, np.arange(g.n[a])).astype(np.float64) for a in range(3))
    return fn(x[:, None, None], y[None, :, None], z[None, None, :]).astype(F)


def _closed_once(tris):
    missing, dup = im.open_edges(tris)
    return missing.shape[0] == 0 and not dup


@pytest.mark.parametrize("n,iso", [(16, 0.0), (29, 0.05), (40, -0.1), (64, 0.0)])
def test_sphere_is_closed_outward_and_of_the_right_volume(n, iso):
    c, r = np.array([0.07, -0.04, 0.03]), 0.7
    g = im.GridI([-1.1, -1.05, -1.0], [2.2 / n, 2.2 / n, 2.1 / n], [n, n + 1, n + 2])
    d = _field(g, lambda x, y, z: np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r)
    v, t = im.extract(g, d, iso)
    assert _closed_once(t)
    assert im.euler(len(v), t) == 2
    nrm = im.normals(v, t)
    assert (np.einsum("ij,ij->i", nrm, v[t].mean(1) - c) > 0).all()
    h = float(g.cs.max())
    want = 4 / 3 * np.pi * (r + iso) ** 3
    assert abs(im.volume(v, t) - want) < 4 * np.pi * (r + iso) ** 2 * h * 0.5


def test_torus_has_euler_characteristic_zero():
    g = im.GridI([-1.5] * 3, [3.0 / 48] * 3, [48, 48, 48])
    d = _field(g, lambda x, y, z: np.sqrt((np.sqrt(x ** 2 + y ** 2) - 0.8) ** 2 + z ** 2) - 0.3)
    v, t = im.extract(g, d)
    assert _closed_once(t) and im.euler(len(v), t) == 0


def test_inside_at_the_boundary_leaves_an_open_rim_on_boundary_points():
    # a slab |z - 0.5| < 0.3 that runs through the whole x / y extent: the surface reaches the grid's x / y faces
    g = im.GridI([0, 0, 0], [0.1, 0.1, 0.1], [12, 13, 11])
    d = _field(g, lambda x, y, z: np.abs(z - 0.5) - 0.3 + 0 * x + 0 * y)
    v, t = im.extract(g, d)
    missing, dup = im.open_edges(t)
    assert not dup and missing.shape[0] > 0
    ends = v[missing.reshape(-1)]
    on_boundary = (ends[:, 0] == g.coord(0, 0)) | (ends[:, 0] == g.coord(0, g.n[0] - 1)) | \
                  (ends[:, 1] == g.coord(1, 0)) | (ends[:, 1] == g.coord(1, g.n[1] - 1))
    assert on_boundary.all()


def test_random_fields_are_closed_and_ambiguous_faces_are_the_only_doubled_edges():
    rng = np.random.default_rng(3)
    for _ in range(4):
        g = im.GridI([0, 0, 0], [1, 1, 1], [10, 11, 12])
        d = rng.standard_normal(g.n).astype(F)
        d[[0, -1]] = 1
        d[:, [0, -1]] = 1
        d[:, :, [0, -1]] = 1
        v, t = im.extract(g, d)
        e = im.directed_edges(t)
        n = len(v)
        fwd = np.bincount(e[:, 0] * n + e[:, 1], minlength=n * n)
        assert np.array_equal(fwd, fwd.reshape(n, n).T.reshape(-1))   # every directed edge as often as its reverse
        a, b = np.nonzero(fwd.reshape(n, n) > 1)
        # a doubled edge joins two vertices on one grid plane: the fan diagonals of the two cells beside an ambiguous face
        same_plane = ((v[a] == v[b]) & np.isin(v[a], np.arange(12, dtype=F))).any(1)
        assert same_plane.all() and (fwd <= 2).all()


def test_plane_at_45_degrees_matches_a_scalar_transliteration():
    g = im.GridI([0.1, -0.2, 0.05], [0.13, 0.11, 0.17], [9, 7, 8])
    d = _field(g, lambda x, y, z: (x + y) * np.sqrt(0.5) + 0.05 * z - 0.3)
    for iso in (0.0, 0.04, -0.1):
        v, t = im.extract(g, d, iso)
        want = []
        nx, ny, nz = g.n
        for i in range(nx):
            for j in range(ny):
                for k in range(nz):
                    for a, (di, dj, dk) in enumerate([(1, 0, 0), (0, 1, 0), (0, 0, 1)]):
                        if i + di >= nx or j + dj >= ny or k + dk >= nz:
                            continue
                        d0, d1 = d[i, j, k], d[i + di, j + dj, k + dk]
                        if (d0 < F(iso)) == (d1 < F(iso)):
                            continue
                        p = [F(g.first[ax] + F(idx) * g.cs[ax]) for ax, idx in enumerate((i, j, k))]
                        idx1 = (i, j, k)[a] + 1
                        p1 = F(g.first[a] + F(idx1) * g.cs[a])
                        tt = F(F(F(iso) - d0) / F(d1 - d0))
                        p[a] = F(p[a] + F(tt * F(p1 - p[a])))
                        want.append(p)
        assert np.array_equal(v, np.array(want, F).reshape(-1, 3))
        assert len(t) > 0


def test_slab_model_equals_the_whole():
    g = im.GridI([-1, -1, -1], [0.1, 0.1, 0.1], [21, 20, 19])
    d = _field(g, lambda x, y, z: np.sqrt(x ** 2 + 1.3 * y ** 2 + z ** 2) - 0.75)
    v, t = im.extract(g, d)
    for x0, x1 in [(0, 5), (5, 11), (11, 21), (19, 21)]:
        vb, pv, tb, tt = im.extract_slab(g, lambda a, b: d[a:b], 0.0, x0, x1, chunk=3)
        assert np.array_equal(pv, v[vb:vb + len(pv)]) and np.array_equal(tt, t[tb:tb + len(tt)])


def test_a_grid_with_one_layer_has_vertices_and_no_triangles():
    g = im.GridI([0, 0, 0], [1, 1, 1], [1, 6, 5])
    d = _field(g, lambda x, y, z: y + z - 4.5 + 0 * x)
    v, t = im.extract(g, d)
    assert len(v) > 0 and len(t) == 0


# ---- argument checks that need no device ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


def test_the_entry_point_is_exported(lib):
    assert "m2s_grid_isosurface" in _lib.EXPORTS and hasattr(lib, "m2s_grid_isosurface")


def test_bad_arguments_fail_before_the_device(lib):
    g = Grid.from_bounding_box([0, 0, 0], [1, 1, 1], [4, 4, 4])
    G = C.byref(g._g)
    d = np.zeros(64, F)
    D = d.ctypes.data
    v, t = np.zeros((8, 3), F), np.zeros((8, 3), np.uint32)
    V, T = v.ctypes.data, t.ctypes.data
    cnt = (C.c_uint64 * 2)()
    BAD = _lib.ERR_BAD_ARG
    iso = lib.m2s_grid_isosurface
    assert iso(None, D, 0.0, None, 0, None, 0, cnt, None) == BAD                  # NULL grid / distances / counts
    assert iso(G, None, 0.0, None, 0, None, 0, cnt, None) == BAD
    assert iso(G, D, 0.0, None, 0, None, 0, None, None) == BAD
    assert iso(G, D, 0.0, V, 8, None, 8, cnt, None) == BAD                        # exactly one output NULL
    assert iso(G, D, 0.0, None, 8, T, 8, cnt, None) == BAD
    for bad_iso in (float("nan"), float("inf"), -float("inf")):
        assert iso(G, D, bad_iso, None, 0, None, 0, cnt, None) == BAD
    for first, size, count in [([0] * 3, [0.25] * 3, [4, 0, 4]), ([0] * 3, [0.25, 0.0, 0.25], [4] * 3),
                               ([0] * 3, [0.25, -0.25, 0.25], [4] * 3), ([0] * 3, [0.25, np.inf, 0.25], [4] * 3),
                               ([0] * 3, [0.25, 0.25, np.nan], [4] * 3), ([0, np.nan, 0], [0.25] * 3, [4] * 3),
                               ([np.inf, 0, 0], [0.25] * 3, [4] * 3)]:
        bad = Grid(first, size, count)
        assert iso(C.byref(bad._g), D, 0.0, None, 0, None, 0, cnt, None) == BAD, (first, size, count)
    for field, value in [("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4)]:
        o = _lib.M2SOpts()
        o.struct_size = C.sizeof(o)
        o.device = -1
        setattr(o, field, value)
        assert iso(G, D, 0.0, None, 0, None, 0, cnt, C.byref(o)) == BAD, field
    o = _lib.M2SOpts()
    o.struct_size = C.sizeof(o)
    o.device = -1
    peers = (C.c_void_p * 1)()
    o.n_peer_out, o.peer_out = 1, C.cast(peers, type(o.peer_out))
    assert iso(G, D, 0.0, None, 0, None, 0, cnt, C.byref(o)) == BAD
    with pytest.raises(M2SPanic):
        grid_isosurface(g, np.zeros(63, F))                                        # distances do not match the grid


# ---- the declarations compile in C and C++ with -Wall -Werror ---------------------------------------------------------------------
@pytest.mark.parametrize("cc,std,src", [("gcc", "-std=c99", "tests/c/isosurface_smoke.c"), ("g++", "-std=c++17", "tests/cpp/isosurface_tests.cpp")])
def test_declarations_compile(tmp_path, cc, std, src):
    if not shutil.which(cc):
        pytest.skip(f"no {cc}")
    exe = str(tmp_path / os.path.basename(src).split(".")[0])
    subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src),
                           "-L", os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64"]
                          + (["-lm"] if cc == "gcc" else []) + ["-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"),
                                                                 "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert os.path.exists(exe)
