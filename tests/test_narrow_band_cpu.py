"""m2s_narrow_band_sdf without a GPU: the exports and the header, every argument check that is decided before device work, the consumers,
the host build of the candidate predicate (band.hip.h through libm2s_probe.so) against its numpy restatement (tests/band_model.py), and the
property the whole call rests on: every cell whose oracle distance is within the band is a candidate."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import band_model as bm
import oracle as orc
import sample_model as sm
from mesh_to_sdf_amd import Grid, M2SPanic, NarrowBand, SignMethod, Topology, _lib, meshes, narrow_band_sdf

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def probe():
    p = C.CDLL(os.path.join(ROOT, "mesh_to_sdf_amd", "libm2s_probe.so"))
    p.probe_band_reach.restype = C.c_float
    p.probe_band_reach.argtypes = [C.c_float, C.c_float]
    p.probe_band_plane.restype = C.c_int
    p.probe_band_plane.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    p.probe_band_box.restype = C.c_int
    p.probe_band_box.argtypes = [C.c_void_p, C.c_void_p]
    p.probe_band_candidates.restype = None
    p.probe_band_candidates.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p]
    return p


def _triangles(v, idx):
    return np.ascontiguousarray(np.asarray(v, F)[np.asarray(idx).reshape(-1, 3)].reshape(-1, 9))


def _padded_grid(v, count, frac=0.1):
    lo, hi = meshes.extended_bbox(v, frac)
    first, size, count = meshes.grid_from_bounding_box(lo, hi, count)
    return np.asarray(first, F), np.asarray(size, F), tuple(int(c) for c in count)


def _probe_candidates(probe, tris, first, size, count, r):
    tris = np.ascontiguousarray(tris, F).reshape(-1, 9)
    occ = np.zeros(count, np.uint8)
    if np.isinf(r):
        return np.ones(count, np.uint8)           # the library takes this branch before any triangle is looked at
    n = np.asarray(count, np.uint32)
    probe.probe_band_candidates(tris.shape[0], tris.ctypes.data, first.ctypes.data, size.ctypes.data, n.ctypes.data, F(r), bm.grid_scale(first, size, count),
                                occ.ctypes.data)
    return occ


# ---- 1. exports, header, version -------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_exported(lib):
    for name in ("m2s_narrow_band_sdf", "m2s_mesh_narrow_band_sdf"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    hdr = open(os.path.join(ROOT, "include", "m2s.h")).read()
    assert "typedef struct m2s_band_opts" in hdr and "float exterior;" in hdr and "float interior;" in hdr
    assert "#define M2S_VERSION_MINOR 5" in hdr
    assert C.sizeof(_lib.M2SBandOpts) == 12
    assert lib.m2s_version() == 5
    assert "M2S_BAND_CHUNK" in _lib.describe_knobs()


# ---- 2. argument checks that need no device -------------------------------------------------------------------------------------------------
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
    bits, cells, dist = np.zeros(16, np.uint32), np.zeros(64, np.uint64), np.zeros(64, F)
    count = C.c_uint64(77)
    V, I = v.ctypes.data, idx.ctypes.data
    outs = [cells.ctypes.data, dist.ctypes.data, 64, bits.ctypes.data, C.byref(count)]
    BAD = _lib.ERR_BAD_ARG
    nb, mnb = lib.m2s_narrow_band_sdf, lib.m2s_mesh_narrow_band_sdf
    g = _grid()
    G = C.byref(g)
    bo = lambda ext=0.5, inte=0.5, size=12: C.byref(_lib.M2SBandOpts(size, ext, inte))        # noqa: E731
    assert nb(V, 4, I, 6, 4, 0, G, 1, bo(), None, None, 0, None, None, None) == BAD                  # all four outputs NULL
    assert "NULL" in _lib.last_error()
    assert nb(V, 4, I, 6, 4, 0, None, 1, bo(), *outs, None) == BAD                                   # NULL grid
    assert mnb(None, G, 1, bo(), *outs, None) == BAD                                                 # NULL mesh
    assert nb(V, 4, I, 6, 4, 0, G, 1, None, *outs, None) == BAD                                      # NULL widths
    for sign in (-1, 2, 7):
        assert nb(V, 4, I, 6, 4, 0, G, sign, bo(), *outs, None) == BAD, sign
    for bad in (_grid(count=(0, 4, 4)), _grid(count=(4, 4, 0)), _grid(count=(2 ** 31, 1, 1)), _grid(count=(2 ** 17, 2 ** 17, 1)),
                _grid(count=(2 ** 13, 2 ** 13, 2 ** 13)),
                _grid(size=(0.25, 0.0, 0.25)), _grid(size=(-0.25, 0.25, 0.25)), _grid(size=(0.25, 0.25, INF)),
                _grid(size=(float("nan"), 0.25, 0.25)), _grid(first=(0, float("nan"), 0)), _grid(first=(-INF, 0, 0))):
        assert nb(V, 4, I, 6, 4, 0, C.byref(bad), 1, bo(), *outs, None) == BAD, (list(bad.cell_count), list(bad.cell_size), list(bad.first_cell))
    for o in (bo(ext=-0.5), bo(inte=-1e-30), bo(ext=float("nan")), bo(inte=float("nan")), bo(ext=-INF), bo(size=8), bo(size=16), bo(size=0)):
        assert nb(V, 4, I, 6, 4, 0, G, 1, o, *outs, None) == BAD
    for field, value in (("x_begin", 1), ("x_end", 2), ("x_period", 4), ("n_peer_out", 1), ("mem_kind", 5), ("algorithm", 2)):
        assert nb(V, 4, I, 6, 4, 0, G, 0, bo(), *outs, C.byref(_opts(**{field: value}))) == BAD, field
    assert nb(V, 4, I, 6, 3, 0, G, 0, bo(), *outs, None) == BAD                                      # index_bytes
    assert nb(V, 4, I, 6, 4, 7, G, 0, bo(), *outs, None) == BAD                                      # topology
    assert nb(None, 4, I, 6, 4, 0, G, 0, bo(), *outs, None) == BAD                                   # NULL vertices
    bad_idx = np.array([0, 1, 2, 0, 2, 4], np.uint32)
    assert nb(V, 4, bad_idx.ctypes.data, 6, 4, 0, G, 0, bo(), *outs, None) == BAD                    # vertex index out of range
    assert "out of range" in _lib.last_error()
    assert count.value == 77                                                                          # no failed check writes *n_active_out
    with pytest.raises(M2SPanic):
        narrow_band_sdf(v, Topology.TriangleList(idx), Grid([0, 0, 0], [0.25, 0.25, 0.25], [4, 4, 4]), -1.0)
    with pytest.raises(M2SPanic):
        narrow_band_sdf(v, Topology.TriangleList(idx), Grid([0, 0, 0], [0.25, 0.25, 0.25], [4, 0, 4]), (0.5, INF), SignMethod.Normal)


def test_narrow_band_views():
    grid = Grid([0, 0, 0], [0.5, 0.5, 0.5], [2, 3, 4])
    b = NarrowBand(np.array([1, 7, 23], np.uint64), np.array([-0.5, 0.25, 1.0], F), None, 3, grid)
    assert b.ijk().tolist() == [[0, 0, 1], [0, 1, 3], [1, 2, 3]]
    d = b.to_dense()
    assert d.shape == (2, 3, 4) and d.dtype == F and np.isnan(d).sum() == 21 and d[0, 1, 3] == F(0.25) and d[1, 2, 3] == 1.0
    assert (b.to_dense(fill=9.0) == 9.0).sum() == 21


# ---- 3. the consumers compile --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cc,std,src", [("gcc", "-std=c99", "tests/c/narrow_band_smoke.c"), ("g++", "-std=c++17", "tests/cpp/narrow_band_tests.cpp")])
def test_consumers_compile_and_check_their_arguments(lib, tmp_path, cc, std, src):
    exe = str(tmp_path / os.path.basename(src).split(".")[0])
    subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                           os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


# ---- 4. the host build of the predicate is the model ----------------------------------------------------------------------------------------------
def test_probe_pieces_match_the_model(probe):
    rng = np.random.default_rng(5)
    for r, scale in [(0.0, 0.0), (0.0, 1.0e4), (0.37, 1.5), (3.0e19, 2.0), (1.0e30, 1.0e30), (F(1.5e-3), F(17.25))] + [tuple(x) for x in rng.random((50, 2)) * 10]:
        assert np.array_equal(F(probe.probe_band_reach(F(r), F(scale))).view(np.uint32), bm.reach(r, scale).view(np.uint32)), (r, scale)
    tri = rng.standard_normal((20, 9)).astype(F)
    tri[1, 4] = np.nan
    tri[2, 0] = np.inf
    tri[3, [0, 3, 6]] = np.nan                                                     # no finite vertex
    tri[4, [1, 8]] = -np.inf                                                       # one finite vertex
    for t in tri:
        out = np.zeros(7, F)
        any_ = probe.probe_band_box(np.ascontiguousarray(t).ctypes.data, out.ctypes.data)
        lo, hi, amax, want_any = bm.box(t)
        assert bool(any_) == want_any and np.array_equal(out[:3], lo) and np.array_equal(out[3:6], hi) and out[6] == amax, t
    assert not bm.box(tri[3])[3] and bm.box(tri[4])[3]
    first, size, count = np.array([-1.5, 0.25, 1e3], F), np.array([0.125, 0.3, 0.01], F), np.array([20, 7, 300], np.uint32)
    tri[5] = [0, 0, 0, 1, 0, 0, 2, 0, 0]                                            # zero area
    tri[6, 6:] = tri[6, :3]                                                        # c == a
    for t in tri:
        out = np.zeros(4, F)
        use = probe.probe_band_plane(np.ascontiguousarray(t).ctypes.data, F(0.37), first.ctypes.data, size.ctypes.data, count.ctypes.data, out.ctypes.data)
        _, n, rhs, want_use = bm.plane(t, F(0.37), first, size, tuple(int(c) for c in count))
        assert bool(use) == want_use
        if want_use:
            assert np.array_equal(out[:3].view(np.uint32), n.view(np.uint32)) and np.array_equal(out[3:].view(np.uint32), np.array([rhs], F).view(np.uint32)), t


@pytest.fixture(scope="module")
def small_meshes(suzanne):
    b12 = meshes.blob(12, 9)
    far = np.array([1.0e4, -1.0e4, 1.0e4], F)
    return {"cube": meshes.cube(), "suzanne": suzanne, "blob-192": b12, "blob-192-far": ((b12[0] + far).astype(F), b12[1])}


def test_probe_raster_matches_the_model_on_awkward_triangles(probe, small_meshes):
    b12 = small_meshes["blob-192"]
    nan = b12[0].copy()
    nan[7, 1] = np.nan
    inf = b12[0].copy()
    inf[3, 0] = np.inf
    cases = {"degenerates": sm.with_degenerates(*b12), "one-huge": sm.one_huge(*b12), "nan-vertex": (nan, b12[1]), "inf-vertex": (inf, b12[1]),
             "larger-than-the-grid": (np.array([[-50, -60, -9], [80, -10, 7], [-20, 90, 6]], F), np.array([0, 1, 2]))}
    first, size, count = _padded_grid(b12[0], (20, 12, 33))
    for name, (v, idx) in cases.items():
        tris = _triangles(v, idx)
        for cells in (0.0, 0.75, 2.5):
            r = F(cells) * size.max()
            got, want = _probe_candidates(probe, tris, first, size, count, r), bm.candidates(tris, first, size, count, r)
            assert np.array_equal(got, want), (name, cells, int(got.sum()), int(want.sum()))
            assert cells == 0.0 or 0 < want.sum(), (name, cells)
    # a triangle that loses a vertex to NaN keeps the box of the other two, and the vertex itself when two are lost
    t = np.array([[0, 0, 0, 1, 0, 0, np.nan, 1, 0]], F)
    g = (np.full(3, -0.875, F), np.full(3, 0.25, F), (12, 8, 8))
    assert np.array_equal(_probe_candidates(probe, t, *g, F(0.3)), bm.candidates(np.array([[0, 0, 0, 1, 0, 0, 1, 0, 0]], F), *g, F(0.3)))


# ---- 5. conservative against the oracle, and not everything ------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [(16, 16, 16), (33, 20, 31)], ids=["16^3", "33x20x31"])
@pytest.mark.parametrize("name", ["cube", "suzanne", "blob-192", "blob-192-far"])
def test_every_cell_within_the_band_is_a_candidate(probe, small_meshes, name, count):
    """The oracle's unsigned distances at the cell centres (the reference's own arithmetic on the CPU): every cell with distance <= r must be in
    the probe's candidate set, for r = 0, 0.5, 1.5 and 3 widths of the largest cell.  The ratio candidates / active is printed for every case,
    so that a raster that marks everything does not pass silently, and on the blob at 1.5 cells the candidates must stay below half the grid.
    That bound is asserted on 33 x 20 x 31, where the oracle's own active cells are 32 % of the grid; on 16^3 they are 48 % by themselves
    (a shell of +-1.5 cells around a ball 13 cells across), so a superset would have to overshoot by less than 1.6 % of the grid to stay
    under one half; the candidates there are 2446 cells, 59.7 %.  The translated copy is printed only: its
    slack of 4e-6 x 1e4 = 0.04 is a quarter of a cell on every side (50.5 % of the grid)."""
    v, idx = small_meshes[name]
    first, size, count = _padded_grid(v, count)
    d = np.abs(orc.generate_grid_sdf(v, idx, first, size, count, sign=0, semantics=orc.EXACT)).reshape(count)
    tris = _triangles(v, idx)
    for cells in (0.0, 0.5, 1.5, 3.0):
        r = F(cells) * size.max()
        cand = _probe_candidates(probe, tris, first, size, count, r)
        assert np.array_equal(cand, bm.candidates(tris, first, size, count, r)), (name, cells)
        active = d <= r
        missed = active & (cand == 0)
        assert not missed.any(), f"{name} at {cells} cells: {int(missed.sum())} active cells are no candidates, first {np.argwhere(missed)[:3].tolist()}"
        print(f"{name} {count} r = {cells} cells: candidates {int(cand.sum())}, active {int(active.sum())}, ratio "
              f"{cand.sum() / max(1, active.sum()):.2f}, of the grid {cand.mean():.3f}")
        if name == "blob-192" and cells == 1.5 and count == (33, 20, 31):
            assert 0 < active.sum() < cand.size / 3 and cand.sum() < 0.5 * cand.size, (int(active.sum()), int(cand.sum()), cand.size)
    assert _probe_candidates(probe, tris, first, size, count, INF).all()


def test_tiny_triangles_take_no_plane_test(probe):
    """Below |n|^2 = 1e-30 the squares of the normal's components underflow and the computed |n| falls short of the true one, so the plane
    test is switched off there and the box alone decides.  A right triangle with legs of 1e-12 in a 10^3 grid of 1e-12 cells at r = 3 cells:
    every cell whose float64 distance is within r must be a candidate; with legs of 1e-6 the plane test is on and the same must hold."""
    for s, plane_on in ((1.0e-12, False), (1.0e-9, False), (1.0e-6, True)):
        tri = np.array([[0, 0, 0, s, 0, 0, 0, s, 0]], F)
        first, size, count = np.full(3, -4.5 * s, F), np.full(3, s, F), (10, 10, 10)
        r = F(3.0 * s)
        assert bm.plane(tri[0], bm.reach(r, 5 * s), first, size, count)[3] == plane_on
        cand = _probe_candidates(probe, tri, first, size, count, r)
        assert np.array_equal(cand, bm.candidates(tri, first, size, count, r))
        q = [np.asarray(bm.centres(first[m], size[m], count[m]), np.float64) / s for m in range(3)]      # in units of s: the triangle (0,0,0) (1,0,0) (0,1,0)
        X, Y, Z = np.meshgrid(*q, indexing="ij")
        # distance to the triangle in the plane z = 0: clamp to the triangle by its three half planes
        px, py = np.clip(X, 0, None), np.clip(Y, 0, None)
        over = px + py > 1
        tt = np.clip((px - py + 1) / 2, 0, 1)
        px, py = np.where(over, tt, px), np.where(over, 1 - tt, py)
        dist = np.sqrt((X - px) ** 2 + (Y - py) ** 2 + Z ** 2)
        active = dist <= 3.0
        assert active.sum() > 100 and cand[active].all(), (s, int(active.sum()), int(cand[active].sum()))
        assert cand.sum() < cand.size
