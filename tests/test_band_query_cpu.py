"""m2s_band_create / m2s_band_sample / m2s_band_raymarch without a GPU: the exports and the header, every argument check that is decided
before device work (host-memory lists that do not ascend, run past the grid or hold a NaN included), the consumers, the default-background
rule, and the model tests/band_query_model.py against grid_query_model: all cells active is the dense field, a partly active band is the
dense D' of the definition, support counts the active reads, and the model takes `cells` as they are."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import band_query_model as bqm
import grid_query_model as gqm
from mesh_to_sdf_amd import BandField, Grid, M2SPanic, Mesh, NarrowBand, Voxels, _lib, default_background

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
MODES = (gqm.SNAP, gqm.TRILINEAR, gqm.TETRAHEDRAL)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


# ---- 1. exports, header ------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_exported(lib):
    for name in ("m2s_band_create", "m2s_band_destroy", "m2s_band_info", "m2s_band_sample", "m2s_band_raymarch"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    hdr = " ".join(open(os.path.join(ROOT, "include", "m2s.h")).read().split())
    for text in ("typedef struct m2s_band m2s_band;",
                 "typedef struct m2s_band_field_opts { uint32_t struct_size;",
                 "int m2s_band_create(const m2s_grid* grid, const uint64_t* cells, const float* distances, uint64_t n_cells, const uint32_t* inside_bits",
                 "const m2s_band_field_opts* fopts, const m2s_opts* opts, m2s_band** out);",
                 "void m2s_band_destroy(m2s_band* band);",
                 "int m2s_band_info(const m2s_band* band, m2s_grid* grid, uint64_t* n_cells, uint64_t* device_bytes);",
                 "int m2s_band_sample(const m2s_band* band, const float* points, size_t n_points, const m2s_sample_opts* sopts, float* value_out, "
                 "float* normal_out, uint8_t* support_out, const m2s_opts* opts);",
                 "int m2s_band_raymarch(const m2s_band* band, const float* origins, const float* directions, size_t n_rays, const m2s_sample_opts* sopts, "
                 "float* hit_out, uint32_t* steps_out, float* normal_out, uint8_t* support_out, const m2s_opts* opts);"):
        assert text in hdr, text
    assert C.sizeof(_lib.M2SBandFieldOpts) == 12
    assert lib.m2s_version() == 5
    for cls, names in ((BandField, ("sample", "raymarch", "close", "__enter__", "__exit__", "__del__")), (NarrowBand, ("field",)),
                       (Mesh, ("narrow_band_field",))):
        for name in names:
            assert hasattr(cls, name), (cls, name)
    assert NarrowBand._fields == ("cells", "distances", "bits", "count", "grid")
    hpp = open(os.path.join(ROOT, "include", "mesh_to_sdf.hpp")).read()
    assert "class BandField {" in hpp and "BandField(const BandField&) = delete;" in hpp
    assert "M2S_BAND_FETCH" in _lib.describe_knobs()


# ---- 2. argument checks that need no device ---------------------------------------------------------------------------------------------------
def _opts(**kw):
    o = _lib.M2SOpts()
    o.struct_size = C.sizeof(_lib.M2SOpts)
    o.device = -1
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _fopts(outside=0.5, inside=0.5, size=None):
    return _lib.M2SBandFieldOpts(C.sizeof(_lib.M2SBandFieldOpts) if size is None else size, outside, inside)


def test_create_rejects_bad_arguments_before_the_device(lib):
    g = Grid.from_bounding_box([0, 0, 0], [1, 1, 1], [4, 4, 4])
    G = C.byref(g._g)
    cells, d = np.arange(64, dtype=np.uint64), np.zeros(64, F)
    P, D = cells.ctypes.data, d.ctypes.data
    BAD = _lib.ERR_BAD_ARG
    create = lib.m2s_band_create
    SENTINEL = 0x1234

    def call(grid=G, p=P, dist=D, n=64, bits=None, fo=None, opts=None, want=BAD, out=True):
        h = C.c_void_p(SENTINEL)
        fo = _fopts() if fo is None else fo
        rc = create(grid, p, dist, n, bits, C.byref(fo) if fo is not False else None, opts, C.byref(h) if out else None)
        assert rc == want, (rc, _lib.last_error())
        assert not out or h.value is None            # no handle is returned

    call(grid=None)
    call(out=False)
    call(fo=False)                                    # the backgrounds have no default
    call(p=None)
    call(dist=None)
    call(n=65)
    assert "n_cells" in _lib.last_error()
    for size in (0, 8, 16):
        call(fo=_fopts(size=size))
    for outside, inside in ((-0.5, 0.5), (0.5, -1e-30), (INF, 0.5), (0.5, INF), (float("nan"), 0.5), (0.5, float("nan")), (-INF, 0.5)):
        call(fo=_fopts(outside, inside))
    for first, size, count in [([0] * 3, [0.25] * 3, [4, 0, 4]), ([0] * 3, [0.25, 0.0, 0.25], [4] * 3),
                               ([0] * 3, [0.25, -0.25, 0.25], [4] * 3), ([0] * 3, [0.25, np.inf, 0.25], [4] * 3),
                               ([0] * 3, [0.25, 0.25, np.nan], [4] * 3), ([0, np.nan, 0], [0.25] * 3, [4] * 3),
                               ([np.inf, 0, 0], [0.25] * 3, [4] * 3), ([3.3e38, 0, 0], [1e37] * 3, [4] * 3),   # the box's end is not finite
                               ([0] * 3, [0.25] * 3, [2 ** 12, 2 ** 12, 2 ** 12]),       # 2^36 cells
                               ([0] * 3, [0.25] * 3, [2 ** 40, 2 ** 30, 2 ** 10])]:      # a product that overflows 64 bits
        bad = Grid(first, size, count)
        call(grid=C.byref(bad._g), n=1)
    for field, value in [("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4), ("mem_kind", 5)]:
        call(opts=C.byref(_opts(**{field: value})))
    o = _opts()
    peers = (C.c_void_p * 1)()
    o.n_peer_out, o.peer_out = 1, C.cast(peers, type(o.peer_out))
    call(opts=C.byref(o))
    # host memory: the list and its values are judged on the host
    for bad_cells in ([5, 4, 9], [4, 5, 5], [4, 5, 64], [0, 2 ** 63], [1, 0]):
        c = np.array(bad_cells, np.uint64)
        for o in (None, C.byref(_opts(mem_kind=_lib.MEM_HOST))):
            call(p=c.ctypes.data, n=c.size, opts=o)
            assert "cells[" in _lib.last_error()
    for bad_value in (float("nan"), INF, -INF):
        dd = d.copy()
        dd[17] = bad_value
        call(dist=dd.ctypes.data, want=_lib.ERR_NAN)
        assert "distances[17]" in _lib.last_error()
    # an order error wins over a NaN further on or before it, as in m2s_band_isosurface (the list is judged first)
    dd = d.copy()
    dd[0] = float("nan")
    call(p=np.array([4, 3], np.uint64).ctypes.data, dist=dd.ctypes.data, n=2)


def test_the_queries_reject_a_null_handle_and_python_checks_its_own(lib):
    p = np.zeros((4, 3), F)
    v, s = np.zeros(4, F), np.zeros(4, np.uint8)
    hit, steps = np.zeros((4, 4), F), np.zeros(4, np.uint32)
    assert lib.m2s_band_sample(None, p.ctypes.data, 4, None, v.ctypes.data, None, s.ctypes.data, None) == _lib.ERR_BAD_ARG
    assert "band is NULL" in _lib.last_error()
    assert lib.m2s_band_raymarch(None, p.ctypes.data, p.ctypes.data, 4, None, hit.ctypes.data, steps.ctypes.data, None, None, None) == _lib.ERR_BAD_ARG
    assert lib.m2s_band_info(None, None, None, None) == _lib.ERR_BAD_ARG
    lib.m2s_band_destroy(None)                                                            # a no-op
    g = Grid.from_bounding_box([0, 0, 0], [1, 1, 1], [4, 4, 4])
    d = np.zeros(3, F)
    with pytest.raises(M2SPanic):
        BandField(g, np.array([1, 2], np.uint64), d)                                      # cells and distances differ in length
    with pytest.raises(M2SPanic):
        BandField(g, np.array([3, 2, 5], np.int64), d)
    with pytest.raises(M2SPanic):
        BandField(g, np.array([-1, 2, 5], np.int64), d)                                   # a negative int64 is out of range
    with pytest.raises(M2SPanic):
        BandField(g, np.array([1, 2, 5], np.int64), d, background=-1.0)
    with pytest.raises(M2SPanic):
        BandField(g, np.array([1, 2, 5], np.int64), d, inside=np.zeros(5, np.uint32))     # a sign mask that does not match the grid
    with pytest.raises(M2SPanic):
        BandField(g, np.array([1, 2, 5], np.int64), d, inside=True)                       # True needs the mesh
    with pytest.raises(M2SPanic):
        BandField(g, np.array([1, 2, 5], np.int64), d, inside=Voxels(None, None, None, 0))
    with pytest.raises(M2SPanic):
        NarrowBand(np.array([7, 7], np.uint64), d[:2], None, 2, g).field()


# ---- 3. the consumers compile -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cc,std,src", [("gcc", "-std=c99", "tests/c/band_query_smoke.c"), ("g++", "-std=c++17", "tests/cpp/band_query_tests.cpp")])
def test_consumers_compile_and_check_their_arguments(lib, tmp_path, cc, std, src):
    exe = str(tmp_path / os.path.basename(src).split(".")[0])
    subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                           os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


# ---- 4. the default background ---------------------------------------------------------------------------------------------------------------------
def test_the_default_background_is_the_bands_own_reach():
    assert default_background(np.array([-0.5, 0.125, 0.25], F)) == (0.5, 0.25)            # (inside, outside)
    assert default_background(np.array([0.125, 0.25], F)) == (0.0, 0.25)                  # nothing negative: no inside reach known
    assert default_background(np.array([-0.75, -0.5], F)) == (0.75, 0.0)
    assert default_background(np.zeros(0, F)) == (0.0, 0.0)
    big = np.array([-np.finfo(F).max, np.finfo(F).max], F)
    assert default_background(big) == (float(np.finfo(F).max), float(np.finfo(F).max))
    torch = pytest.importorskip("torch")
    assert default_background(torch.tensor([-0.5, 0.25])) == (0.5, 0.25)


# ---- 5. the model -----------------------------------------------------------------------------------------------------------------------------------
def _case(seed, n):
    rng = np.random.default_rng(seed)
    q = gqm.GridQ(rng.uniform(-1, 1, 3), rng.uniform(0.05, 0.3, 3), n)
    d = rng.uniform(-1, 1, n).astype(F)
    lo, hi = q.start - q.cs, q.end + q.cs
    pts = (lo + rng.random((600, 3)) * (hi - lo)).astype(F)
    pts = np.concatenate([pts, [[np.nan, 0, 0], [np.inf, 0, 0], q.start, q.end]]).astype(F)
    rays_o = (lo + rng.random((60, 3)) * (hi - lo)).astype(F)
    rays_d = rng.normal(size=(60, 3)).astype(F)
    rays_d /= np.linalg.norm(rays_d, axis=1, keepdims=True)
    return rng, q, d, pts, rays_o, rays_d.astype(F)


@pytest.mark.parametrize("n", [(5, 7, 67), (9, 1, 9), (1, 6, 6), (2, 2, 2)], ids=lambda n: "x".join(map(str, n)))
def test_all_cells_active_is_the_dense_field(n):
    _, q, d, pts, ro, rd = _case(21, n)
    band = bqm.Band(n, np.arange(d.size, dtype=np.uint64), d.reshape(-1), 0.75, 0.5)
    flat = d.reshape(-1)
    inside = gqm._state(q, pts) == 0
    for mode in MODES:
        for iso in (0.0, 0.25):
            v, s = bqm.sample(q, band, pts, mode, iso)
            assert gqm.same_bits(v, gqm.sample(q, flat, pts, mode, iso))
            assert np.array_equal(s, np.where(inside, bqm.K_OF[mode], 0))
            assert gqm.same_bits(bqm.normal(q, band, pts, mode, iso), gqm.normal(q, flat, pts, mode, iso))
            got = bqm.raymarch(q, band, ro, rd, mode, iso, max_steps=20, normals=True)
            want = gqm.raymarch(q, flat, ro, rd, mode, iso, max_steps=20, normals=True)
            assert gqm.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
            assert gqm.same_bits(got[4], want[3])


def test_a_partly_active_band_is_the_dense_d_prime_and_support_counts_the_active_reads():
    n = (6, 5, 70)
    rng, q, d, pts, ro, rd = _case(22, n)
    active = rng.random(n) < 0.5
    cells, vals = np.flatnonzero(active.reshape(-1)).astype(np.uint64), d.reshape(-1)[active.reshape(-1)]
    for with_bits in (False, True):
        bits = rng.integers(0, 2 ** 32, (n[0], n[1], (n[2] + 31) // 32), dtype=np.uint64).astype(np.uint32) if with_bits else None
        band = bqm.Band(n, cells, vals, 0.75, 0.5, bits)
        dp = band.dense()
        # D' by the definition, cell by cell
        i, j, k = np.meshgrid(*(np.arange(c) for c in n), indexing="ij")
        ins = ((bits[i, j, k >> 5] >> (k & 31).astype(np.uint32)) & 1).astype(bool) if with_bits else np.zeros(n, bool)
        want = np.where(active, d, np.where(ins, F(-0.5), F(0.75))).astype(F)
        assert np.array_equal(dp.view(np.uint32), want.view(np.uint32))
        assert not with_bits or ((dp == F(-0.5)).any() and (dp == F(0.75)).any())
        flat = dp.reshape(-1)
        mixed = 0
        for mode in MODES:
            v, s = bqm.sample(q, band, pts, mode, 0.25)
            assert gqm.same_bits(v, gqm.sample(q, flat, pts, mode, 0.25))
            assert s.max() <= bqm.K_OF[mode] and (s[gqm._state(q, pts) != 0] == 0).all()
            mixed += int(((s > 0) & (s < bqm.K_OF[mode])).sum())
            got = bqm.raymarch(q, band, ro, rd, mode, 0.25, max_steps=20, normals=True)
            want_r = gqm.raymarch(q, flat, ro, rd, mode, 0.25, max_steps=20, normals=True)
            assert gqm.same_bits(got[0], want_r[0]) and np.array_equal(got[1], want_r[1]) and gqm.same_bits(got[4], want_r[3])
            never = np.isnan(ro).any(1) | ((got[1] == 0) & (got[0][:, 3] == 1))
            assert (got[3][never] == 0).all()
        assert mixed > 0
    # support of a snapped sample is whether its cell is active: cell by cell at the centres (first_cell is the centre of cell 0)
    idx = np.stack(np.meshgrid(*(np.arange(c) for c in n), indexing="ij"), -1).reshape(-1, 3)
    centres = (q.start + idx.astype(F) * q.cs).astype(F)
    _, s = bqm.sample(q, band, centres, gqm.SNAP)
    assert np.array_equal(s.astype(bool), active.reshape(-1))


def test_the_model_takes_cells_as_they_are():
    """Order and range are m2s_band_create's checks, not the model's: int64 or uint64, any shape, an empty list, a single cell."""
    n = (3, 4, 5)
    q = gqm.GridQ([0, 0, 0], [0.25] * 3, n)
    pts = np.array([[0.3, 0.4, 0.5], [0.01, 0.01, 0.01]], F)
    a = bqm.Band(n, np.array([7, 30], np.uint64), np.array([0.125, -0.25], F), 0.75, 0.5)
    b = bqm.Band(n, np.array([[7], [30]], np.int64), [0.125, -0.25], 0.75, 0.5)
    for mode in MODES:
        va, sa = bqm.sample(q, a, pts, mode)
        vb, sb = bqm.sample(q, b, pts, mode)
        assert gqm.same_bits(va, vb) and np.array_equal(sa, sb)
    empty = bqm.Band(n, np.zeros(0, np.uint64), np.zeros(0, F), 0.75, 0.5)
    for mode in MODES:                                     # the interpolated background: the weights need not sum to one exactly
        v, s = bqm.sample(q, empty, pts, mode)
        assert gqm.same_bits(v, gqm.sample(q, np.full(60, 0.75, F), pts, mode)) and (s == 0).all()
    assert (bqm.sample(q, empty, pts, gqm.SNAP)[0] == F(0.75)).all()
    assert (empty.dense() == F(0.75)).all()
