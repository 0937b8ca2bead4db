"""m2s_band_isosurface without a GPU: the export and the header, every argument check that is decided before device work (host-memory lists
that do not ascend or run past the grid included), the consumers, the isosurface_band helper, and the model tests/band_isosurface_model.py
against isosurface_model.extract: all points active, independence from the filler, and the corollary on the oracle's dense grids — a band
of 1.001 cell diagonals around iso gives the dense mesh, half a diagonal does not and says so through n_open."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import band_isosurface_model as bim
import isosurface_model as im
import oracle as orc
from mesh_to_sdf_amd import Grid, M2SPanic, NarrowBand, _lib, band_isosurface, isosurface_band, meshes, remesh  # noqa: F401

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


# ---- 1. exports, header ------------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_exported(lib):
    assert "m2s_band_isosurface" in _lib.EXPORTS and hasattr(lib, "m2s_band_isosurface")
    hdr = open(os.path.join(ROOT, "include", "m2s.h")).read()
    assert "int m2s_band_isosurface(const m2s_grid* grid, const uint64_t* cells, const float* distances, uint64_t n_cells, float iso," in hdr
    assert "#define M2S_VERSION_MINOR 5" in hdr
    assert lib.m2s_version() == 5
    assert hasattr(NarrowBand, "isosurface")
    hpp = open(os.path.join(ROOT, "include", "mesh_to_sdf.hpp")).read()
    assert "BandIsosurface<V> band_isosurface(" in hpp


# ---- 2. argument checks that need no device ---------------------------------------------------------------------------------------------------
def _opts(**kw):
    o = _lib.M2SOpts()
    o.struct_size = C.sizeof(_lib.M2SOpts)
    o.device = -1
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_bad_arguments_fail_before_the_device(lib):
    g = Grid.from_bounding_box([0, 0, 0], [1, 1, 1], [4, 4, 4])
    G = C.byref(g._g)
    cells, d = np.arange(64, dtype=np.uint64), np.zeros(64, F)
    P, D = cells.ctypes.data, d.ctypes.data
    v, t = np.full((8, 3), -7.0, F), np.full((8, 3), 0xABCDEF01, np.uint32)
    V, T = v.ctypes.data, t.ctypes.data
    cnt = (C.c_uint64 * 3)(77, 77, 77)
    BAD = _lib.ERR_BAD_ARG
    iso = lib.m2s_band_isosurface
    assert iso(None, P, D, 64, 0.0, None, 0, None, 0, cnt, None) == BAD                 # NULL grid
    assert iso(G, P, D, 64, 0.0, None, 0, None, 0, None, None) == BAD                   # NULL counts
    assert iso(G, None, D, 64, 0.0, None, 0, None, 0, cnt, None) == BAD                 # NULL cells, n_cells > 0
    assert iso(G, P, None, 64, 0.0, None, 0, None, 0, cnt, None) == BAD                 # NULL distances, n_cells > 0
    assert iso(G, P, D, 65, 0.0, None, 0, None, 0, cnt, None) == BAD                    # n_cells above the cell count
    assert "n_cells" in _lib.last_error()
    assert iso(G, P, D, 64, 0.0, V, 8, None, 8, cnt, None) == BAD                       # exactly one output NULL
    assert iso(G, P, D, 64, 0.0, None, 8, T, 8, cnt, None) == BAD
    for bad_iso in (float("nan"), INF, -INF):
        assert iso(G, P, D, 64, bad_iso, None, 0, None, 0, cnt, None) == BAD
    for first, size, count in [([0] * 3, [0.25] * 3, [4, 0, 4]), ([0] * 3, [0.25, 0.0, 0.25], [4] * 3),
                               ([0] * 3, [0.25, -0.25, 0.25], [4] * 3), ([0] * 3, [0.25, np.inf, 0.25], [4] * 3),
                               ([0] * 3, [0.25, 0.25, np.nan], [4] * 3), ([0, np.nan, 0], [0.25] * 3, [4] * 3),
                               ([np.inf, 0, 0], [0.25] * 3, [4] * 3),
                               ([0] * 3, [0.25] * 3, [2 ** 12, 2 ** 12, 2 ** 12]),       # 2^36 cells: the band's own limit
                               ([0] * 3, [0.25] * 3, [2 ** 40, 2 ** 30, 2 ** 10])]:      # a product that overflows 64 bits
        bad = Grid(first, size, count)
        assert iso(C.byref(bad._g), P, D, 1, 0.0, None, 0, None, 0, cnt, None) == BAD, (first, size, count)
    for field, value in [("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4), ("mem_kind", 5)]:
        assert iso(G, P, D, 64, 0.0, None, 0, None, 0, cnt, C.byref(_opts(**{field: value}))) == BAD, field
    o = _opts()
    peers = (C.c_void_p * 1)()
    o.n_peer_out, o.peer_out = 1, C.cast(peers, type(o.peer_out))
    assert iso(G, P, D, 64, 0.0, None, 0, None, 0, cnt, C.byref(o)) == BAD
    # host memory: the list is judged on the host
    for bad_cells in ([5, 4, 9], [4, 5, 5], [4, 5, 64], [0, 2 ** 63], [1, 0]):
        c = np.array(bad_cells, np.uint64)
        for o in (None, C.byref(_opts(mem_kind=_lib.MEM_HOST))):
            assert iso(G, c.ctypes.data, D, c.size, 0.0, V, 8, T, 8, cnt, o) == BAD, bad_cells
            assert "cells[" in _lib.last_error()
    assert list(cnt) == [77, 77, 77]                                                      # no failed check writes counts
    assert (v == F(-7.0)).all() and (t == 0xABCDEF01).all()
    assert iso(G, None, None, 0, 0.0, None, 0, None, 0, cnt, None) == _lib.M2S_OK and list(cnt) == [0, 0, 0]   # an empty band needs no device
    with pytest.raises(M2SPanic):
        band_isosurface(g, cells, d[:63])                                                 # cells and distances differ in length
    with pytest.raises(M2SPanic):
        band_isosurface(g, np.array([3, 2], np.int64), d[:2])
    with pytest.raises(M2SPanic):
        band_isosurface(g, np.array([-1, 2], np.int64), d[:2])                            # a negative int64 is out of range
    with pytest.raises(M2SPanic):
        NarrowBand(np.array([7, 7], np.uint64), d[:2], None, 2, g).isosurface()
    ve, te, n_open = band_isosurface(g, np.zeros(0, np.uint64), np.zeros(0, F))
    assert ve.shape == (0, 3) and te.shape == (0, 3) and te.dtype == np.uint32 and n_open == 0


# ---- 3. the consumers compile -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cc,std,src", [("gcc", "-std=c99", "tests/c/band_isosurface_smoke.c"), ("g++", "-std=c++17", "tests/cpp/band_isosurface_tests.cpp")])
def test_consumers_compile_and_check_their_arguments(lib, tmp_path, cc, std, src):
    exe = str(tmp_path / os.path.basename(src).split(".")[0])
    subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                           os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


# ---- 4. the helper --------------------------------------------------------------------------------------------------------------------------------
def _up(x):
    y = F(x)
    return float(y if float(y) >= x else np.nextafter(y, F(np.inf)))


def test_isosurface_band_is_the_stated_pair():
    for size in ([0.25, 0.25, 0.25], [0.1, 0.3, 0.07], [1e-3, 2.0, 0.5]):
        grid = Grid([0, 0, 0], size, [4, 5, 6])
        sx, sy, sz = (float(s) for s in grid.get_cell_size())
        w = _up(1.001 * float(np.sqrt(sx * sx + sy * sy + sz * sz)))
        assert float(F(w)) == w >= 1.001 * np.sqrt(sx * sx + sy * sy + sz * sz)
        for iso in (0.0, 0.07, -0.05, 10.0, -10.0):
            interior, exterior = isosurface_band(grid, iso)
            i32 = float(F(iso))
            assert (interior, exterior) == (_up(max(0.0, w - i32)), _up(max(0.0, i32 + w))), (size, iso)
            assert interior >= 0 and exterior >= 0 and float(F(interior)) == interior and float(F(exterior)) == exterior
            if abs(iso) < w:                                      # the band contains [iso - w, iso + w]
                assert -interior <= i32 - w and i32 + w <= exterior
    assert isosurface_band(Grid([0, 0, 0], [0.25] * 3, [4, 4, 4])) == isosurface_band(Grid([0, 0, 0], [0.25] * 3, [4, 4, 4]), 0.0)


# ---- 5. the model -----------------------------------------------------------------------------------------------------------------------------------
def _random_case(seed, n):
    rng = np.random.default_rng(seed)
    g = im.GridI(rng.uniform(-1, 1, 3), rng.uniform(0.05, 0.3, 3), n)
    d = rng.uniform(-1, 1, n).astype(F)
    return rng, g, d


@pytest.mark.parametrize("n", [(5, 7, 9), (9, 1, 9), (1, 6, 6), (2, 2, 2)])
def test_all_points_active_is_the_dense_extraction(n):
    _, g, d = _random_case(11, n)
    for iso in (0.0, 0.25):
        wv, wt = im.extract(g, d, iso)
        v, t, n_open = bim.extract(g, np.arange(d.size, dtype=np.uint64), d.reshape(-1), iso)
        assert n_open == 0 and np.array_equal(v.view(np.uint32), wv.view(np.uint32)) and np.array_equal(t, wt)
        assert len(wv) > 0


def test_the_result_does_not_depend_on_the_filler():
    rng, g, d = _random_case(12, (6, 7, 8))
    total = 0
    for frac in (0.9, 0.5, 0.1):
        active = rng.random(d.size) < frac
        cells, vals = np.flatnonzero(active).astype(np.uint64), d.reshape(-1)[active]
        for iso in (0.0, 0.25):
            a = bim.extract(g, cells, vals, iso, fill=0.0)
            for fill in (1.0e30, -3.5):
                b = bim.extract(g, cells, vals, iso, fill=fill)
                assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]) and a[2] == b[2], (frac, iso, fill)
            total += len(a[0])
            if frac == 0.5:
                assert a[2] > 0 and 0 < len(a[0]) < len(im.extract(g, d, iso)[0])
    assert total > 0


def test_the_box_form_is_the_whole_on_a_small_grid():
    rng, g, d = _random_case(13, (9, 8, 10))
    box = ((2, 7), (1, 8), (3, 10))                     # reaches the grid's end on y and z, is cut on x
    act = np.zeros(g.n, bool)
    act[2:6, 1:8, 3:10] = rng.random((4, 7, 7)) < 0.8   # x layer 6 of the box stays empty: no owned cell is cut off
    cells, vals = np.flatnonzero(act.reshape(-1)).astype(np.uint64), d[act]
    a, b = bim.extract(g, cells, vals, 0.1), bim.extract_box(g, box, cells, vals, 0.1)
    assert len(a[0]) > 0 and len(a[1]) > 0 and a[2] > 0
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.fixture(scope="module")
def oracle_grids():
    """name -> (GridI, the oracle's dense Raycast grid): the reference's own arithmetic on the CPU."""
    out = {}
    for name, (v, idx), count in (("cube", meshes.cube(), (12, 9, 10)), ("blob", meshes.blob(slices=24, stacks=17), (24, 20, 17))):
        lo, hi = meshes.extended_bbox(v, 0.25)
        first, size, count = meshes.grid_from_bounding_box(lo, hi, count)
        first, size, count = np.asarray(first, F), np.asarray(size, F), tuple(int(c) for c in count)
        d = orc.generate_grid_sdf(np.asarray(v, F), np.asarray(idx, np.uint32), first, size, count, sign=0, semantics=orc.EXACT)
        out[name] = (im.GridI(first, size, count), np.asarray(d, F).reshape(count))
    return out


@pytest.mark.parametrize("iso", [0.0, 0.07, -0.05])
@pytest.mark.parametrize("name", ["cube", "blob"])
def test_the_corollary_on_the_oracles_grids(oracle_grids, name, iso):
    g, d = oracle_grids[name]
    diag = float(np.sqrt((g.cs.astype(np.float64) ** 2).sum()))
    wv, wt = im.extract(g, d, iso)
    assert len(wt) > 0
    # 1.001 diagonals either side of iso: covered, and the dense mesh bit for bit
    w = 1.001 * diag
    cells, vals = bim.band_of(d, max(0.0, w - iso), max(0.0, iso + w))
    active = np.zeros(d.size, bool)
    active[cells.astype(np.int64)] = True
    assert 0 < cells.size < d.size
    assert bim.covered(g, d, active, iso)
    v, t, n_open = bim.extract(g, cells, vals, iso)
    assert n_open == 0 and np.array_equal(v.view(np.uint32), wv.view(np.uint32)) and np.array_equal(t, wt)
    # half a diagonal: not covered, a different mesh, and n_open says so
    w = 0.5 * diag
    cells, vals = bim.band_of(d, max(0.0, w - iso), max(0.0, iso + w))
    active[:] = False
    active[cells.astype(np.int64)] = True
    assert not bim.covered(g, d, active, iso)
    v, t, n_open = bim.extract(g, cells, vals, iso)
    assert n_open > 0 and len(t) < len(wt) and len(v) <= len(wv)
    if name == "blob" and iso == 0.0:
        assert (len(v), len(wv), len(t), len(wt)) == (822, 872, 509, 1740)
