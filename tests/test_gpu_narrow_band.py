"""m2s_narrow_band_sdf / m2s_mesh_narrow_band_sdf on the GPU.  The yardstick in every test is the dense generate_grid_sdf of the same mesh,
grid and sign method, filtered in numpy: cells exactly, distances as uint32 views, bits against the packed filter, and the count — host
and device memory, one-shot and Mesh, the default path and algorithm 1, one chunk and several."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import band_model as bm
import sample_model as sm
import voxel_model as vm
from mesh_to_sdf_amd import Grid, M2SPanic, M2STimings, Mesh, NarrowBand, SignMethod, Topology, _lib, generate_grid_sdf, meshes, narrow_band_sdf

F = np.float32
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
SIGNS = [SignMethod.Raycast, SignMethod.Normal]
# (interior, exterior) in cells of the grid's smallest cell size
WIDTHS = [(0.0, 0.0), (1.5, 1.5), (3.0, 0.75), (INF, INF)]


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _dev(v, idx):
    return torch.as_tensor(v, device=DEV), (None if idx is None else torch.as_tensor(idx.astype(np.int64), device=DEV))


def _grid_of(v, count, frac=0.1):
    lo, hi = meshes.extended_bbox(v, frac)
    return Grid.from_bounding_box(lo, hi, list(count))


def _shape(grid):
    return tuple(int(c) for c in grid.get_cell_count())


def _band(grid, cells):
    h = float(min(grid.get_cell_size()))
    return tuple(F(c) * F(h) if np.isfinite(c) else INF for c in cells)


def _dense(v, idx, grid, sign):
    """The dense result, flat float32 on the host.  None when the dense call itself fails with a NaN distance, as the reference panics
    (Normal: a NaN vertex, coordinates near 3e38 whose products overflow)."""
    try:
        return _np(generate_grid_sdf(v, Topology.TriangleList(idx), grid, sign)).reshape(-1).astype(F)
    except M2SPanic as e:
        assert e.code == _lib.ERR_NAN and sign == SignMethod.Normal, e
        return None


def _check(got: NarrowBand, D, band, grid, what):
    """cells, distances, bits and count of `got` against the filter of the dense result D."""
    assert isinstance(got, NarrowBand)
    interior, exterior = band
    with np.errstate(invalid="ignore"):
        active = (F(-interior) <= D) & (D <= F(exterior))
    want_cells = np.flatnonzero(active).astype(np.uint64)
    cells, dist = _np(got.cells).astype(np.uint64), _np(got.distances)
    assert got.count == want_cells.size == cells.size == dist.size, f"{what}: count {got.count}, want {want_cells.size}"
    assert np.array_equal(cells, want_cells), f"{what}: cells"
    assert dist.dtype == F and np.array_equal(dist.view(np.uint32), D[active].view(np.uint32)), f"{what}: distances"
    if got.bits is not None:
        assert np.array_equal(_np(got.bits).view(np.uint32), vm.pack_bits(active.reshape(_shape(grid)).astype(np.uint8))), f"{what}: bits"
    return want_cells.size


@pytest.fixture(scope="module")
def cases(suzanne):
    """name -> (vertices, indices, Grid): the cases of test_gpu_voxelize.py plus an open mesh."""
    b12 = meshes.blob(12, 9)
    far = np.array([1.0e4, -1.0e4, 1.0e4], F)
    b12_far = ((b12[0] + far).astype(F), b12[1])
    deg, huge = sm.with_degenerates(*b12), sm.one_huge(*b12)
    nan = (b12[0].copy(), b12[1])
    nan[0][7, 1] = np.nan
    one = np.array([0, 1, 2], np.uint32)
    g12 = _grid_of(b12[0], (40, 24, 33))
    open_idx = np.ascontiguousarray(b12[1].reshape(-1, 3)[5:-3].reshape(-1))      # a cap of triangles removed at both poles
    all_ = {"cube": (*meshes.cube(), _grid_of(meshes.cube()[0], (16, 16, 16))),
            "suzanne": (*suzanne, _grid_of(suzanne[0], (33, 20, 31))),
            "blob-192": (*b12, _grid_of(b12[0], (32, 32, 65))),
            "blob-192-far": (*b12_far, _grid_of(b12_far[0], (32, 32, 32))),
            "degenerates": (*deg, g12),
            "one-huge": (*huge, _grid_of(huge[0], (40, 24, 33))),
            "larger-than-the-grid": (np.array([[-50, -60, -9], [80, -10, 7], [-20, 90, 6]], F), one, g12),
            "wholly-outside": (np.array([[5, 5, 5], [6, 5, 5], [5, 6, 7]], F), one, g12),
            "nan-vertex": (*nan, g12),
            "one-cell": (*b12, _grid_of(b12[0], (1, 1, 1))),
            "empty": (np.zeros((0, 3), F), np.zeros(0, np.uint32), g12),
            "open": (b12[0], open_idx, _grid_of(b12[0], (32, 32, 65)))}
    return {k: (np.ascontiguousarray(v, F), np.ascontiguousarray(i, np.uint32), g) for k, (v, i, g) in all_.items()}


@pytest.fixture(scope="module")
def dense(cases):
    """(name, sign) -> the dense result, computed once and left unchanged."""
    return {(name, sign): _dense(v, idx, grid, sign) for name, (v, idx, grid) in cases.items() for sign in SIGNS}


@pytest.fixture(scope="module")
def blob100k():
    v, idx = meshes.named("blob-100k")
    assert idx.size // 3 > 2 * 4096 and (idx.size // 3) % 4096 != 0           # several scan tiles, the last one short
    return _dev(v, idx) + (v,)


MESHES = ["cube", "suzanne", "blob-192", "blob-192-far", "degenerates", "one-huge", "larger-than-the-grid", "wholly-outside", "nan-vertex",
          "one-cell", "empty", "open"]


# ---- 1. every path is the dense filter, in every output -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("sign", SIGNS, ids=["raycast", "normal"])
@pytest.mark.parametrize("name", MESHES)
def test_every_path_matches_the_dense_filter(cases, dense, name, sign, device):
    v, idx, grid = cases[name]
    D = dense[(name, sign)]
    a, b = _dev(v, idx) if device else (v, idx)
    topo = Topology.TriangleList(b)
    if D is None:
        # the dense call fails with M2S_ERR_NAN (the reference panics): there is nothing to filter.  With both widths infinite every cell
        # is walked, so the call meets the same NaN; narrower bands may or may not walk a cell that does.
        assert name in ("nan-vertex", "one-huge", "degenerates") and sign == SignMethod.Normal
        for algorithm in (0, 1):
            with pytest.raises(M2SPanic) as e:
                narrow_band_sdf(a, topo, grid, (INF, INF), sign, algorithm=algorithm)
            assert e.value.code == _lib.ERR_NAN
        return
    total = 0
    for cells in WIDTHS:
        band = _band(grid, cells)
        total += _check(narrow_band_sdf(a, topo, grid, band, sign, bits=True), D, band, grid, f"{name} {cells}: one shot")
        _check(narrow_band_sdf(a, topo, grid, band, sign, bits=True, algorithm=1), D, band, grid, f"{name} {cells}: one shot, algorithm 1")
    with Mesh(a, topo) as m:
        for cells in WIDTHS:
            band = _band(grid, cells)
            _check(m.narrow_band_sdf(grid, band, sign, bits=True), D, band, grid, f"{name} {cells}: Mesh")
            _check(m.narrow_band_sdf(grid, band, sign, algorithm=1), D, band, grid, f"{name} {cells}: Mesh, algorithm 1")
    full = narrow_band_sdf(a, topo, grid, INF, sign)
    assert full.count == D.size and np.array_equal(_np(full.distances).view(np.uint32), D.view(np.uint32)), "both widths infinite: the dense grid"
    assert np.array_equal(_np(full.to_dense()).reshape(-1).view(np.uint32), D.view(np.uint32))
    if name not in ("wholly-outside", "empty", "one-cell"):
        assert D.size < total < 4 * D.size, (name, total)                      # the finite bands are neither empty nor everything


def test_a_single_width_is_both_widths_and_ijk(cases, dense):
    v, idx, grid = cases["suzanne"]
    D = dense[("suzanne", SignMethod.Raycast)]
    band = _band(grid, (2.0, 2.0))
    got = narrow_band_sdf(*_dev(v, idx)[:1], Topology.TriangleList(_dev(v, idx)[1]), grid, band[0])
    _check(got, D, band, grid, "one width")
    ijk = _np(got.ijk())
    ny, nz = _shape(grid)[1:]
    assert np.array_equal(ijk[:, 2] + ijk[:, 1] * nz + ijk[:, 0] * ny * nz, _np(got.cells))
    dd = _np(got.to_dense()).reshape(-1)
    assert np.isnan(dd).sum() == D.size - got.count and np.array_equal(dd[_np(got.cells)].view(np.uint32), _np(got.distances).view(np.uint32))


# ---- 2. chunks -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", SIGNS, ids=["raycast", "normal"])
def test_a_forced_small_chunk_gives_the_same_outputs(cases, dense, sign):
    v, idx, grid = cases["suzanne"]
    D = dense[("suzanne", sign)]
    dv, di = _dev(v, idx)
    topo = Topology.TriangleList(di)
    band = _band(grid, (1.5, 1.5))
    t = M2STimings()
    _check(narrow_band_sdf(dv, topo, grid, band, sign, bits=True, timings=t), D, band, grid, "one chunk")
    n = int(t.n_units)
    first, size = np.array(grid.get_first_cell(), F), np.array(grid.get_cell_size(), F)
    tris = v[idx.reshape(-1, 3)].reshape(-1, 9)
    assert n == int(bm.candidates(tris, first, size, _shape(grid), max(band)).sum()), "n_units is the number of candidates of the model"
    chunk = 3 * n // 7
    assert (n + chunk - 1) // chunk == 3 and 0 < n % chunk < chunk            # three chunks, the last one short
    with _lib.knobs(M2S_BAND_CHUNK=chunk):
        _check(narrow_band_sdf(dv, topo, grid, band, sign, bits=True), D, band, grid, "three chunks")
        _check(narrow_band_sdf(v, Topology.TriangleList(idx), grid, band, sign, bits=True), D, band, grid, "three chunks, host")
        with Mesh(dv, topo) as m:
            _check(m.narrow_band_sdf(grid, band, sign, bits=True), D, band, grid, "three chunks, Mesh")
    with _lib.knobs(M2S_BAND_CHUNK=97):
        _check(narrow_band_sdf(dv, topo, grid, band, sign, bits=True), D, band, grid, "chunks of 97")


# ---- 3. capacity -------------------------------------------------------------------------------------------------------------------------------
def test_capacity_one_short(cases, dense):
    v, idx, grid = cases["suzanne"]
    D = dense[("suzanne", SignMethod.Raycast)]
    band = _band(grid, (1.5, 1.5))
    active = (F(-band[0]) <= D) & (D <= F(band[1]))
    n = int(active.sum())
    L = _lib.lib()
    bo = _lib.M2SBandOpts(C.sizeof(_lib.M2SBandOpts), band[1], band[0])
    bits = np.full(33 * 20, 0xFFFFFFFF, np.uint32)
    cells, dist = np.full(n, 12345, np.uint64), np.full(n, -7.0, F)
    count = C.c_uint64(0)
    args = (v.ctypes.data, v.shape[0], idx.ctypes.data, idx.size, 4, 0, C.byref(grid._g), 0, C.byref(bo))
    for algorithm in (0, 1):
        o = _lib.M2SOpts()
        o.struct_size, o.device, o.mem_kind, o.synchronous, o.algorithm = C.sizeof(_lib.M2SOpts), -1, _lib.MEM_HOST, 1, algorithm
        bits[:], count.value = 0xFFFFFFFF, 0
        assert L.m2s_narrow_band_sdf(*args, cells.ctypes.data, dist.ctypes.data, n - 1, bits.ctypes.data, C.byref(count), C.byref(o)) == _lib.ERR_BAD_ARG
        assert "capacity" in _lib.last_error()
        assert count.value == n and (cells == 12345).all() and (dist == F(-7.0)).all()
        assert np.array_equal(bits.reshape(33, 20, 1), vm.pack_bits(active.reshape(33, 20, 31).astype(np.uint8)))
    assert L.m2s_narrow_band_sdf(*args, cells.ctypes.data, None, n, None, C.byref(count), None) == _lib.M2S_OK
    assert np.array_equal(cells, np.flatnonzero(active).astype(np.uint64)) and (dist == F(-7.0)).all()
    assert L.m2s_narrow_band_sdf(*args, None, dist.ctypes.data, n, None, None, None) == _lib.M2S_OK
    assert np.array_equal(dist.view(np.uint32), D[active].view(np.uint32))
    dv, di = _dev(v, idx)
    d_cells = torch.full((n,), 12345, dtype=torch.int64, device=DEV)
    d_dist = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    o = _lib.M2SOpts()
    o.struct_size, o.device, o.mem_kind, o.synchronous = C.sizeof(_lib.M2SOpts), 0, _lib.MEM_DEVICE, 0
    count.value = 0
    rc = L.m2s_narrow_band_sdf(dv.data_ptr(), v.shape[0], di.to(torch.int32).data_ptr(), idx.size, 4, 0, C.byref(grid._g), 0, C.byref(bo),
                               d_cells.data_ptr(), d_dist.data_ptr(), n - 1, None, C.byref(count), C.byref(o))
    torch.cuda.synchronize()
    assert rc == _lib.ERR_BAD_ARG and count.value == n and bool((d_cells == 12345).all()) and bool((d_dist == -7.0).all())
    with pytest.raises(M2SPanic):
        narrow_band_sdf(dv, Topology.TriangleList(di), grid, band, capacity=n - 1)
    _check(narrow_band_sdf(dv, Topology.TriangleList(di), grid, band, capacity=n + 100, bits=True), D, band, grid, "a roomy capacity: one call")


# ---- 4. larger meshes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", SIGNS, ids=["raycast", "normal"])
def test_blob_100k_against_the_dense_filter(blob100k, sign):
    dv, di, v = blob100k
    grid = _grid_of(v, (64, 48, 80))
    topo = Topology.TriangleList(di)
    D = _np(generate_grid_sdf(dv, topo, grid, sign)).reshape(-1)
    band = _band(grid, (2.0, 2.0))
    t = M2STimings()
    n = _check(narrow_band_sdf(dv, topo, grid, band, sign, bits=True, timings=t), D, band, grid, "blob-100k")
    assert 1000 < n <= t.n_units < D.size // 2, (n, t.n_units, D.size)         # a band, and candidates that are not the whole grid
    with Mesh(dv, topo) as m:
        _check(m.narrow_band_sdf(grid, band, sign), D, band, grid, "blob-100k, Mesh")


def test_more_scan_tiles_than_threads():
    """1040 x 1010 x 8 cells are 1 050 400 mask words, 257 scan tiles: every thread of the one workgroup that scans the candidates' tile
    sums walks two of them, and the emit kernel reads the offsets of all 257.  Algorithm 1 takes its mask from the dense grid."""
    v, idx = meshes.blob(12, 9)
    dv, di = _dev(v, idx)
    shape = (1040, 1010, 8)
    grid = _grid_of(v, shape)
    topo = Topology.TriangleList(di)
    band = _band(grid, (1.0, 1.0))
    fast = narrow_band_sdf(dv, topo, grid, band, SignMethod.Raycast)
    slow = narrow_band_sdf(dv, topo, grid, band, SignMethod.Raycast, algorithm=1)
    cells = _np(fast.cells).astype(np.uint64)
    n_tiles, held = vm.scan_tiles(cells, shape)
    assert n_tiles > 256, n_tiles
    even = held[held % 2 == 0]
    assert np.isin(even + 1, held).any(), "no thread of the scan holds two tiles with candidates"
    assert fast.count == slow.count == cells.size > 0
    assert np.array_equal(cells, _np(slow.cells).astype(np.uint64))
    assert np.array_equal(_np(fast.distances).view(np.uint32), _np(slow.distances).view(np.uint32))


def test_suzanne_96_leaves_the_all_pairs_branch(cases):
    """96^3 cells: a chunk of candidates times suzanne's triangles is past the all-pairs limit of the query path (M2S_BRUTE_MAX: 1.2e8 pairs
    without rays), so the tree is walked; with the limit forced to 0 and with the lane walk forced the outputs are the same."""
    v, idx, _ = cases["suzanne"]
    dv, di = _dev(v, idx)
    topo = Topology.TriangleList(di)
    grid = _grid_of(v, (96, 96, 96))
    for sign in SIGNS:
        D = _np(generate_grid_sdf(dv, topo, grid, sign)).reshape(-1)
        band = _band(grid, (5.0, 5.0))
        t = M2STimings()
        _check(narrow_band_sdf(dv, topo, grid, band, sign, bits=True, timings=t), D, band, grid, "suzanne 96^3")
        assert float(t.n_units) * (idx.size // 3) > 1.2e8, (t.n_units, idx.size // 3)
        with _lib.knobs(M2S_BRUTE_MAX=0):
            _check(narrow_band_sdf(dv, topo, grid, band, sign), D, band, grid, "suzanne 96^3, no all-pairs path")
        with _lib.knobs(M2S_LANE_WALK=1):
            _check(narrow_band_sdf(dv, topo, grid, band, sign), D, band, grid, "suzanne 96^3, lane walk")
        with _lib.knobs(M2S_LANE_WALK=0, M2S_BRUTE_MAX=0, M2S_BAND_CHUNK=50000):
            _check(narrow_band_sdf(dv, topo, grid, band, sign), D, band, grid, "suzanne 96^3, packets, chunks of 50000")


# ---- 5. persistent meshes ---------------------------------------------------------------------------------------------------------------------------
def test_mesh_before_and_after_a_grid_call_and_asynchronous_calls(cases, dense):
    v, idx, grid = cases["suzanne"]
    dv, di = _dev(v, idx)
    band = _band(grid, (1.5, 1.5))
    with Mesh(dv, Topology.TriangleList(di)) as m:
        for sign in SIGNS:
            D = dense[("suzanne", sign)]
            _check(m.narrow_band_sdf(grid, band, sign, bits=True), D, band, grid, "before")
            m.generate_grid_sdf(_grid_of(v, (24, 24, 24)), sign)                   # re-marks the tree's leaves
            _check(m.narrow_band_sdf(grid, band, sign, bits=True), D, band, grid, "after a grid call")
        D = dense[("suzanne", SignMethod.Raycast)]
        t = M2STimings()
        n = _check(m.narrow_band_sdf(grid, band, timings=t), D, band, grid, "timed")
        cand = int(t.n_units)
        assert n <= cand < D.size and t.n_triangles == idx.size // 3 and t.distance_ms > 0 and t.seed_ms > 0 and t.total_ms >= t.distance_ms
        m.drain_timings()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            a = m.narrow_band_sdf(grid, band, bits=True, capacity=n, synchronous=False)
        with torch.cuda.stream(s2):
            b = m.narrow_band_sdf(grid, band, SignMethod.Normal, capacity=cand, synchronous=False)
        d = m.drain_timings()
        torch.cuda.synchronize()
        assert d.n_units == 2 * cand and d.distance_launches == 2 and d.distance_ms > 0
        _check(a, D, band, grid, "asynchronous, stream 1")
        _check(b, dense[("suzanne", SignMethod.Normal)], band, grid, "asynchronous, stream 2")
    t = M2STimings()
    _check(narrow_band_sdf(dv, Topology.TriangleList(di), grid, band, timings=t), D, band, grid, "one shot, timed")
    assert t.n_units == cand and t.accel_build_ms > 0 and t.seed_ms > 0 and t.distance_ms > 0


# ---- 6. consumers ---------------------------------------------------------------------------------------------------------------------------------
def _build(tmp_path, cc, std, src, extra=()):
    exe = str(tmp_path / os.path.basename(src).split(".")[0])
    subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                           os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", *extra, "-o", exe])
    return exe


def test_c_and_cpp_consumers_run_clean(tmp_path):
    exe = _build(tmp_path, "gcc", "-std=c99", "tests/c/narrow_band_smoke.c", ["-lm"])
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    exe = _build(tmp_path, "g++", "-std=c++17", "tests/cpp/narrow_band_tests.cpp")
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
