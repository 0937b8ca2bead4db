"""m2s_voxelize / m2s_mesh_voxelize on the GPU: every output against the numpy model of the contract (tests/voxel_model.py) bit for bit —
host and device memory, one-shot and Mesh —, the default path against algorithm 1, the outputs against each other, SOLID against the
Raycast sign of generate_grid_sdf, the set against the distance field, and the persistent-mesh paths."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import sample_model as sm
import voxel_model as vm
from mesh_to_sdf_amd import Grid, M2STimings, Mesh, SignMethod, Topology, Voxels, _lib, generate_grid_sdf, meshes, voxelize

F = np.float32
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _dev(v, idx):
    return torch.as_tensor(v, device=DEV), (None if idx is None else torch.as_tensor(idx.astype(np.int64), device=DEV))


def _grid_of(v, count, frac=0.1):
    lo, hi = meshes.extended_bbox(v, frac)
    return Grid.from_bounding_box(lo, hi, list(count))


def _raw(grid):
    return np.array(grid.get_first_cell(), F), np.array(grid.get_cell_size(), F), tuple(int(c) for c in grid.get_cell_count())


def _check(got: Voxels, want_occ, what):
    """occupancy, bits, cells and count of `got` against the model's occupancy."""
    assert isinstance(got, Voxels)
    occ = _np(got.occupancy)
    assert occ.dtype == np.uint8 and occ.shape == want_occ.shape, (what, occ.shape, want_occ.shape)
    bad = np.argwhere(occ != want_occ)
    assert bad.shape[0] == 0, f"{what}: occupancy differs on {bad.shape[0]} cells, first {bad[:5].tolist()} (got {occ[tuple(bad[0])]})"
    if got.bits is not None:
        assert np.array_equal(_np(got.bits).view(np.uint32), vm.pack_bits(want_occ)), f"{what}: bits"
    if got.cells is not None:
        cells = _np(got.cells).astype(np.uint64)
        assert np.array_equal(cells, np.flatnonzero(want_occ.reshape(-1)).astype(np.uint64)), f"{what}: cells"
    assert got.count == int(want_occ.sum()), f"{what}: count {got.count} != {int(want_occ.sum())}"


@pytest.fixture(scope="module")
def cases(suzanne):
    """name -> (vertices, indices, Grid, the model's SURFACE occupancy).  Computed once."""
    b12 = meshes.blob(12, 9)
    far = np.array([1.0e4, -1.0e4, 1.0e4], F)
    b12_far = ((b12[0] + far).astype(F), b12[1])
    deg, huge = sm.with_degenerates(*b12), sm.one_huge(*b12)
    nan = (b12[0].copy(), b12[1])
    nan[0][7, 1] = np.nan
    one = np.array([0, 1, 2], np.uint32)
    g12 = _grid_of(b12[0], (40, 24, 33))
    all_ = {"cube": (*meshes.cube(), _grid_of(meshes.cube()[0], (16, 16, 16))),
            "suzanne": (*suzanne, _grid_of(suzanne[0], (33, 20, 31))),
            "blob-192": (*b12, _grid_of(b12[0], (32, 32, 65))),
            "blob-192-far": (*b12_far, _grid_of(b12_far[0], (32, 32, 32))),
            "degenerates": (*deg, g12),
            "one-huge": (*huge, _grid_of(huge[0], (40, 24, 33))),          # the grid spans the far triangle too: its columns outnumber a workgroup
            "larger-than-the-grid": (np.array([[-50, -60, -9], [80, -10, 7], [-20, 90, 6]], F), one, g12),
            "wholly-outside": (np.array([[5, 5, 5], [6, 5, 5], [5, 6, 7]], F), one, g12),
            "nan-vertex": (*nan, g12),
            "one-cell": (*b12, _grid_of(b12[0], (1, 1, 1))),
            "empty": (np.zeros((0, 3), F), np.zeros(0, np.uint32), g12)}
    out = {}
    for name, (v, idx, grid) in all_.items():
        v, idx = np.ascontiguousarray(v, F), np.ascontiguousarray(idx, np.uint32)
        out[name] = (v, idx, grid, vm.surface(vm.triangles_of(v, idx), *_raw(grid))[0])
    assert out["one-huge"][3].sum() > 256 and out["larger-than-the-grid"][3].sum() > 256
    assert out["wholly-outside"][3].sum() == 0 and out["empty"][3].sum() == 0 and out["one-cell"][3].sum() == 1
    assert 0 < out["nan-vertex"][3].sum() < out["degenerates"][3].sum()
    return out


@pytest.fixture(scope="module")
def blob100k():
    v, idx = meshes.named("blob-100k")
    assert idx.size // 3 > 2 * 4096 and (idx.size // 3) % 4096 != 0           # several scan tiles, the last one short
    return _dev(v, idx) + (v,)


MESHES = ["cube", "suzanne", "blob-192", "blob-192-far", "degenerates", "one-huge", "larger-than-the-grid", "wholly-outside", "nan-vertex",
          "one-cell", "empty"]


# ---- 1. the default path is the model, in every output ----------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", MESHES)
def test_default_path_matches_the_model(cases, name, device):
    v, idx, grid, want = cases[name]
    a, b = _dev(v, idx) if device else (v, idx)
    topo = Topology.TriangleList(b)
    _check(voxelize(a, topo, grid, bits=True, cells=True), want, f"{name}: one shot")
    _check(voxelize(a, topo, grid, algorithm=1), want, f"{name}: one shot, algorithm 1")
    with Mesh(a, topo) as m:
        _check(m.voxelize(grid, bits=True, cells=True), want, f"{name}: Mesh")
        _check(m.voxelize(grid, algorithm=1, bits=True), want, f"{name}: Mesh, algorithm 1")


def test_index_widths_and_strips(cases):
    v, idx, grid, want = cases["blob-192"]
    _check(voxelize(v, Topology.TriangleList(idx.astype(np.uint16)), grid), want, "16-bit indices")
    _check(voxelize(v[idx], Topology.TriangleList(), grid), want, "no indices")
    strip = np.array([0, 1, 2, 3, 4, 5, 6], np.uint32)
    want_strip = vm.surface(vm.triangles_of(v, strip, 1), *_raw(grid))[0]
    assert want_strip.sum() > 0
    _check(voxelize(v, Topology.TriangleStrip(strip), grid, bits=True), want_strip, "strip")


@pytest.mark.parametrize("name,count", [("blob-6144", (64, 64, 64)), ("blob-100k", (64, 64, 64))])
def test_default_equals_all_pairs(blob100k, name, count):
    dv, di = blob100k[:2] if name == "blob-100k" else _dev(*meshes.blob(48, 65))
    grid = _grid_of(_np(dv), count)
    topo = Topology.TriangleList(di)
    fast = voxelize(dv, topo, grid, bits=True)
    slow = voxelize(dv, topo, grid, bits=True, algorithm=1)
    assert fast.count == slow.count and fast.count > 1000
    assert torch.equal(fast.occupancy, slow.occupancy) and torch.equal(fast.bits.view(torch.int32), slow.bits.view(torch.int32))


BIG = (1040, 1010, 8)                                                          # one mask word per row: 1 050 400 words, 257 scan tiles


def test_more_scan_tiles_than_threads():
    """The scan of the tile sums is one workgroup of 256 threads: with 257 tiles every thread walks two sums.  The cells come through the
    tile offsets and the occupancy does not, so the two check each other; algorithm 1 checks both."""
    v, idx = meshes.blob(12, 9)
    dv, di = _dev(v, idx)
    grid = _grid_of(v, BIG)
    topo = Topology.TriangleList(di)
    fast = voxelize(dv, topo, grid, bits=True, cells=True)
    slow = voxelize(dv, topo, grid, bits=True, algorithm=1)
    occ = _np(fast.occupancy).reshape(-1)
    want_cells = np.flatnonzero(occ).astype(np.uint64)
    n_tiles, held = vm.scan_tiles(want_cells, BIG)
    assert n_tiles > 256, n_tiles
    even = held[held % 2 == 0]
    assert np.isin(even + 1, held).any(), "no thread of the scan holds two tiles with set cells"
    assert torch.equal(fast.occupancy, slow.occupancy) and torch.equal(fast.bits.view(torch.int32), slow.bits.view(torch.int32))
    assert np.array_equal(_np(fast.cells).astype(np.uint64), want_cells)
    assert fast.count == slow.count == int(occ.sum()) > 0


# ---- 2. the outputs agree with each other -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solid", [False, True], ids=["surface", "solid"])
def test_outputs_agree_with_each_other(cases, solid):
    v, idx, grid, _ = cases["blob-192"]                                         # 32 x 32 x 65: three words per row, one live bit in the last
    for a, b in ((v, idx), _dev(v, idx)):
        r = voxelize(a, Topology.TriangleList(b), grid, solid, bits=True, cells=True)
        occ, bits, cells = _np(r.occupancy), _np(r.bits).view(np.uint32), _np(r.cells).astype(np.uint64)
        assert set(np.unique(occ)) <= {0, 1}
        assert np.array_equal(vm.unpack_bits(bits, 65), occ)
        assert (bits[:, :, 2] >> 1 == 0).all(), "padding bits"
        assert np.array_equal(cells, np.flatnonzero(occ.reshape(-1)).astype(np.uint64)) and (np.diff(cells.astype(np.int64)) > 0).all()
        assert r.count == int(occ.sum()) == cells.size > 0


def test_capacity_one_short(cases):
    v, idx, grid, want = cases["suzanne"]
    L = _lib.lib()
    n = int(want.sum())
    occ, bits = np.full(want.size, 9, np.uint8), np.full(33 * 20, 0xFFFFFFFF, np.uint32)
    cells = np.full(n, 12345, np.uint64)
    count = C.c_uint64(0)
    args = (v.ctypes.data, v.shape[0], idx.ctypes.data, idx.size, 4, 0, C.byref(grid._g), None)
    assert L.m2s_voxelize(*args, bits.ctypes.data, occ.ctypes.data, cells.ctypes.data, n - 1, C.byref(count), None) == _lib.ERR_BAD_ARG
    assert "cell_capacity" in _lib.last_error()
    assert count.value == n and (cells == 12345).all()
    assert np.array_equal(occ.reshape(want.shape), want) and np.array_equal(bits.reshape(33, 20, 1), vm.pack_bits(want))
    assert L.m2s_voxelize(*args, None, None, cells.ctypes.data, n, C.byref(count), None) == _lib.M2S_OK
    assert np.array_equal(cells, np.flatnonzero(want.reshape(-1)).astype(np.uint64))
    dv, di = _dev(v, idx)
    d_cells = torch.full((n,), 12345, dtype=torch.int64, device=DEV)
    o = _lib.M2SOpts()
    o.struct_size, o.device, o.mem_kind, o.synchronous = C.sizeof(_lib.M2SOpts), 0, _lib.MEM_DEVICE, 0
    count.value = 0
    rc = L.m2s_voxelize(dv.data_ptr(), v.shape[0], di.to(torch.int32).data_ptr(), idx.size, 4, 0, C.byref(grid._g), None, None, None,
                        d_cells.data_ptr(), n - 1, C.byref(count), C.byref(o))
    torch.cuda.synchronize()
    assert rc == _lib.ERR_BAD_ARG and count.value == n and bool((d_cells == 12345).all())


# ---- 3. SOLID ---------------------------------------------------------------------------------------------------------------------------------
def _solid_identity(v, idx, grid, what):
    topo = Topology.TriangleList(idx)
    surface, solid = voxelize(v, topo, grid, bits=True), voxelize(v, topo, grid, True, bits=True)
    d = generate_grid_sdf(v, topo, grid, SignMethod.Raycast)
    inside = (torch.signbit(d) if hasattr(d, "is_cuda") else torch.as_tensor(np.signbit(d))).reshape(solid.occupancy.shape).cpu().numpy()
    want = _np(surface.occupancy) | inside.astype(np.uint8)
    _check(solid, want, what)
    assert inside.sum() > 0 and (want != _np(surface.occupancy)).any(), what
    return surface, solid


@pytest.mark.parametrize("name,count", [("cube", (16, 16, 16)), ("suzanne", (48, 48, 48)), ("blob-100k", (128, 128, 128))])
def test_solid_is_surface_or_raycast_sign(cases, blob100k, name, count):
    if name == "blob-100k":
        dv, di, v = blob100k
    else:
        v, idx = cases[name][:2]
        dv, di = _dev(v, idx)
    grid = _grid_of(v, count)
    _solid_identity(dv, di, grid, f"{name}: device")
    if name != "blob-100k":
        _solid_identity(v, cases[name][1], grid, f"{name}: host")
        with Mesh(dv, Topology.TriangleList(di)) as m:
            want = voxelize(dv, Topology.TriangleList(di), grid, True)
            got = m.voxelize(grid, True, bits=True, cells=True)
            _check(got, _np(want.occupancy), f"{name}: Mesh, solid")
            _check(m.voxelize(grid, True, algorithm=1), _np(want.occupancy), f"{name}: Mesh, solid, algorithm 1")


def test_solid_on_an_open_mesh(cases):
    v, idx = cases["blob-192"][:2]
    open_idx = np.ascontiguousarray(idx.reshape(-1, 3)[5:-3].reshape(-1))      # a few triangles removed at both poles
    grid = _grid_of(v, (32, 32, 65))
    _solid_identity(v, open_idx, grid, "open mesh: host")
    _solid_identity(*_dev(v, open_idx), grid, "open mesh: device")


def test_an_empty_mesh_sets_nothing_in_both_modes(cases):
    v, idx, grid, want = cases["empty"]
    for a, b in ((v, idx), _dev(v, idx)):
        for solid in (False, True):
            _check(voxelize(a, Topology.TriangleList(b), grid, solid, bits=True, cells=True), want, "empty")


# ---- 4. against the distance field --------------------------------------------------------------------------------------------------------------
def test_set_cells_against_unsigned_distances(blob100k):
    """Every set cell's centre is within the cell's half diagonal of the mesh, and every cell whose centre is nearer than its smallest half
    extent is set.  The 1e-4 margin is derived, not measured: the rounding of the quantities involved is below 2^-20 times the largest
    coordinate, about 1e-6 here, two orders under 1e-4 h at h = 0.01."""
    dv, di, v = blob100k
    grid = _grid_of(v, (128, 128, 128))
    topo = Topology.TriangleList(di)
    occ = voxelize(dv, topo, grid).occupancy.reshape(-1).bool()
    d = generate_grid_sdf(dv, topo, grid, SignMethod.Raycast).abs()
    h = np.array(grid.get_cell_size(), np.float64) * 0.5
    assert 0.005 < h.min() < 0.02
    near = d < (1 - 1e-4) * h.min()
    assert int(occ.sum()) >= 1000 and int(near.sum()) >= 1000
    assert bool((d[occ] <= (1 + 1e-4) * np.linalg.norm(h)).all()), float(d[occ].max())
    assert bool(occ[near].all()), int((~occ[near]).sum())


# ---- 5. persistent meshes --------------------------------------------------------------------------------------------------------------------------
def test_mesh_before_and_after_a_grid_call_and_asynchronous_calls(cases):
    v, idx, grid, want = cases["suzanne"]
    dv, di = _dev(v, idx)
    cells = int(np.prod(want.shape))
    with Mesh(dv, Topology.TriangleList(di)) as m:
        _check(m.voxelize(grid, bits=True), want, "before")
        m.generate_grid_sdf(_grid_of(v, (24, 24, 24)))                          # re-marks the tree's leaves
        _check(m.voxelize(grid, bits=True, cells=True), want, "after a grid call")
        t = M2STimings()
        _check(m.voxelize(grid, timings=t), want, "timed")
        assert t.n_units == cells and t.n_triangles == idx.size // 3 and t.distance_ms > 0 and t.seed_ms == 0 and t.total_ms >= t.distance_ms
        m.voxelize(grid, True, timings=t)
        assert t.seed_ms > 0 and t.distance_ms > 0
        m.drain_timings()
        a = m.voxelize(grid, bits=True, synchronous=False)
        b = m.voxelize(grid, True, synchronous=False)
        d = m.drain_timings()
        assert d.n_units == 2 * cells and d.distance_launches == 2 and d.distance_ms > 0
        assert a.count is None and b.count is None
        assert np.array_equal(_np(a.occupancy), want) and np.array_equal(_np(a.bits).view(np.uint32), vm.pack_bits(want))
        assert np.array_equal(_np(b.occupancy), _np(voxelize(dv, Topology.TriangleList(di), grid, True).occupancy))
    t = M2STimings()
    _check(voxelize(dv, Topology.TriangleList(di), grid, timings=t), want, "one shot, timed")
    assert t.seed_ms == 0 and t.distance_ms > 0 and t.n_units == cells


def _build(tmp_path, cc, std, src, extra=()):
    exe = str(tmp_path / os.path.basename(src).split(".")[0])
    subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                           os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", *extra, "-o", exe])
    return exe


def test_c_and_cpp_consumers_run_clean(tmp_path):
    tet_v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    tet = vm.surface(vm.triangles_of(tet_v, np.array([0, 1, 2, 0, 2, 3])), np.full(3, 0.125, F), np.full(3, 0.25, F), (4, 4, 4))[0]
    exe = _build(tmp_path, "gcc", "-std=c99", "tests/c/voxelize_smoke.c", ["-lm"])
    r = subprocess.run([exe, str(int(tet.sum()))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    v, idx = meshes.cube()
    first, size, count = meshes.grid_from_bounding_box([-1.5] * 3, [1.5] * 3, (8, 8, 8))
    surface = vm.surface(vm.triangles_of(v, idx), first, size, count)[0]
    # (the Raycast sign of a cell whose grid lines run through the cube's face diagonals is the library's own business: the SOLID count comes
    # from the Python binding on the same input, the SURFACE count from the model)
    solid = voxelize(v, Topology.TriangleList(idx), Grid.from_bounding_box([-1.5] * 3, [1.5] * 3, [8, 8, 8]), True)
    assert np.array_equal(_raw(Grid.from_bounding_box([-1.5] * 3, [1.5] * 3, [8, 8, 8]))[0], first)
    assert surface.sum() == 152 and (_np(solid.occupancy) >= surface).all()
    exe = _build(tmp_path, "g++", "-std=c++17", "tests/cpp/voxelize_tests.cpp")
    r = subprocess.run([exe, str(int(surface.sum())), str(solid.count)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
