"""m2s_grid_isosurface on the MI355X, bit for bit against the test oracle tests/isosurface_model.py: grids the library generates itself
(iso 0, +-half a cell, and a value equal to a grid value), x-slabs of a 512^3 grid and of a 4.2 GB grid (64-bit offsets), a round trip
through generate_grid_sdf, the count / capacity / NaN contract, host / device / torch memory, caller streams and lanes, and the C and
C++ programs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import isosurface_model as im
from mesh_to_sdf_amd import (M2STimings, SignMethod, Topology, _lib, closest_points, generate_grid_sdf, grid_isosurface, meshes)
from mesh_to_sdf_amd.api import Grid

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid_sdf(v, idx, grid, sign=SignMethod.Raycast):
    return generate_grid_sdf(torch.as_tensor(v, device="cuda:0"), Topology.TriangleList(torch.as_tensor(idx.astype(np.int64).reshape(-1), device="cuda:0")),
                             grid, sign)


def _cubic(v, n):
    lo, hi = meshes.extended_bbox(v, 0.1)
    return Grid.from_bounding_box(lo, hi, [n, n, n])


@pytest.fixture(scope="module")
def grids(suzanne):
    out = {"suzanne-64": (_cubic(suzanne[0], 64),) + tuple(suzanne)}
    for name in ("blob-11k", "blob-100k"):
        v, idx = meshes.named(name)
        out[name + "-128"] = (_cubic(v, 128), v, idx)
    v, idx = meshes.named("blob-11k")
    lo, hi = meshes.extended_bbox(v, 0.1)
    n = np.array([37, 64, 50])
    cs = ((hi - lo) / n * np.array([1.0, 0.93, 1.17])).astype(F)          # unequal cell sizes, a box that does not fit the mesh
    out["ragged"] = (Grid(lo + cs / 2, cs, n.tolist()), v, idx)
    return {k: (g, _grid_sdf(v, idx, g), v, idx) for k, (g, v, idx) in out.items()}


def _np(x):
    if hasattr(x, "cpu"):
        if x.dtype == getattr(torch, "uint32", None):
            x = x.view(torch.int32)
        x = x.cpu().numpy()
    return x


def _same(got, want, what):
    got, want = np.ascontiguousarray(_np(got)), np.ascontiguousarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{what}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} values differ"


def _isos(grid, dh):
    h = float(min(grid.get_cell_size()))
    near = dh[np.argsort(np.abs(dh))[len(dh) // 1000]]   # a value of the grid itself, near the surface: zero-area triangles
    return [0.0, 0.5 * h, -0.5 * h, float(near)]


@pytest.mark.parametrize("name", ["suzanne-64", "blob-11k-128", "blob-100k-128", "ragged"])
def test_extraction_is_bit_exact(grids, name):
    grid, d, _, _ = grids[name]
    g = im.GridI.of(grid)
    dh = d.cpu().numpy()
    for iso in _isos(grid, dh):
        v, t = grid_isosurface(grid, d, iso=iso)
        wv, wt = im.extract(g, dh, F(iso))
        assert len(wt) > 0
        _same(v, wv, f"{name} iso {iso} vertices")
        _same(t, wt, f"{name} iso {iso} indices")


# ---- x-slabs of large grids, with counts of the layers before them computed by torch on the device ---------------------------------
_TRI_COUNT = None


def _torch_counts(d3, iso, x0, x1, chunk=32):
    """isosurface_model.counts on the device: crossing edges of the points and triangles of the cells in layers [x0, x1)."""
    global _TRI_COUNT
    if _TRI_COUNT is None:
        _TRI_COUNT = torch.as_tensor(im.TRI_COUNT, device=d3.device)
    nx = d3.shape[0]
    nv = nt = 0
    for a in range(x0, x1, chunk):
        b = min(a + chunk, x1)
        ins = d3[a:min(b + 1, nx)] < float(iso)
        own = ins[:b - a]
        nv += int((own[:, :-1] != own[:, 1:]).sum()) + int((own[:, :, :-1] != own[:, :, 1:]).sum())
        nxe = min(b - a, ins.shape[0] - 1)
        nv += int((ins[:nxe] != ins[1:nxe + 1]).sum())
        if nxe > 0:
            ny, nz = d3.shape[1] - 1, d3.shape[2] - 1
            case = torch.zeros((nxe, ny, nz), dtype=torch.int64, device=d3.device)
            for dx in (0, 1):
                for dy in (0, 1):
                    for dz in (0, 1):
                        case |= ins[dx:dx + nxe, dy:dy + ny, dz:dz + nz].to(torch.int64) << (4 * dx + 2 * dy + dz)
            nt += int(_TRI_COUNT[case].sum())
    return nv, nt


def _check_slab(g, d3, v, t, iso, x0, x1, what):
    layers = lambda a, b: d3[a:b].cpu().numpy()
    vb, tb = _torch_counts(d3, F(iso), 0, x0)
    nx = g.n[0]
    xe = min(x1 + 1, nx)
    d = layers(x0, min(xe + 1, nx))
    inside = d < F(iso)
    pv, keys = im._vertices(g, d, im._crossings(inside, xe - x0, nx - x0), x0, iso)
    tt = im._triangles(g, im._cases(inside, min(x1, nx - 1) - x0), x0, keys, vb).astype(np.uint32)
    assert len(tt) > 0, what
    _same(_np(v[vb:vb + len(pv)]), pv, f"{what} vertices")
    got_t = _np(t[tb:tb + len(tt)])
    _same(got_t, tt, f"{what} indices")
    _same(_np(v)[got_t.astype(np.int64)] if not hasattr(v, "cpu") else v[torch.as_tensor(got_t.astype(np.int64), device=v.device)],
          pv[(tt.astype(np.int64) - vb)], f"{what} triangle corners")


def test_torch_counts_equal_the_model(grids):
    grid, d, _, _ = grids["ragged"]
    g = im.GridI.of(grid)
    d3 = d.view(*g.n)
    dh = d.cpu().numpy().reshape(g.n)
    for x0, x1 in [(0, 10), (10, 37)]:
        assert _torch_counts(d3, F(0.0), x0, x1, chunk=4) == im.counts(g, lambda a, b: dh[a:b], 0.0, x0, x1, chunk=5)


def test_512_grid_slabs():
    v_m, idx = meshes.named("blob-100k")
    grid = _cubic(v_m, 512)
    d = _grid_sdf(v_m, idx, grid)
    g = im.GridI.of(grid)
    v, t = grid_isosurface(grid, d)
    d3 = d.view(*g.n)
    for x0, x1 in [(60, 64), (255, 259), (440, 444)]:
        _check_slab(g, d3, v, t, 0.0, x0, x1, f"512^3 slab {x0}")
    assert _torch_counts(d3, F(0.0), 0, 512) == (v.shape[0], t.shape[0])


def test_large_grid_64_bit_offsets():
    # 1040 x 1024 x 1024 points (4.2 GB): a sphere cut by the grid's faces; the far end's byte offsets exceed 2^32
    n = (1040, 1024, 1024)
    grid = Grid([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], n)
    g = im.GridI.of(grid)
    xs = (torch.arange(n[0], dtype=torch.float32, device="cuda:0") - 520.0).view(-1, 1, 1)
    ys = (torch.arange(n[1], dtype=torch.float32, device="cuda:0") - 511.5).view(1, -1, 1)
    zs = (torch.arange(n[2], dtype=torch.float32, device="cuda:0") - 512.25).view(1, 1, -1)
    d = (torch.sqrt(xs * xs + ys * ys + zs * zs) - 530.0).reshape(-1)
    v, t = grid_isosurface(grid, d)
    d3 = d.view(*n)
    for x0, x1 in [(0, 3), (518, 521), (1036, 1040)]:
        _check_slab(g, d3, v, t, 0.0, x0, x1, f"large grid slab {x0}")
    del d, d3, v, t


# ---- a round trip through the library ------------------------------------------------------------------------------------------------
def test_round_trip_through_generate_grid_sdf(grids):
    grid, d, vm, im_idx = grids["blob-100k-128"]
    v, t = grid_isosurface(grid, d)
    v, t = _np(v), _np(t).astype(np.int64)
    h = float(max(grid.get_cell_size()))
    _, _, dist = closest_points(vm, Topology.TriangleList(im_idx), v)
    assert float(np.max(dist)) <= h
    e = im.directed_edges(t)
    n = len(v)
    k = np.sort(e[:, 0] * n + e[:, 1])
    r = np.sort(e[:, 1] * n + e[:, 0])
    assert np.array_equal(k, r)   # closed: every directed edge as often as its reverse
    # the extracted vertices lie on the grid's lines, where the Raycast grid path casts its rays: evaluate on a grid shifted by a
    # fraction of a cell, against the source mesh on that grid
    cs = np.array(grid.get_cell_size(), F)
    shifted = Grid((np.array(grid.get_first_cell(), F) + cs * F(0.37)).astype(F), cs, grid.get_cell_count())
    ref = _grid_sdf(vm, im_idx, shifted).cpu().numpy()
    far = np.abs(ref) > 2 * h * np.sqrt(3)
    for sign in (SignMethod.Raycast, SignMethod.Normal):
        d2 = _grid_sdf(v, t.astype(np.uint32), shifted, sign).cpu().numpy()
        bad = int(((d2[far] < 0) != (ref[far] < 0)).sum())
        assert bad == 0, f"{sign}: {bad} of {int(far.sum())} far cells change sign"


# ---- the count / capacity / NaN contract and the memory kinds ------------------------------------------------------------------------
def _opts(device_mem, stream=None, stream_mode=0, lane=0, timings=None):
    o = _lib.M2SOpts()
    o.struct_size = C.sizeof(o)
    o.device = 0
    o.mem_kind = _lib.MEM_DEVICE if device_mem else _lib.MEM_HOST
    o.stream = stream
    o.stream_mode = stream_mode
    o.lane = lane
    o.synchronous = 0
    if timings is not None:
        o.timings = C.pointer(timings)
    return o


def test_counts_capacity_and_nan(grids):
    grid, d, _, _ = grids["suzanne-64"]
    L = _lib.lib()
    G = C.byref(grid._g)
    dh = d.cpu().numpy()
    wv, wt = im.extract(im.GridI.of(grid), dh)
    cnt = (C.c_uint64 * 2)()
    t = M2STimings()
    assert L.m2s_grid_isosurface(G, dh.ctypes.data, 0.0, None, 0, None, 0, cnt, C.byref(_opts(False, timings=t))) == _lib.M2S_OK
    assert (cnt[0], cnt[1]) == (len(wv), len(wt)) and t.n_units == dh.size and t.distance_ms > 0
    nv, nt = len(wv), len(wt)
    sentinel = np.float32(-7.0)
    v = np.full((nv + 4, 3), sentinel, F)
    tri = np.full((nt + 4, 3), 0xABCDEF01, np.uint32)
    for cv, ct in [(nv - 1, nt), (nv, nt - 1), (0, 0)]:
        cnt[0] = cnt[1] = 0
        rc = L.m2s_grid_isosurface(G, dh.ctypes.data, 0.0, v.ctypes.data, cv, tri.ctypes.data, ct, cnt, None)
        assert rc == _lib.ERR_BAD_ARG and (cnt[0], cnt[1]) == (nv, nt)
        assert (v == sentinel).all() and (tri == 0xABCDEF01).all()
    assert L.m2s_grid_isosurface(G, dh.ctypes.data, 0.0, v.ctypes.data, nv, tri.ctypes.data, nt, cnt, None) == _lib.M2S_OK
    _same(v[:nv], wv, "host vertices")
    _same(tri[:nt], wt, "host indices")
    assert (v[nv:] == sentinel).all() and (tri[nt:] == 0xABCDEF01).all()   # nothing past the counts
    for bad in (np.nan, np.inf, -np.inf):
        db = dh.copy()
        db[len(db) // 3] = bad
        v[:] = sentinel
        rc = L.m2s_grid_isosurface(G, db.ctypes.data, 0.0, v.ctypes.data, nv + 4, tri.ctypes.data, nt + 4, cnt, None)
        assert rc == _lib.ERR_NAN and (v == sentinel).all(), bad
        with pytest.raises(Exception):
            grid_isosurface(grid, torch.as_tensor(db, device="cuda:0"))
    # one layer: vertices, no triangles
    g1 = Grid([0, 0, 0], [1, 1, 1], [1, 6, 5])
    d1 = (np.arange(30, dtype=F) - 14.5).astype(F)
    v1, t1 = grid_isosurface(g1, d1)
    w1, _ = im.extract(im.GridI.of(g1), d1)
    assert len(t1) == 0 and len(v1) == len(w1) > 0
    _same(v1, w1, "one layer")


def test_host_device_torch_streams_and_lanes(grids):
    grid, d, _, _ = grids["blob-11k-128"]
    G = C.byref(grid._g)
    dh = d.cpu().numpy()
    wv, wt = im.extract(im.GridI.of(grid), dh, F(0.01))
    vh, th = grid_isosurface(grid, dh, iso=0.01)
    _same(vh, wv, "host vertices")
    _same(th, wt, "host indices")
    vd, td = grid_isosurface(grid, d, iso=0.01)
    assert vd.is_cuda and td.is_cuda
    _same(vd, wv, "torch vertices")
    _same(td, wt, "torch indices")
    L = _lib.lib()
    cnt = (C.c_uint64 * 2)()
    for stream_mode, lane, own in [(0, 0, True), (1, 0, True), (1, 0, False), (0, 1, True)]:
        s = torch.cuda.Stream() if own else None
        vo = torch.zeros((len(wv), 3), dtype=torch.float32, device="cuda:0")
        to = torch.zeros((len(wt), 3), dtype=torch.int32, device="cuda:0")
        o = _opts(True, s.cuda_stream if s is not None else None, stream_mode, lane)
        torch.cuda.synchronize()
        rc = L.m2s_grid_isosurface(G, d.data_ptr(), F(0.01), vo.data_ptr(), len(wv), to.data_ptr(), len(wt), cnt, C.byref(o))
        assert rc == _lib.M2S_OK, _lib.last_error()
        assert (cnt[0], cnt[1]) == (len(wv), len(wt))
        _same(vo, wv, f"stream_mode {stream_mode} lane {lane}")
        _same(to, wt.view(np.int32), f"stream_mode {stream_mode} lane {lane} indices")


def test_c_and_cpp_programs(tmp_path):
    common = ["-L", os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
              "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib"]
    for cc, std, src in [("gcc", "-std=c99", "tests/c/isosurface_smoke.c"), ("g++", "-std=c++17", "tests/cpp/isosurface_tests.cpp")]:
        exe = str(tmp_path / os.path.basename(src).split(".")[0])
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src)] + common
                              + (["-lm"] if cc == "gcc" else []) + ["-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
