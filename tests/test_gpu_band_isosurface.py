"""m2s_band_isosurface on the GPU, bit for bit against tests/band_isosurface_model.py (the definition in numpy) and, where the band is wide
enough, against the library's own dense grid_isosurface: random fields with random active sets, real narrow bands of meshes at three iso
values under both sign rules, the same with a band too narrow, the count / capacity / NaN / validation contract, the call forms, and a
4.6e9-point grid whose cell indices pass 2^32.  Every comparison is exact equality of bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import band_isosurface_model as bim
import isosurface_model as im
import mesh_to_sdf_amd.api as api
from mesh_to_sdf_amd import (Grid, M2SError, M2SPanic, M2STimings, Mesh, NarrowBand, SignMethod, Topology, _lib, band_isosurface, generate_grid_sdf,
                             grid_isosurface, isosurface_band, meshes, narrow_band_sdf, remesh)

F = np.float32
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNS = [SignMethod.Raycast, SignMethod.Normal]


def _np(x):
    if hasattr(x, "cpu"):
        if x.dtype == getattr(torch, "uint32", None):
            x = x.view(torch.int32)
        x = x.cpu().numpy()
    return np.asarray(x)


def _same(got, want, what):
    got, want = np.ascontiguousarray(_np(got)), np.ascontiguousarray(_np(want))
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{what}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} values differ"


def _same_mesh(got, want, what):
    """(V, T[, n_open]) against (V, T[, n_open])."""
    _same(got[0], want[0], what + " vertices")
    _same(got[1], want[1], what + " indices")
    if len(got) > 2 and len(want) > 2:
        assert got[2] == want[2], f"{what}: n_open {got[2]} != {want[2]}"


def _differs(a, b):
    va, vb, ta, tb = _np(a[0]), _np(b[0]), _np(a[1]), _np(b[1])
    return va.shape != vb.shape or ta.shape != tb.shape or not np.array_equal(va.view(np.uint32), vb.view(np.uint32)) or \
        not np.array_equal(ta.view(np.uint32), tb.view(np.uint32))


def _dev(x, dtype=None):
    return torch.as_tensor(np.asarray(x).astype(dtype) if dtype else x, device=DEV)


# ---- 1. random fields with random active sets ----------------------------------------------------------------------------------------------------
def _random_grid(n, seed):
    rng = np.random.default_rng(seed)
    grid = Grid(rng.uniform(-1, 1, 3), rng.uniform(0.05, 0.3, 3), list(n))
    return rng, grid, im.GridI.of(grid)


@pytest.mark.parametrize("n", [(5, 7, 67), (9, 1, 9), (1, 6, 6), (2, 2, 2), (33, 20, 31)], ids=lambda n: "x".join(map(str, n)))
def test_random_fields_with_random_active_sets(n):
    """Uniform values in [-1, 1]: such fields are full of ambiguous faces.  5 x 7 x 67 has rows of nz that cross a 64-bit mask word."""
    rng, grid, g = _random_grid(n, sum(n))
    d = rng.uniform(-1, 1, n).astype(F).reshape(-1)
    nv = nt = opened = 0
    for k, frac in enumerate((1.0, 0.9, 0.5, 0.0)):
        active = rng.random(d.size) < frac
        cells, vals = np.flatnonzero(active).astype(np.uint64), d[active]
        for iso in (0.0, 0.25):
            want = bim.extract(g, cells, vals, iso)
            if k % 2:
                got = band_isosurface(grid, cells, vals, iso=iso)                                   # host arrays
            else:
                got = band_isosurface(grid, _dev(cells, np.int64), _dev(vals), iso=iso)             # device tensors
            _same_mesh(got, want, f"{n} fraction {frac} iso {iso}")
            if frac == 1.0:
                assert got[2] == 0
                _same_mesh(got, grid_isosurface(grid, _dev(d), iso=iso), f"{n} iso {iso}: all active against the dense call")
            if frac == 0.0:
                assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[2] == 0
            nv, nt, opened = nv + len(want[0]), nt + len(want[1]), opened + want[2]
    assert nv > 0 and (nt > 0) == (min(n) > 1) and (opened > 0) == (min(n) > 1 and d.size > 8)


def test_values_equal_to_iso_count_as_outside():
    """Values on a grid of eighths hit iso = 0 and iso = 0.25 exactly on many points: equality is outside, and the zero-area triangles
    that result are kept."""
    rng, grid, g = _random_grid((5, 7, 67), 99)
    d = (np.round(rng.uniform(-1, 1, g.n) * 8) / 8).astype(F).reshape(-1)
    for iso in (0.0, 0.25):
        assert 50 < int((d == F(iso)).sum())
        for frac in (1.0, 0.9):
            active = rng.random(d.size) < frac
            cells, vals = np.flatnonzero(active).astype(np.uint64), d[active]
            want = bim.extract(g, cells, vals, iso)
            _same_mesh(band_isosurface(grid, _dev(cells, np.int64), _dev(vals), iso=iso), want, f"ties, iso {iso}, fraction {frac}")
            v = want[0][want[1].astype(np.int64)]
            assert (np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1) == 0).any(), "no zero-area triangle: the case is not covered"


# ---- 2. real bands -----------------------------------------------------------------------------------------------------------------------------------
def _grid_of(v, count, frac=0.1):
    lo, hi = meshes.extended_bbox(v, frac)
    return Grid.from_bounding_box(lo, hi, list(count))


@pytest.fixture(scope="module")
def real(suzanne):
    """(name, sign) -> (vertices, topology, Grid, the dense grid on the device, the same on the host), computed once and left unchanged."""
    b11 = meshes.named("blob-11k")
    inputs = {"suzanne-64": (suzanne, (64, 64, 64)), "blob-768-64": (meshes.blob(slices=24, stacks=17), (64, 64, 64)),
              "blob-11k-96": (b11, (96, 96, 96)), "ragged": (b11, (70, 45, 83))}
    out = {}
    for name, ((v, idx), count) in inputs.items():
        grid = _grid_of(v, count)
        dv, topo = _dev(v), Topology.TriangleList(_dev(idx, np.int64).reshape(-1))
        for sign in SIGNS:
            d = generate_grid_sdf(dv, topo, grid, sign)
            out[(name, sign)] = (dv, topo, grid, d, d.cpu().numpy().reshape(-1))
    return out


def _isos(grid):
    h = float(min(grid.get_cell_size()))
    return [0.0, 1.5 * h, -1.0 * h]


def _active(cells, size):
    a = np.zeros(size, bool)
    a[_np(cells).astype(np.int64)] = True
    return a


# Suzanne is not watertight: on the reference's own arithmetic its grid at 64^3 has cells of mixed sign far from the surface under either
# sign rule, at all three iso values, so the corollary's condition fails and no band of finite width gives the dense mesh.  A watertight
# blob of 768 triangles takes its place at 64^3 where the dense mesh is the yardstick; suzanne stays where the model is.
WATERTIGHT = [(n, s) for n in ("blob-768-64", "blob-11k-96", "ragged") for s in SIGNS]
REAL = [(n, s) for n in ("suzanne-64", "blob-768-64", "blob-11k-96", "ragged") for s in SIGNS]
_ids = lambda cases: [f"{n}-{s.name.lower()}" for n, s in cases]   # noqa: E731


@pytest.mark.parametrize("name,sign", WATERTIGHT, ids=_ids(WATERTIGHT))
def test_a_band_of_one_diagonal_gives_the_dense_mesh(real, name, sign):
    dv, topo, grid, d, dh = real[(name, sign)]
    g = im.GridI.of(grid)
    for iso in _isos(grid):
        band = narrow_band_sdf(dv, topo, grid, isosurface_band(grid, iso), sign)
        assert 0 < band.count < dh.size // 2
        assert bim.covered(g, dh, _active(band.cells, dh.size), iso), f"{name} {sign} iso {iso}: a cut cell has a corner outside the band"
        want = grid_isosurface(grid, d, iso=iso)
        assert len(want[1]) > 0
        got = band.isosurface(iso)
        assert got[0].is_cuda and got[1].is_cuda
        _same_mesh(got, (_np(want[0]), _np(want[1]), 0), f"{name} {sign} iso {iso}")


# ---- 3. the same with half that band ----------------------------------------------------------------------------------------------------------------
def _half_band(grid, iso):
    w = 0.5 * 1.001 * float(np.sqrt((np.asarray(grid.get_cell_size(), np.float64) ** 2).sum()))
    return max(0.0, w - iso), max(0.0, iso + w)


@pytest.mark.parametrize("name,sign", REAL, ids=_ids(REAL))
def test_half_that_band_is_the_model_and_not_the_dense_mesh(real, name, sign):
    dv, topo, grid, d, dh = real[(name, sign)]
    g = im.GridI.of(grid)
    for iso in _isos(grid):
        band = narrow_band_sdf(dv, topo, grid, _half_band(grid, iso), sign)
        got = band.isosurface(iso)
        want = bim.extract(g, _np(band.cells).astype(np.uint64), _np(band.distances), iso)
        _same_mesh(got, want, f"{name} {sign} iso {iso}, half band")
        assert got[2] > 0 and len(want[1]) > 0
        assert _differs(got, grid_isosurface(grid, d, iso=iso))


def test_remesh_is_the_dense_mesh_and_raises_on_a_narrow_band(real, monkeypatch):
    dv, topo, grid, d, _ = real[("blob-11k-96", SignMethod.Raycast)]
    h = float(min(grid.get_cell_size()))
    for iso in (0.0, -1.0 * h):
        want = grid_isosurface(grid, d, iso=iso)
        _same_mesh(remesh(dv, topo, grid, iso=iso), want, f"remesh iso {iso}")
    dn = real[("blob-11k-96", SignMethod.Normal)][3]
    _same_mesh(remesh(dv, topo, grid, iso=0.5 * h, sign_method=SignMethod.Normal), grid_isosurface(grid, dn, iso=0.5 * h), "remesh, Normal")
    with Mesh(dv, topo) as m:
        _same_mesh(m.remesh(grid, iso=0.5 * h), grid_isosurface(grid, d, iso=0.5 * h), "Mesh.remesh")
        monkeypatch.setattr(api, "isosurface_band", _half_band)
        with pytest.raises(M2SError, match="too narrow"):
            m.remesh(grid)
    with pytest.raises(M2SError, match="too narrow"):
        remesh(dv, topo, grid, iso=0.5 * h)


# ---- 4. counting, capacity, NaN, validation -------------------------------------------------------------------------------------------------------
def _opts(device_mem, stream=None, stream_mode=0, timings=None):
    o = _lib.M2SOpts()
    o.struct_size = C.sizeof(o)
    o.device = 0
    o.mem_kind = _lib.MEM_DEVICE if device_mem else _lib.MEM_HOST
    o.stream = stream
    o.stream_mode = stream_mode
    o.synchronous = 0
    if timings is not None:
        o.timings = C.pointer(timings)
    return o


@pytest.fixture(scope="module")
def small_band():
    """A random field on 12 x 11 x 13 with 80 % of its points active: (Grid, cells u64, values, the model's result)."""
    rng, grid, g = _random_grid((12, 11, 13), 5)
    d = rng.uniform(-1, 1, g.n).astype(F).reshape(-1)
    active = rng.random(d.size) < 0.8
    cells, vals = np.flatnonzero(active).astype(np.uint64), d[active]
    return grid, cells, vals, bim.extract(g, cells, vals, 0.1)


def test_counts_capacity_and_nan(small_band):
    grid, cells, vals, (wv, wt, w_open) = small_band
    L = _lib.lib()
    G = C.byref(grid._g)
    nv, nt = len(wv), len(wt)
    assert nv > 0 and nt > 0 and w_open > 0
    cnt = (C.c_uint64 * 3)()
    t = M2STimings()
    iso = F(0.1)
    assert L.m2s_band_isosurface(G, cells.ctypes.data, vals.ctypes.data, cells.size, iso, None, 0, None, 0, cnt, C.byref(_opts(False, timings=t))) == _lib.M2S_OK
    assert list(cnt) == [nv, nt, w_open] and t.n_units == cells.size and t.distance_ms > 0
    sentinel = F(-7.0)
    v = np.full((nv + 4, 3), sentinel, F)
    tri = np.full((nt + 4, 3), 0xABCDEF01, np.uint32)
    dc, dd = _dev(cells, np.int64), _dev(vals)
    dv = torch.full((nv + 4, 3), -7.0, dtype=torch.float32, device=DEV)
    dt = torch.full((nt + 4, 3), 0x0BCDEF01, dtype=torch.int32, device=DEV)
    for cv, ct in [(nv - 1, nt), (nv, nt - 1), (0, 0)]:
        cnt[0] = cnt[1] = cnt[2] = 0
        assert L.m2s_band_isosurface(G, cells.ctypes.data, vals.ctypes.data, cells.size, iso, v.ctypes.data, cv, tri.ctypes.data, ct, cnt, None) == _lib.ERR_BAD_ARG
        assert "capacity" in _lib.last_error() and list(cnt) == [nv, nt, w_open]
        assert (v == sentinel).all() and (tri == 0xABCDEF01).all()
        cnt[0] = cnt[1] = cnt[2] = 0
        rc = L.m2s_band_isosurface(G, dc.data_ptr(), dd.data_ptr(), cells.size, iso, dv.data_ptr(), cv, dt.data_ptr(), ct, cnt, C.byref(_opts(True)))
        torch.cuda.synchronize()
        assert rc == _lib.ERR_BAD_ARG and list(cnt) == [nv, nt, w_open] and bool((dv == -7.0).all()) and bool((dt == 0x0BCDEF01).all())
    assert L.m2s_band_isosurface(G, cells.ctypes.data, vals.ctypes.data, cells.size, iso, v.ctypes.data, nv, tri.ctypes.data, nt, cnt, None) == _lib.M2S_OK
    _same(v[:nv], wv, "host vertices")
    _same(tri[:nt], wt, "host indices")
    assert (v[nv:] == sentinel).all() and (tri[nt:] == 0xABCDEF01).all()                  # nothing past the counts
    assert L.m2s_band_isosurface(G, dc.data_ptr(), dd.data_ptr(), cells.size, iso, dv.data_ptr(), nv + 4, dt.data_ptr(), nt + 4, cnt,
                                 C.byref(_opts(True))) == _lib.M2S_OK
    _same(dv[:nv], wv, "device vertices")
    _same(dt[:nt], wt.view(np.int32), "device indices")
    assert bool((dv[nv:] == -7.0).all()) and bool((dt[nt:] == 0x0BCDEF01).all())
    for bad in (np.nan, np.inf, -np.inf):
        vb = vals.copy()
        vb[len(vb) // 3] = bad
        v[:], tri[:] = sentinel, 0xABCDEF01
        cnt[0] = cnt[1] = cnt[2] = 9
        rc = L.m2s_band_isosurface(G, cells.ctypes.data, vb.ctypes.data, cells.size, iso, v.ctypes.data, nv + 4, tri.ctypes.data, nt + 4, cnt, None)
        assert rc == _lib.ERR_NAN and list(cnt) == [0, 0, 0] and (v == sentinel).all() and (tri == 0xABCDEF01).all(), bad
        dv[:] = -7.0
        rc = L.m2s_band_isosurface(G, dc.data_ptr(), _dev(vb).data_ptr(), cells.size, iso, dv.data_ptr(), nv + 4, dt.data_ptr(), nt + 4, cnt, C.byref(_opts(True)))
        torch.cuda.synchronize()
        assert rc == _lib.ERR_NAN and list(cnt) == [0, 0, 0] and bool((dv == -7.0).all()), bad
        with pytest.raises(M2SPanic) as e:
            band_isosurface(grid, dc, _dev(vb), iso=0.1)
        assert e.value.code == _lib.ERR_NAN
    # f32::MAX is finite and legal: a band with exterior = +inf holds it
    vm = vals.copy()
    vm[::7] = np.finfo(F).max
    _same_mesh(band_isosurface(grid, dc, _dev(vm), iso=0.1), bim.extract(im.GridI.of(grid), cells, vm, 0.1), "f32::MAX")


def test_device_lists_that_do_not_ascend_are_refused_and_the_next_call_is_correct(small_band):
    grid, cells, vals, want = small_band
    L = _lib.lib()
    G = C.byref(grid._g)
    total = grid.get_total_cell_count()
    nv, nt = len(want[0]), len(want[1])
    dd = _dev(vals)
    cnt = (C.c_uint64 * 3)()
    swapped, dup, far, huge, neg = (cells.copy() for _ in range(5))
    swapped[[100, 101]] = swapped[[101, 100]]
    dup[500] = dup[499]
    far[-1] = total
    huge[-1] = 2 ** 63 + 5
    neg[0] = np.uint64(2 ** 64 - 1)
    for name, bad in (("swapped", swapped), ("duplicate", dup), ("at the cell count", far), ("huge", huge), ("negative as int64", neg)):
        dv = torch.full((nv + 4, 3), -7.0, dtype=torch.float32, device=DEV)
        dt = torch.full((nt + 4, 3), 0x0BCDEF01, dtype=torch.int32, device=DEV)
        dc = _dev(bad.view(np.int64))
        cnt[0] = cnt[1] = cnt[2] = 0
        rc = L.m2s_band_isosurface(G, dc.data_ptr(), dd.data_ptr(), cells.size, F(0.1), dv.data_ptr(), nv + 4, dt.data_ptr(), nt + 4, cnt, C.byref(_opts(True)))
        torch.cuda.synchronize()
        assert rc == _lib.ERR_BAD_ARG and "ascending" in _lib.last_error(), name
        assert bool((dv == -7.0).all()) and bool((dt == 0x0BCDEF01).all()), name
        with pytest.raises(M2SPanic):
            band_isosurface(grid, dc, dd, iso=0.1)
        _same_mesh(band_isosurface(grid, _dev(cells, np.int64), dd, iso=0.1), want, f"the call after '{name}'")


# ---- 5. call forms -----------------------------------------------------------------------------------------------------------------------------------
def test_host_device_and_stream_give_the_same_bits(small_band):
    grid, cells, vals, want = small_band
    host = band_isosurface(grid, cells, vals, iso=0.1)
    assert isinstance(host[0], np.ndarray) and host[1].dtype == np.uint32
    _same_mesh(host, want, "host arrays")
    _same_mesh(band_isosurface(grid, cells.astype(np.int64), vals, iso=0.1), want, "host arrays, int64 cells")
    dc, dd = _dev(cells, np.int64), _dev(vals)
    dev = band_isosurface(grid, dc, dd, iso=0.1)
    assert dev[0].is_cuda and dev[1].is_cuda and dc.dtype == torch.int64
    _same_mesh(dev, want, "device tensors")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        t = M2STimings()
        on = NarrowBand(dc, dd, None, int(dc.numel()), grid).isosurface(0.1, timings=t)
    s.synchronize()
    _same_mesh(on, want, "a torch stream")
    assert t.n_units == cells.size and t.distance_ms > 0
    L = _lib.lib()
    cnt = (C.c_uint64 * 3)()
    for stream_mode, own in [(0, True), (1, True), (1, False)]:
        st = torch.cuda.Stream() if own else None
        vo = torch.zeros((len(want[0]), 3), dtype=torch.float32, device=DEV)
        to = torch.zeros((len(want[1]), 3), dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        rc = L.m2s_band_isosurface(C.byref(grid._g), dc.data_ptr(), dd.data_ptr(), cells.size, F(0.1), vo.data_ptr(), len(want[0]), to.data_ptr(), len(want[1]),
                                   cnt, C.byref(_opts(True, st.cuda_stream if st is not None else None, stream_mode)))
        assert rc == _lib.M2S_OK, _lib.last_error()
        _same_mesh((vo, to, int(cnt[2])), (want[0], want[1].view(np.int32), want[2]), f"stream_mode {stream_mode}")


def _build(tmp_path, cc, std, src, extra=()):
    exe = str(tmp_path / os.path.basename(src).split(".")[0])
    subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                           os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", *extra, "-o", exe])
    return exe


def test_c_and_cpp_consumers_run_clean(tmp_path):
    exe = _build(tmp_path, "gcc", "-std=c99", "tests/c/band_isosurface_smoke.c", ["-lm"])
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    exe = _build(tmp_path, "g++", "-std=c++17", "tests/cpp/band_isosurface_tests.cpp")
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


# ---- 6. 64-bit offsets ---------------------------------------------------------------------------------------------------------------------------------
def _block(n, lo, side=6):
    """The cells of a side^3 block with lowest corner `lo`, ascending, as a device tensor."""
    r = [torch.arange(lo[a], lo[a] + side, dtype=torch.int64, device=DEV) for a in range(3)]
    return (r[0].view(-1, 1, 1) * (n[1] * n[2]) + r[1].view(1, -1, 1) * n[2] + r[2].view(1, 1, -1)).reshape(-1)


def test_cell_indices_beyond_32_bits():
    """2048 x 2048 x 1100 = 4.6e9 points: the mask is 0.58 GB and no array of distances exists, on the device or the host.  Two 6^3 blocks
    of active points with random values: one that straddles L = 2^32 = (1906, 1027, 796) and one at the grid's high corner."""
    n = (2048, 2048, 1100)
    grid = Grid([-3.0, 0.5, 2.0], [0.01, 0.02, 0.015], list(n))
    g = im.GridI.of(grid)
    lo_b, lo_a = (1904, 1025, 794), (2042, 2042, 1094)
    cb, ca = _block(n, lo_b), _block(n, lo_a)
    assert int(cb[0]) < 2 ** 32 < int(cb[-1]) and int((cb < 2 ** 32).sum()) > 50 and int((cb >= 2 ** 32).sum()) > 50
    assert int(ca[-1]) == n[0] * n[1] * n[2] - 1 and int(cb[-1]) < int(ca[0])
    gen = torch.Generator(device=DEV)
    gen.manual_seed(7)
    vals = torch.rand(432, generator=gen, device=DEV) * 2 - 1
    got = band_isosurface(grid, torch.cat([cb, ca]), vals)
    vh = vals.cpu().numpy()
    # the lower block's box has a layer of inactive points on every high side (no cell it owns is cut off); the upper one ends with the grid
    wb = bim.extract_box(g, tuple((lo_b[a], lo_b[a] + 7) for a in range(3)), cb.cpu().numpy(), vh[:216], 0.0)
    wa = bim.extract_box(g, tuple((lo_a[a], n[a]) for a in range(3)), ca.cpu().numpy(), vh[216:], 0.0)
    assert len(wb[1]) > 50 and len(wa[1]) > 50 and wb[2] > 0 and wa[2] == 0
    want = (np.concatenate([wb[0], wa[0]]), np.concatenate([wb[1], wa[1] + np.uint32(len(wb[0]))]), wb[2] + wa[2])
    _same_mesh(got, want, "two blocks of a 4.6e9-point grid")
