"""Grid queries on the MI355X (include/m2s.h m2s_sample_grid / m2s_raymarch_grid), bit for bit against the test oracle
tests/grid_query_model.py: grids the library generates itself, every sampling mode, iso and point set, normals, ray marching,
large grids (64-bit cell offsets), host / device / torch memory, caller streams, and the C and C++ programs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import grid_query_model as gqm
from mesh_to_sdf_amd import M2STimings, SampleMode, SignMethod, Topology, _lib, generate_grid_sdf, meshes, raymarch_grid, sample_grid
from mesh_to_sdf_amd.api import Grid

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [SampleMode.Snap, SampleMode.Trilinear, SampleMode.Tetrahedral]


def _grid_sdf(v, idx, n):
    lo, hi = meshes.extended_bbox(v, 0.1)
    grid = Grid.from_bounding_box(lo, hi, [n, n, n])
    d = generate_grid_sdf(torch.as_tensor(v, device="cuda:0"), Topology.TriangleList(torch.as_tensor(idx.astype(np.int64), device="cuda:0")),
                          grid, SignMethod.Raycast)
    return grid, d


@pytest.fixture(scope="module")
def grids(suzanne):
    out = {"suzanne-64": _grid_sdf(*suzanne, 64)}
    for name in ("blob-11k", "blob-100k"):
        out[name + "-128"] = _grid_sdf(*meshes.named(name), 128)
    return out


def _point_sets(q, seed):
    rng = np.random.default_rng(seed)
    lo, hi = q.start.astype(np.float64), q.end.astype(np.float64)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    ix, iy, iz = (rng.integers(0, q.n[k], 3000) for k in range(3))
    centres = (q.start + np.stack([ix, iy, iz], 1).astype(F) * q.cs).astype(F)
    faces = rng.uniform(lo, hi, (3000, 3)).astype(F)
    faces[np.arange(3000), rng.integers(0, 3, 3000)] = q.end[rng.integers(0, 3, 3000)]   # on an upper face (or beyond it)
    special = rng.uniform(lo, hi, (600, 3)).astype(F)
    special[0::3, 0] = np.inf
    special[1::3, 1] = -np.inf
    special[2::6, 2] = np.nan
    return {
        "box": rng.uniform(lo, hi, (20000, 3)).astype(F),
        "box1.5": rng.uniform(mid - 1.5 * half, mid + 1.5 * half, (20000, 3)).astype(F),
        "centres": centres,
        "faces": faces,
        "inf-nan": special,
    }


def _np(x):
    if hasattr(x, "cpu"):
        if x.dtype == getattr(torch, "uint32", None):
            x = x.view(torch.int32)
        x = x.cpu().numpy()
    return x


def _check(got, want, what):
    got = _np(got)
    assert gqm.same_bits(got, want), f"{what}: {int((got.view(np.uint32) != np.asarray(want, F).view(np.uint32)).sum())} values differ"


@pytest.mark.parametrize("name", ["suzanne-64", "blob-11k-128", "blob-100k-128"])
def test_sampling_is_bit_exact(grids, name):
    grid, d = grids[name]
    q = gqm.GridQ.of(grid)
    dh = d.cpu().numpy()
    for set_name, pts in _point_sets(q, 7).items():
        tp = torch.as_tensor(pts, device="cuda:0")
        for mode in MODES:
            for iso in (0.0, 0.05, -0.02):
                got, nrm = sample_grid(grid, d, tp, mode=mode, iso=iso, normals=True)
                _check(got, gqm.sample(q, dh, pts, mode, iso), f"{name} {set_name} {mode.name} iso {iso}")
                if iso == 0.05:
                    _check(nrm, gqm.normal(q, dh, pts, mode, iso), f"{name} {set_name} {mode.name} normals")
    # the outside value is a parameter
    pts = _point_sets(q, 8)["box1.5"]
    got = sample_grid(grid, d, torch.as_tensor(pts, device="cuda:0"), outside=-3.5)
    _check(got, gqm.sample(q, dh, pts, gqm.TRILINEAR, 0.0, -3.5), f"{name} outside -3.5")


def _camera(q, res=64, seed=0):
    lo, hi = q.start.astype(np.float64), q.end.astype(np.float64)
    c, ext = (lo + hi) / 2, (hi - lo).max()
    eye = c + np.array([0.3, 0.4, -1.6]) * ext
    fwd = (c - eye) / np.linalg.norm(c - eye)
    right = np.cross(fwd, [0, 1, 0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    u, v = np.meshgrid((np.arange(res) + 0.5) / res * 2 - 1, (np.arange(res) + 0.5) / res * 2 - 1)
    r = fwd + 0.45 * (u.reshape(-1, 1) * right + v.reshape(-1, 1) * up)
    r = (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(F)
    return np.tile(eye.astype(F), (res * res, 1)), r


def _ray_sets(q, seed):
    rng = np.random.default_rng(seed)
    lo, hi = q.start.astype(np.float64), q.end.astype(np.float64)
    o_cam, r_cam = _camera(q)
    inside = rng.uniform(lo, hi, (2000, 3)).astype(F)
    rin = rng.normal(size=(2000, 3))
    rin = (rin / np.linalg.norm(rin, axis=1, keepdims=True)).astype(F)
    axis = np.zeros((1200, 3), F)
    k = rng.integers(0, 3, 1200)
    axis[np.arange(1200), k] = np.where(rng.random(1200) < 0.5, 1, -1)
    oax = rng.uniform(lo, hi, (1200, 3)).astype(F)
    far = np.where(axis[np.arange(1200), k] > 0, lo[k] - 0.3 * (hi - lo)[k], hi[k] + 0.3 * (hi - lo)[k])
    oax[np.arange(1200), k] = far                                 # outside, entering along an axis
    oax[:300] = rng.uniform(lo, hi, (300, 3))                     # ... and from inside
    miss_o = rng.uniform(lo, hi, (500, 3)).astype(F)
    miss_o[:, 0] = hi[0] + 0.5 * (hi - lo)[0]                       # beside the box in x ...
    miss_r = rng.normal(size=(500, 3))
    miss_r[:, 0] = 0                                              # ... moving parallel to it: the line never meets the box
    miss_r = (miss_r / np.linalg.norm(miss_r, axis=1, keepdims=True)).astype(F)
    nan_o, nan_r = inside[:8].copy(), rin[:8].copy()
    nan_o[0::2, 1] = np.nan
    nan_r[1::2, 2] = np.nan
    return {"camera": (o_cam, r_cam), "inside": (inside, rin), "axis": (oax, axis), "miss": (miss_o, miss_r), "nan": (nan_o, nan_r)}


@pytest.mark.parametrize("name", ["suzanne-64", "blob-11k-128", "blob-100k-128"])
def test_raymarch_is_bit_exact(grids, name):
    grid, d = grids[name]
    q = gqm.GridQ.of(grid)
    dh = d.cpu().numpy()
    for set_name, (o, r) in _ray_sets(q, 3).items():
        to, tr = torch.as_tensor(o, device="cuda:0"), torch.as_tensor(r, device="cuda:0")
        for mode in MODES:
            for max_steps in (1, 100):
                iso = 0.02 if mode == SampleMode.Tetrahedral else 0.0
                pos, dist, steps, hit, nrm = raymarch_grid(grid, d, to, tr, mode=mode, iso=iso, max_steps=max_steps, normals=True)
                w_out, w_steps, w_hit, w_nrm = gqm.raymarch(q, dh, o, r, mode, iso, 100.0, max_steps, normals=True)
                what = f"{name} {set_name} {mode.name} max_steps {max_steps}"
                _check(torch.cat([pos, dist[:, None]], 1), w_out, what)
                assert np.array_equal(_np(steps).astype(np.uint32), w_steps), what
                assert np.array_equal(_np(hit), w_hit), what
                _check(nrm, w_nrm, what + " normals")
                if set_name == "camera" and max_steps == 100:
                    assert w_hit.mean() > 0.1, "the camera sees the mesh"
                if set_name == "miss":
                    assert not w_hit.any() and not w_steps.any()


def test_512_grid_million_points():
    v, idx = meshes.named("blob-100k")
    grid, d = _grid_sdf(v, idx, 512)
    q = gqm.GridQ.of(grid)
    rng = np.random.default_rng(11)
    pts = rng.uniform(q.start, q.end, (1_000_000, 3)).astype(F)
    got, nrm = sample_grid(grid, d, torch.as_tensor(pts, device="cuda:0"), normals=True)
    dh = d.cpu().numpy()
    sub = rng.choice(pts.shape[0], 50_000, replace=False)
    _check(_np(got)[sub], gqm.sample(q, dh, pts[sub]), "512^3 values")
    _check(_np(nrm)[sub], gqm.normal(q, dh, pts[sub]), "512^3 normals")


class _Affine:
    """The distances of the large test grid, d = x + y / 2 + z / 4 (exact in f32), computed from cell offsets."""

    def __init__(self, n):
        self.n = n

    def __getitem__(self, off):
        off = np.asarray(off, np.int64)
        nx, ny, nz = self.n
        x, y, z = off // (ny * nz), (off // nz) % ny, off % nz
        return (x + y / 2 + z / 4).astype(F)


def test_large_grid_64_bit_offsets():
    # 1040 x 1024 x 1024 cells (> 2^30, 4.2 GB): the far corner's byte offsets exceed 2^32
    n = (1040, 1024, 1024)
    grid = Grid([0.5, 0.5, 0.5], [1, 1, 1], n)
    xs = torch.arange(n[0], dtype=torch.float32, device="cuda:0").view(-1, 1, 1)
    ys = torch.arange(n[1], dtype=torch.float32, device="cuda:0").view(1, -1, 1) * 0.5
    zs = torch.arange(n[2], dtype=torch.float32, device="cuda:0").view(1, 1, -1) * 0.25
    d = (xs + ys + zs).reshape(-1)
    assert float(d[-1]) == 1039 + 1023 / 2 + 1023 / 4
    q = gqm.GridQ.of(grid)
    rng = np.random.default_rng(12)
    pts = (q.end - rng.uniform(0, 40, (20000, 3))).astype(F)
    pts[:100] = q.end
    model = _Affine(n)
    for mode in MODES:
        got, nrm = sample_grid(grid, d, torch.as_tensor(pts, device="cuda:0"), mode=mode, iso=0.05, normals=True)
        _check(got, gqm.sample(q, model, pts, mode, 0.05), f"large grid {mode.name}")
        _check(nrm, gqm.normal(q, model, pts, mode, 0.05), f"large grid {mode.name} normals")
    o = (q.end + F(3)).astype(F)[None].repeat(500, 0)
    r = -np.abs(rng.normal(size=(500, 3))) - 0.1
    r = (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(F)
    pos, dist, steps, hit = raymarch_grid(grid, d, torch.as_tensor(o, device="cuda:0"), torch.as_tensor(r, device="cuda:0"), iso=1790.0,
                                          max_steps=20)
    w_out, w_steps, _ = gqm.raymarch(q, model, o, r, gqm.TRILINEAR, 1790.0, 100.0, 20)
    _check(torch.cat([pos, dist[:, None]], 1), w_out, "large grid rays")
    assert np.array_equal(_np(steps).astype(np.uint32), w_steps)
    del d


def test_host_device_and_torch_memory_agree(grids):
    grid, d = grids["blob-11k-128"]
    q = gqm.GridQ.of(grid)
    dh = d.cpu().numpy()
    pts = _point_sets(q, 21)["box1.5"]
    o, r = _ray_sets(q, 22)["camera"]
    t = M2STimings()
    v_host, n_host = sample_grid(grid, dh, pts, mode=SampleMode.Tetrahedral, normals=True, timings=t)
    assert t.n_units == pts.shape[0] and t.distance_ms > 0
    v_dev, n_dev = sample_grid(grid, d, torch.as_tensor(pts, device="cuda:0"), mode=SampleMode.Tetrahedral, normals=True)
    _check(v_dev, v_host, "values host vs torch")
    _check(n_dev, n_host, "normals host vs torch")
    _check(v_host, gqm.sample(q, dh, pts, gqm.TETRAHEDRAL), "values host vs model")
    rh = raymarch_grid(grid, dh, o, r, normals=True)
    rd = raymarch_grid(grid, d, torch.as_tensor(o, device="cuda:0"), torch.as_tensor(r, device="cuda:0"), normals=True)
    for a, b in zip(rh, rd):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(_np(b).astype(np.asarray(a).dtype))
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # raw device pointers through the C ABI, asynchronous, on a caller stream
    L = _lib.lib()
    tp = torch.as_tensor(pts, device="cuda:0")
    out = torch.empty(pts.shape[0], dtype=torch.float32, device="cuda:0")
    s = torch.cuda.Stream()
    o_ = _lib.M2SOpts()
    o_.struct_size = C.sizeof(o_)
    o_.device = 0
    o_.mem_kind = _lib.MEM_DEVICE
    o_.stream = s.cuda_stream
    o_.stream_mode = 1
    o_.synchronous = 0
    so = _lib.M2SSampleOpts()
    so.struct_size, so.mode, so.iso, so.outside, so.max_steps = C.sizeof(so), 2, 0.0, 100.0, 100
    torch.cuda.synchronize()
    rc = L.m2s_sample_grid(C.byref(grid._g), d.data_ptr(), tp.data_ptr(), pts.shape[0], C.byref(so), out.data_ptr(), None, C.byref(o_))
    assert rc == 0, _lib.last_error()
    s.synchronize()
    _check(out, v_host, "asynchronous call on a caller stream")


def test_c_and_cpp_programs(tmp_path):
    common = ["-L", os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
              "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib"]
    for cc, std, src in [("gcc", "-std=c99", "tests/c/grid_query_smoke.c"), ("g++", "-std=c++17", "tests/cpp/grid_query_tests.cpp")]:
        exe = str(tmp_path / os.path.basename(src).split(".")[0])
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src)] + common
                              + (["-lm"] if cc == "gcc" else []) + ["-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
