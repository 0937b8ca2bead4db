"""Surface sampling on the MI355X (include/m2s.h m2s_sample_surface, m2s_mesh_sample_surface) against the numpy model of the contract
(tests/sample_model.py): every output bit for bit, in every form of the call.  Run with `-m gpu`.

The library's topologies are the reference's two, list and strip (there is no fan), so those two, with and without indices, are what the
topology test covers."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import sample_model as sm
from mesh_to_sdf_amd import (AccelerationMethod, Grid, M2STimings, Mesh, SignMethod, SurfaceSamples, Topology, cast_rays, meshes, sample_sdf_near_surface,
                             sample_surface, surface_area)

F = np.float32
pytestmark = pytest.mark.gpu
N = 100_000
DEV = "cuda:0"


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def bits(x):
    a = np.ascontiguousarray(_np(x))
    return a.view(np.uint32) if a.dtype == F else a


def _same(got: SurfaceSamples, want, what, n=None, first=0):
    """All five outputs of `got` against rows [first, first + n) of the model's."""
    assert isinstance(got, SurfaceSamples)
    n = _np(got.points).shape[0] if n is None else n
    assert got.area == want["area"], f"{what}: area {got.area!r} != {want['area']!r}"
    for k, g in (("point", got.points), ("triangle", got.triangle), ("uv", got.uv), ("normal", got.normal)):
        if g is None:
            continue
        g, w = bits(g), bits(want[k][first:first + n])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(n, -1).any(1)) if n else np.zeros(0, np.int64)
        assert bad.size == 0, f"{what}: {k} differs on {bad.size} of {n} samples, first {bad[:5]}: got {_np(g)[bad[:3]]}, want {w[bad[:3]]}"


def _dev(v, idx):
    return torch.as_tensor(v, device=DEV), (None if idx is None else torch.as_tensor(idx.astype(np.int64), device=DEV))


@pytest.fixture(scope="module")
def cases(suzanne):
    """name -> (vertices, indices, model of samples 0 .. N-1 under seed 0).  Computed once; smaller calls are rows of it."""
    b12 = meshes.blob(12, 9)
    far = np.array([1.0e4, -1.0e4, 1.0e4], F)
    all_ = {"cube": meshes.cube(), "suzanne": suzanne, "blob-192": b12, "blob-6144": meshes.blob(48, 65),
            "blob-192-far": ((b12[0] + far).astype(F), b12[1]),
            "degenerates": sm.with_degenerates(*b12), "one-huge": sm.one_huge(*b12),
            "blob-100k": meshes.named("blob-100k"),           # 25 scan tiles of 4096 triangles, the last one short
            "one-triangle": (np.array([[0, 0, 0], [2, 0, 0], [0, 3, 1]], F), np.array([0, 1, 2], np.uint32))}
    out = {}
    for name, (v, idx) in all_.items():
        v, idx = np.ascontiguousarray(v, F), np.ascontiguousarray(idx, np.uint32)
        out[name] = (v, idx, sm.sample(sm.triangles_of(v, idx), N, seed=0))
    n100k = out["blob-100k"][1].size // 3
    assert n100k > 2 * 4096 and n100k % 4096 != 0
    return out


MESHES = ["cube", "suzanne", "blob-192", "blob-6144", "blob-192-far", "degenerates", "one-huge", "blob-100k", "one-triangle"]


# ---- 1. the one-shot call ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_one_shot_matches_the_model(cases, name):
    v, idx, want = cases[name]
    _same(sample_surface(v, Topology.TriangleList(idx), N, normals=True), want, f"{name}, host memory")
    dv, di = _dev(v, idx)
    _same(sample_surface(dv, Topology.TriangleList(di), N, normals=True), want, f"{name}, device memory")
    assert surface_area(v, Topology.TriangleList(idx)) == want["area"] == surface_area(dv, Topology.TriangleList(di))


def test_triangles_without_area_are_present_and_never_sampled(cases):
    v, idx, want = cases["degenerates"]
    A, n = sm.tri_area2(sm.triangles_of(v, idx))
    raw = np.sqrt((n.astype(np.float64) ** 2).sum(1))
    assert (A == 0).sum() >= 16 and np.isnan(raw).any() and np.isinf(n).any() and (raw[A == 0] == 0).any()
    got = sample_surface(v, Topology.TriangleList(idx), N)
    assert (A[got.triangle] > 0).all() and np.isfinite(got.points).all()
    assert got.area == sm.table(sm.triangles_of(*cases["blob-192"][:2]))[3]       # they add nothing to the area either


def test_one_huge_triangle_takes_its_share(cases):
    v, idx, want = cases["one-huge"]
    A, _ = sm.tri_area2(sm.triangles_of(v, idx))
    assert A[-1] / np.delete(A, -1).mean() > 0.9e6
    got = sample_surface(v, Topology.TriangleList(idx), N)
    rest = int((got.triangle != A.size - 1).sum())
    assert 0 < rest < 100 and rest == int((want["triangle"] != A.size - 1).sum())   # 192 / 1e6 of 100 000 samples: about 19


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_sample_counts(cases, n):
    v, idx, want = cases["suzanne"]
    dv, di = _dev(v, idx)
    for what, call in (("host", lambda: sample_surface(v, Topology.TriangleList(idx), n, normals=True)),
                       ("device", lambda: sample_surface(dv, Topology.TriangleList(di), n, normals=True))):
        got = call()
        assert _np(got.points).shape == (n, 3) and _np(got.triangle).shape == (n,) and _np(got.uv).shape == (n, 2)
        _same(got, want, f"{what}, {n} samples", n)


@pytest.mark.parametrize("seed", [0, 2 ** 32 + 7])
@pytest.mark.parametrize("first", [0, 2 ** 32 - 10, 2 ** 40])
def test_seeds_and_offsets(cases, seed, first):
    """first = 2^32 - 10: the counter's low word wraps inside the call."""
    v, idx, _ = cases["blob-6144"]
    want = sm.sample(sm.triangles_of(v, idx), 1000, seed=seed, first_sample=first)
    _same(sample_surface(v, Topology.TriangleList(idx), 1000, seed=seed, first_sample=first, normals=True), want, "host")
    dv, di = _dev(v, idx)
    _same(sample_surface(dv, Topology.TriangleList(di), 1000, seed=seed, first_sample=first, normals=True), want, "device")
    with Mesh(dv, Topology.TriangleList(di)) as m:
        _same(m.sample_surface(1000, seed=seed, first_sample=first, normals=True), want, "Mesh")


def test_index_widths_and_topologies(cases):
    v, idx, _ = cases["blob-192"]
    n = 3000
    want = sm.sample(sm.triangles_of(v, idx), n, seed=5)
    _same(sample_surface(v, Topology.TriangleList(idx.astype(np.uint16)), n, seed=5, normals=True), want, "u16 list")
    _same(sample_surface(v, Topology.TriangleList(idx.astype(np.uint32)), n, seed=5, normals=True), want, "u32 list")
    flat = np.ascontiguousarray(v[idx.astype(np.int64)])                              # no indices: the vertices themselves
    _same(sample_surface(flat, Topology.TriangleList(), n, seed=5, normals=True), want, "list without indices")
    want = sm.sample(sm.triangles_of(flat[:301], None, 0), n, seed=5)                 # a trailing partial triple is dropped
    _same(sample_surface(flat[:301], Topology.TriangleList(), n, seed=5, normals=True), want, "list with a partial triple")
    for ib in (np.uint16, np.uint32):
        want = sm.sample(sm.triangles_of(v, idx, 1), n, seed=5)                       # the index list read as a strip: degenerate windows among them
        _same(sample_surface(v, Topology.TriangleStrip(idx.astype(ib)), n, seed=5, normals=True), want, f"strip {ib.__name__}")
        dv, di = _dev(v, idx)
        _same(sample_surface(dv, Topology.TriangleStrip(di), n, seed=5, normals=True), want, "strip, device memory")
    want = sm.sample(sm.triangles_of(flat[:300], None, 1), n, seed=5)
    _same(sample_surface(flat[:300], Topology.TriangleStrip(), n, seed=5, normals=True), want, "strip without indices")


# ---- 2. the persistent mesh, algorithm 1, and what the contract implies -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "suzanne", "degenerates", "blob-100k", "one-triangle"])
@pytest.mark.parametrize("device", [False, True])
def test_mesh_form_matches_before_and_after_a_grid_call(cases, name, device):
    v, idx, want = cases[name]
    lo, hi = meshes.extended_bbox(cases["blob-192"][0] if name == "degenerates" else v, 0.1)
    a, b = _dev(v, idx) if device else (v, idx)
    with Mesh(a, Topology.TriangleList(b)) as m:
        assert m.surface_area() == want["area"]
        _same(m.sample_surface(N, normals=True), want, f"{name}: Mesh")
        if name != "degenerates":                                                  # (a NaN vertex has no place in a distance grid)
            m.generate_grid_sdf(Grid.from_bounding_box(lo, hi, [24, 24, 24]))      # re-marks the tree's leaves
        _same(m.sample_surface(N, normals=True), want, f"{name}: Mesh after a grid call")
        _same(m.sample_surface(4000, normals=True, algorithm=1), want, f"{name}: Mesh, algorithm 1", 4000)
    _same(sample_surface(a, Topology.TriangleList(b), 4000, normals=True, algorithm=1), want, f"{name}: one shot, algorithm 1", 4000)


def test_two_half_calls_equal_one_whole_call(cases):
    v, idx, want = cases["blob-6144"]
    k = 33_333
    topo = Topology.TriangleList(idx)
    _same(sample_surface(v, topo, k, normals=True), want, "[0, k)", k)
    _same(sample_surface(v, topo, N - k, first_sample=k, normals=True), want, "[k, n)", N - k, k)
    dv, di = _dev(v, idx)
    with Mesh(dv, Topology.TriangleList(di)) as m:
        _same(m.sample_surface(N - k, first_sample=k, normals=True), want, "Mesh [k, n)", N - k, k)


def test_points_only_and_asynchronous_calls(cases):
    v, idx, want = cases["suzanne"]
    dv, di = _dev(v, idx)
    with Mesh(dv, Topology.TriangleList(di)) as m:
        only = m.sample_surface(N, points_only=True)
        assert only.triangle is None and only.uv is None and only.normal is None
        _same(only, want, "points only")
        t = M2STimings()
        _same(m.sample_surface(N, normals=True, timings=t), want, "timed")
        assert t.n_units == N and t.n_triangles == idx.size // 3 and t.distance_ms > 0 and t.total_ms >= t.distance_ms
        a = m.sample_surface(N, normals=True, synchronous=False)
        b = m.sample_surface(5000, first_sample=N - 5000, synchronous=False)
        d = m.drain_timings()
        assert d.n_units == N + 5000 and d.distance_launches == 2 and d.distance_ms > 0
        _same(a, want, "asynchronous")
        _same(b, want, "asynchronous, offset", 5000, N - 5000)
    with Mesh(dv, Topology.TriangleList(di)) as m:          # the table made by an asynchronous first call
        a = m.sample_surface(N, normals=True, synchronous=False)
        assert m.drain_timings().n_units == N
        _same(a, want, "asynchronous first call")
    t = M2STimings()
    _same(sample_surface(dv, Topology.TriangleList(di), N, normals=True, timings=t), want, "one shot, timed")
    assert t.accel_build_ms < 0.05 and t.seed_ms > 0 and t.distance_ms > 0 and t.n_units == N


# ---- 3. ties to the rest of the library -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "suzanne", "blob-6144", "blob-192-far"])
def test_samples_lie_on_the_mesh(cases, name):
    """The point's arithmetic has four roundings per component, each at most an ulp of the coordinate scale: 1e-6 of the largest |coordinate|
    (16 ulp) bounds the distance back to the mesh."""
    v, idx, _ = cases[name]
    with Mesh(v, Topology.TriangleList(idx)) as m:
        s = m.sample_surface(20000, seed=11)
        tri, pts, dist = m.closest_points(s.points)
    assert dist.max() <= 1e-6 * np.abs(v).max(), dist.max()


def test_rays_back_along_the_normal_hit_the_sampled_triangle(cases):
    v, idx, _ = cases["cube"]
    s = sample_surface(v, Topology.TriangleList(idx), 20000, seed=12, normals=True)
    o = (s.points + F(0.25) * s.normal).astype(F)
    h = cast_rays(v, Topology.TriangleList(idx), o, -s.normal)
    assert np.isfinite(h.t).all() and np.abs(h.t - 0.25).max() < 1e-5
    same = h.triangle == s.triangle
    # otherwise a triangle that shares the hit point: the other half of the face, with the hit on the common diagonal
    tris = sm.triangles_of(v, idx)[h.triangle[~same]]
    hit = tris[:, 0] + h.uv[~same, :1] * (tris[:, 1] - tris[:, 0]) + h.uv[~same, 1:] * (tris[:, 2] - tris[:, 0])
    assert same.mean() > 0.99 and np.abs(hit - s.points[~same]).max(initial=0) < 1e-5
    assert (h.triangle[~same] // 2 == s.triangle[~same] // 2).all()


# ---- 4. training samples ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", ["winding", "raycast", "normal"])
@pytest.mark.parametrize("device", [False, True])
def test_sample_sdf_near_surface(cases, sign, device):
    v, idx, _ = cases["blob-6144"]
    a, b = _dev(v, idx) if device else (v, idx)
    n, frac = 20000, 0.05
    pts, sdf = sample_sdf_near_surface(a, Topology.TriangleList(b), n, uniform_fraction=frac, sign=sign, seed=21)
    if device:
        assert pts.device == a.device and sdf.device == a.device and pts.dtype == torch.float32
    else:
        assert isinstance(pts, np.ndarray) and isinstance(sdf, np.ndarray)
    assert tuple(pts.shape) == (n, 3) and tuple(sdf.shape) == (n,)
    again, sdf2 = sample_sdf_near_surface(a, Topology.TriangleList(b), n, uniform_fraction=frac, sign=sign, seed=21)
    assert np.array_equal(bits(again), bits(pts)) and np.array_equal(bits(sdf2), bits(sdf))       # the same seed, the same device
    other, _ = sample_sdf_near_surface(a, Topology.TriangleList(b), n, uniform_fraction=frac, sign=sign, seed=22)
    assert not np.array_equal(bits(other), bits(pts))
    with Mesh(a, Topology.TriangleList(b)) as m:
        if sign == "winding":
            want = m.generate_sdf_winding(pts)
        elif sign == "raycast":
            want = m.generate_sdf(pts, AccelerationMethod.RtreeBvh)
        else:
            want = m.generate_sdf(pts, AccelerationMethod.Bvh(SignMethod.Normal))
        assert np.array_equal(bits(want), bits(sdf))
        p2, s2 = m.sample_sdf_near_surface(n, uniform_fraction=frac, sign=sign, seed=21)
        assert np.array_equal(bits(p2), bits(pts)) and np.array_equal(bits(s2), bits(sdf))
        n_near = n - int(round(n * frac))
        surf = _np(m.sample_surface(n_near, seed=21).points)
    p, d = _np(pts), _np(sdf)
    # a displaced row is no farther from the mesh than from the surface sample it came from, which lies on the mesh up to the bound above
    moved = np.linalg.norm(p[:n_near].astype(np.float64) - surf.astype(np.float64), axis=1)
    assert (np.abs(d[:n_near]) <= moved * (1 + 1e-5) + 1e-6 * np.abs(v).max()).all()
    assert (d < 0).any() and (d > 0).any()
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    c, h = 0.5 * (lo + hi), 0.55 * (hi - lo)
    assert (p[n_near:] >= c - h - 1e-5).all() and (p[n_near:] <= c + h + 1e-5).all()
    sig = 0.5 * np.linalg.norm(hi - lo) * np.array([0.05, 0.0158])
    for k in (0, 1):     # equal shares: row i takes sigmas[i % 2]
        rms = np.sqrt((moved[k:n_near:2] ** 2).mean() / 3)
        assert abs(rms / sig[k] - 1) < 0.05, (k, rms, sig[k])


# ---- 5. consumers -----------------------------------------------------------------------------------------------------------------------------
def test_cpp_consumer_reproduces_the_first_samples(cases, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    v, idx, _ = cases["cube"]
    seed, n = 2 ** 32 + 7, 16
    want = sm.sample(sm.triangles_of(v, idx), n, seed=seed)
    exe = str(tmp_path / "sample_tests")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(root, "include"), os.path.join(root, "tests/cpp/sample_tests.cpp"),
                           "-L", os.path.join(root, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(root, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    hx = lambda f: "%08x" % struct.unpack("<I", struct.pack("<f", float(f)))[0]   # noqa: E731
    args = [str(seed), str(n), float(want["area"]).hex()]
    for i in range(n):
        args += [str(int(want["triangle"][i])), hx(want["uv"][i, 0]), hx(want["uv"][i, 1])] + [hx(x) for x in want["point"][i]]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
