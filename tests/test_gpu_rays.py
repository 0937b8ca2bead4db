"""Ray casting on the MI355X (include/m2s.h m2s_cast_rays, m2s_mesh_cast_rays) against the numpy model of the contract (tests/ray_model.py):
the tree walk, the all-pairs form and the model agree bit for bit in every output.  Run with `-m gpu`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ray_model as rm
import mesh_to_sdf_amd
from mesh_to_sdf_amd import Grid, M2STimings, Mesh, RayHits, Topology, _lib, cast_rays, count_intersections, meshes

occluded_rays = mesh_to_sdf_amd.test_occlusions   # (under a name pytest does not collect)

F = np.float32
INF = float("inf")
pytestmark = pytest.mark.gpu
RANGE = (0.9, 1.6)   # cuts hits off at both ends on every ray set below (asserted in the fixture)


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def bits(x):
    a = np.ascontiguousarray(_np(x))
    return a.view(np.uint32) if a.dtype == F else a


def _rays(v, idx, seed, n_radial, n_box, n_inside, n_axis):
    """One ray set of a mesh: radial vertex / edge-midpoint rays, random rays in 1.8 x the box (|d| != 1, and a scaled copy of some of
    them), origins inside, axis-parallel rays with exact zeros."""
    parts = [rm.radial_rays(v, idx, n_radial), rm.box_rays(v, n_box, seed), rm.inside_rays(v, n_inside, seed + 1), rm.axis_rays(v, n_axis, seed + 2)]
    o, d = parts[1]
    k = max(n_box // 4, 1)
    parts.append((o[:k], (d[:k] * F(37.5)).astype(F)))
    parts.append((o[k:2 * k], (d[k:2 * k] * F(1.0e-3)).astype(F)))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


@pytest.fixture(scope="module")
def cases(suzanne):
    """name -> (vertices, indices, origins, directions, model over [0, inf], model over RANGE or None).  Computed once."""
    out = {}
    far = np.array([1.0e4, -1.0e4, 1.0e4], F)   # the leaf boxes' 1e-4 padding is below an ulp (9.8e-4) there
    b12 = meshes.blob(12, 9)
    meshes_ = {"cube": (meshes.cube(), (0, 1500, 500, 900), True), "suzanne": (suzanne, (2000, 1500, 300, 400), True),
               "blob-192": (b12, (4000, 2000, 500, 500), True), "blob-6144": (meshes.blob(48, 65), (4000, 800, 300, 300), False),
               "blob-192-far": (((b12[0] + far).astype(F), b12[1]), (4000, 2000, 500, 500), False)}
    for seed, (name, ((v, idx), sizes, ranged)) in enumerate(meshes_.items()):
        n_radial = sizes[0]
        if name == "cube":   # radial rays at a cube's corners and edge midpoints, all of them
            n_radial = 64
        o, d = _rays(v, idx, 100 * seed, n_radial, *sizes[1:])
        assert o.shape[0] <= 6000
        tris = rm.triangles_of(v, idx)
        full = rm.cast(tris, o, d)
        cut = rm.cast(tris, o, d, *RANGE) if ranged else None
        if ranged:   # the range drops first hits (t < t_min) and later ones (t > t_max)
            assert ((full["t"] < RANGE[0]) & (cut["t"] > full["t"])).any() and (cut["count"] < full["count"]).any()
            assert ((full["count"] > cut["count"]) & (cut["t"] == full["t"])).any()
        out[name] = (v, idx, o, d, full, cut)
    return out


def _all_outputs(call, *args, **kw):
    """The three public calls -> the five outputs, as numpy."""
    h = call["hits"](*args, **kw)
    assert isinstance(h, RayHits)
    return {"t": _np(h.t), "triangle": _np(h.triangle), "uv": _np(h.uv), "count": _np(call["count"](*args, **kw)),
            "occluded": _np(call["occluded"](*args, **kw)).astype(np.uint8)}


def _same(got, want, what):
    for k in ("t", "triangle", "uv", "count", "occluded"):
        g, w = bits(got[k]), bits(np.asarray(want[k]))
        bad = np.flatnonzero((g != w).reshape(g.shape[0], -1).any(1))
        assert bad.size == 0, f"{what}: {k} differs on {bad.size} rays, first {bad[:5]}: got {got[k][bad[:3]]}, want {want[k][bad[:3]]}"


ONE_SHOT = {"hits": cast_rays, "count": count_intersections, "occluded": occluded_rays}


def _mesh_calls(m):
    return {"hits": m.cast_rays, "count": m.count_intersections, "occluded": m.test_occlusions}


def _raw(lib_call, o, d, n_out, t_min=0.0, t_max=INF, algorithm=0, which=(1, 1, 1, 1, 1)):
    """All five outputs from ONE call of the C entry point (host memory): lib_call(origins, directions, n, ropts, 5 outputs, opts)."""
    t, tri, uv = np.full(n_out, -1, F), np.full(n_out, 7, np.uint32), np.full((n_out, 2), -1, F)
    cnt, occ = np.full(n_out, 7, np.uint32), np.full(n_out, 7, np.uint8)
    ro = _lib.M2SRayOpts(C.sizeof(_lib.M2SRayOpts), t_min, t_max)
    op = _lib.M2SOpts()
    op.struct_size, op.device, op.synchronous, op.algorithm = C.sizeof(_lib.M2SOpts), -1, 1, algorithm
    ptrs = [x.ctypes.data if w else None for x, w in zip((t, tri, uv, cnt, occ), which)]
    rc = lib_call(o.ctypes.data, d.ctypes.data, o.shape[0], C.byref(ro), *ptrs, C.byref(op))
    assert rc == _lib.M2S_OK, _lib.last_error()
    return {"t": t, "triangle": tri, "uv": uv, "count": cnt, "occluded": occ}


# ---- 1. walk == all pairs == model, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "suzanne", "blob-192", "blob-6144", "blob-192-far"])
def test_walk_all_pairs_and_model_agree_bit_for_bit(cases, name):
    v, idx, o, d, full, cut = cases[name]
    topo = Topology.TriangleList(idx)
    for algorithm in (0, 1):
        _same(_all_outputs(ONE_SHOT, v, topo, o, d, algorithm=algorithm), full, f"{name} one-shot algorithm {algorithm}")
        if cut is not None:
            _same(_all_outputs(ONE_SHOT, v, topo, o, d, *RANGE, algorithm=algorithm), cut, f"{name} one-shot range algorithm {algorithm}")
    with Mesh(v, topo) as m:
        for algorithm in (0, 1):
            _same(_all_outputs(_mesh_calls(m), o, d, algorithm=algorithm), full, f"{name} Mesh algorithm {algorithm}")
        if cut is not None:
            _same(_all_outputs(_mesh_calls(m), o, d, *RANGE), cut, f"{name} Mesh range")
        # every output from one call (the walk then prunes nothing: the count needs every hit)
        L = _lib.lib()
        _same(_raw(lambda *r: L.m2s_mesh_cast_rays(m._h, *r), o, d, o.shape[0]), full, f"{name} Mesh, one call")


def test_mesh_whose_leaves_another_call_re_marked(cases):
    """The walk takes the tree as it is marked: after grid calls of two density classes (leaves of 2, and collapsed leaves) a Mesh returns
    the same bits, and the ray calls in between re-mark nothing."""
    v, idx, o, d, full, _ = cases["blob-6144"]
    L = _lib.lib()
    L.m2s_debug_leaf_sizes.restype = C.c_int
    lo, hi = meshes.extended_bbox(v, 0.1)
    sizes = {}
    for n in (128, 16):
        g = Grid.from_bounding_box(lo, hi, [n, n, n])
        out3 = (C.c_uint32 * 3)()
        assert L.m2s_debug_leaf_sizes(C.byref(g._g), C.c_size_t(idx.size // 3), C.c_size_t(0), out3) == 0
        sizes[n] = out3[0]
    assert sizes[128] == 2 and sizes[16] > 2, sizes
    with Mesh(v, Topology.TriangleList(idx)) as m:
        for n in (16, 128, 16):
            want = m.generate_grid_sdf(Grid.from_bounding_box(lo, hi, [n, n, n]))
            _same(_all_outputs(_mesh_calls(m), o, d), full, f"after a {n}^3 grid call (leaves of {sizes[n]})")
            again = m.generate_grid_sdf(Grid.from_bounding_box(lo, hi, [n, n, n]))
            assert np.array_equal(bits(want), bits(again))


# ---- 2. watertight on the device ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blob-192", "blob-6144"])
def test_radial_rays_all_hit_in_front(cases, name):
    v, idx, o, d, _, _ = cases[name]
    n = rm.radial_rays(v, idx, 4000)[0].shape[0]   # the set's leading rays: 386 (every vertex and edge midpoint) and 4000
    assert n in (386, 4000)
    for algorithm in (0, 1):
        h = cast_rays(v, Topology.TriangleList(idx), o[:n], d[:n], algorithm=algorithm)
        print(f"{name} algorithm {algorithm}: misses {int(np.isinf(h.t).sum())}, largest first t {h.t.max():.7f}")
        assert np.isfinite(h.t).all() and h.t.max() <= 1.001 and (h.triangle < idx.size // 3).all()


# ---- 3. the outputs agree with each other -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "suzanne", "blob-192", "blob-6144", "blob-192-far"])
def test_occluded_is_t_finite_is_count_positive(cases, name):
    v, idx, o, d, full, cut = cases[name]
    L = _lib.lib()
    with Mesh(v, Topology.TriangleList(idx)) as m:
        call = lambda *r: L.m2s_mesh_cast_rays(m._h, *r)   # noqa: E731
        for rng, want in (((0.0, INF), full), (RANGE, cut)):
            if want is None:
                continue
            r = _raw(call, o, d, o.shape[0], *rng)
            assert np.array_equal(r["occluded"] == 1, r["t"] < np.inf) and np.array_equal(r["occluded"] == 1, r["count"] > 0)
            assert np.array_equal(r["triangle"] != rm.NONE, r["occluded"] == 1) and np.array_equal(np.isnan(r["uv"]).any(1), r["occluded"] == 0)
            for algorithm in (0, 1):   # occluded alone: the walk stops at the first hit it meets
                only = _raw(call, o, d, o.shape[0], *rng, algorithm=algorithm, which=(0, 0, 0, 0, 1))
                assert np.array_equal(only["occluded"], want["occluded"])
                assert (only["t"] == -1).all() and (only["count"] == 7).all()   # outputs not asked for are not written
            first = _raw(call, o, d, o.shape[0], *rng, which=(1, 1, 1, 0, 0))   # first hit alone: the walk prunes against the best t
            for k in ("t", "triangle", "uv"):
                assert np.array_equal(bits(first[k]), bits(want[k])), k


# ---- 4. edge cases ------------------------------------------------------------------------------------------------------------------------
def test_bad_rays_hit_nothing_and_disturb_no_neighbour(cases):
    v, idx, o, d, full, _ = cases["blob-192"]
    o2, d2 = o.copy(), d.copy()
    rows = [3, 64, 65, 700, 1999]
    d2[3] = 0
    d2[64, 1] = np.nan
    o2[65, 2] = np.inf
    d2[700] = [np.inf, 0, 0]
    o2[1999] = np.nan
    ok = np.ones(o.shape[0], bool)
    ok[rows] = False
    for algorithm in (0, 1):
        got = _all_outputs(ONE_SHOT, v, Topology.TriangleList(idx), o2, d2, algorithm=algorithm)
        assert np.isinf(got["t"][rows]).all() and (got["triangle"][rows] == rm.NONE).all() and np.isnan(got["uv"][rows]).all()
        assert (got["count"][rows] == 0).all() and (got["occluded"][rows] == 0).all()
        _same({k: x[ok] for k, x in got.items()}, {k: x[ok] for k, x in full.items()}, f"good rays, algorithm {algorithm}")


def test_empty_mesh_and_no_rays(cases):
    import torch

    v, idx, o, d, _, _ = cases["cube"]
    none = Topology.TriangleList(np.zeros(0, np.uint32))
    for call in (ONE_SHOT, ):
        got = _all_outputs(call, np.zeros((4, 3), F), none, o[:70], d[:70])
        assert np.isinf(got["t"]).all() and (got["triangle"] == rm.NONE).all() and np.isnan(got["uv"]).all()
        assert (got["count"] == 0).all() and (got["occluded"] == 0).all()
    dev = cast_rays(torch.zeros((4, 3), device="cuda"), Topology.TriangleList(torch.zeros(0, dtype=torch.int64, device="cuda")),
                    torch.as_tensor(o[:70], device="cuda"), torch.as_tensor(d[:70], device="cuda"))
    assert dev.t.is_cuda and np.isinf(_np(dev.t)).all() and (_np(dev.triangle) == rm.NONE).all()
    with Mesh(np.zeros((2, 3), F), Topology.TriangleList()) as m:
        assert m.triangle_count() == 0
        assert (m.count_intersections(o[:70], d[:70]) == 0).all() and not m.test_occlusions(o[:70], d[:70], algorithm=1).any()
    h = cast_rays(v, Topology.TriangleList(idx), np.zeros((0, 3), F), np.zeros((0, 3), F))
    assert h.t.shape == (0,) and h.triangle.shape == (0,) and h.uv.shape == (0, 2)
    with Mesh(v, Topology.TriangleList(idx)) as m:
        assert m.count_intersections(np.zeros((0, 3), F), np.zeros((0, 3), F)).shape == (0,)


def test_host_and_device_memory_and_timings(cases):
    import torch

    v, idx, o, d, full, cut = cases["suzanne"]
    t = M2STimings()
    host = cast_rays(v, Topology.TriangleList(idx), o, d, timings=t)
    assert t.n_units == o.shape[0] and t.n_triangles == idx.size // 3 and t.distance_ms > 0 and t.accel_build_ms > 0
    assert t.total_ms >= t.distance_ms and t.distance_launches == 1
    dv, di, do, dd = (torch.as_tensor(x, device="cuda") for x in (v, idx.astype(np.int64), o, d))
    dev_calls = _all_outputs(ONE_SHOT, dv, Topology.TriangleList(di), do, dd, *RANGE)
    _same(dev_calls, cut, "device memory, one-shot")
    dev = cast_rays(dv, Topology.TriangleList(di), do, dd)
    assert dev.t.is_cuda and dev.triangle.is_cuda and dev.uv.is_cuda and dev.uv.shape == (o.shape[0], 2)
    assert np.array_equal(bits(dev.t), bits(host.t)) and np.array_equal(_np(dev.triangle), host.triangle) and np.array_equal(bits(dev.uv), bits(host.uv))
    occ = occluded_rays(dv, Topology.TriangleList(di), do, dd)
    assert occ.is_cuda and occ.dtype == torch.bool and np.array_equal(_np(occ), full["occluded"] == 1)
    with Mesh(dv, Topology.TriangleList(di)) as m:
        _same(_all_outputs(_mesh_calls(m), do, dd), full, "device memory, Mesh")
        _same(_all_outputs(_mesh_calls(m), o, d), full, "device Mesh, host rays")


def test_asynchronous_calls_and_drain(cases):
    import torch

    v, idx, o, d, full, cut = cases["blob-192"]
    dv, di, do, dd = (torch.as_tensor(x, device="cuda") for x in (v, idx.astype(np.int64), o, d))
    with Mesh(dv, Topology.TriangleList(di)) as m:
        m.cast_rays(do, dd)
        m.drain_timings()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            h = m.cast_rays(do, dd, synchronous=False)
            n = m.count_intersections(do, dd, *RANGE, synchronous=False)
            occ = m.test_occlusions(do, dd, synchronous=False)
        t = m.drain_timings()
        assert t.n_units == 3 * o.shape[0] and t.distance_launches == 3 and t.distance_ms > 0
        assert np.array_equal(bits(h.t), bits(full["t"])) and np.array_equal(_np(h.triangle), full["triangle"])
        assert np.array_equal(bits(h.uv), bits(full["uv"]))
        assert np.array_equal(_np(n), cut["count"]) and np.array_equal(_np(occ), full["occluded"] == 1)


def test_strips_and_u16_indices(cases):
    """A list's indices read as a strip give triangles strung along the blob's meridians, and the radial rays lie in those meridian
    planes: edge-on triangles, whose edge functions are rounding noise.  The definition's bounding clauses decide those (the bare test
    would report hits far from such triangles, asserted here), and walk, all pairs and model agree bit for bit on them too."""
    v, idx = meshes.blob(16, 17)
    o, d = _rays(v, idx, 900, 300, 500, 100, 100)
    i16 = idx.astype(np.uint16)
    for topology, topo in ((0, Topology.TriangleList(i16)), (1, Topology.TriangleStrip(i16)), (1, Topology.TriangleStrip(idx))):
        tris = rm.triangles_of(v, idx, topology)
        want = rm.cast(tris, o, d)
        if topology == 1:
            assert (rm.cast(tris, o, d, bare=True)["count"] > want["count"]).any()   # the clauses are at work on this set
        for algorithm in (0, 1):
            _same(_all_outputs(ONE_SHOT, v, topo, o, d, algorithm=algorithm), want, f"topology {topology} algorithm {algorithm}")
    strip = v[idx.astype(np.int64)[:300]]   # no indices: the vertices themselves as a strip (degenerate triangles among them)
    want = rm.cast(rm.triangles_of(strip, None, 1), o, d)
    for algorithm in (0, 1):
        _same(_all_outputs(ONE_SHOT, strip, Topology.TriangleStrip(), o, d, algorithm=algorithm), want, f"strip without indices, algorithm {algorithm}")
    # the same tree marked with collapsed leaves: the boxes differ, the bits do not
    lo, hi = meshes.extended_bbox(v, 0.1)
    with Mesh(v, Topology.TriangleStrip(idx)) as m:
        want = rm.cast(rm.triangles_of(v, idx, 1), o, d)
        for n in (16, 128):
            m.generate_grid_sdf(Grid.from_bounding_box(lo, hi, [n, n, n]))
            _same(_all_outputs(_mesh_calls(m), o, d), want, f"strip Mesh after a {n}^3 grid call")


# ---- 5. consumers ---------------------------------------------------------------------------------------------------------------------------
def test_c_and_cpp_programs_run(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["-L", os.path.join(root, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
              "-Wl,-rpath," + os.path.join(root, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib"]
    for cc, std, src in [("gcc", "-std=c99", "tests/c/rays_smoke.c"), ("g++", "-std=c++17", "tests/cpp/rays_tests.cpp")]:
        exe = str(tmp_path / os.path.basename(src).split(".")[0])
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(root, "include"), os.path.join(root, src)] + common
                              + (["-lm"] if cc == "gcc" else []) + ["-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
