"""Winding numbers on the MI355X (include/m2s.h m2s_winding_numbers & co.) against the f64 model of tests/winding_model.py: the exact forms
within f32 rounding, the Barnes-Hut walk within twice the model's own expansion error, the inside test, the signed distances, and bit
equality of every way of asking on one Mesh.  Run with `-m gpu`."""
import os
import subprocess

import numpy as np
import pytest

import winding_model as wm
from mesh_to_sdf_amd import (Grid, M2SPanic, M2STimings, Mesh, SignMethod, Topology, _lib, generate_grid_sdf, generate_grid_sdf_winding,
                             generate_sdf_winding, grid_closest_points, grid_winding_numbers, meshes, winding_numbers, closest_points)
from test_closest_cpu import grid_centres
from test_winding_cpu import BETAS, fixed_case

F = np.float32
INF = float("inf")
pytestmark = pytest.mark.gpu


def f32_term(n_tris):
    """Each of T f32 terms is at most 1/2 in magnitude and carries a few ulps of atan2f and of the running sum."""
    return n_tris * 2.0 ** -22 + 1e-6


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def bits(x):
    return np.ascontiguousarray(_np(x)).view(np.uint32)


@pytest.fixture(scope="module")
def cases():
    """closed / holed: (vertices, indices, points, triangles f64, exact w f64, {beta: E_model}) on the fixed mesh and point set."""
    out = {}
    for name, holed in (("closed", False), ("holed", True)):
        v, idx, q = fixed_case(holed)
        tris = wm.triangles_of(v, idx)
        err, w = wm.model_error(tris, q, BETAS + (_lib.WINDING_BETA_DEFAULT,))
        out[name] = (v, idx, q, tris, w, err)
    return out


# ---- accuracy --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(48, 65), (100, 101)])   # 6,144 and 20,000 triangles
def test_exact_forms_match_the_model(shape):
    v, idx = meshes.blob(*shape)
    lo, hi = meshes.extended_bbox(v, 0.4)
    q = meshes.uniform_queries(lo, hi, 1500)
    tris = wm.triangles_of(v, idx)
    want = wm.exact_winding(tris, q)
    tol = f32_term(tris.shape[0])
    for what, got in (("beta = inf", winding_numbers(v, Topology.TriangleList(idx), q, beta=INF)),
                      ("algorithm 1", winding_numbers(v, Topology.TriangleList(idx), q, algorithm=1))):
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"{shape} {what}: max |w - exact| = {err:.3e} (tolerance {tol:.3e})")
        assert err <= tol, what
    grid = Grid.from_bounding_box(lo, hi, [12, 10, 11])
    centres = grid_centres(grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count())
    gw = grid_winding_numbers(v, Topology.TriangleList(idx), grid, beta=INF)
    assert np.abs(gw.astype(np.float64) - wm.exact_winding(tris, centres)).max() <= tol


@pytest.mark.parametrize("name", ["closed", "holed"])
def test_expansion_error_within_twice_the_models(cases, name):
    """max |w_gpu - w_exact,f64| <= 2 E_model(beta) + the f32 term, for the default beta and every recorded one.  Measured ratios
    max |w_gpu - w_exact| / E_model(beta) are printed (DESIGN.md §4.9 quotes them)."""
    v, idx, q, tris, w, err = cases[name]
    for beta in sorted(err):
        got = winding_numbers(v, Topology.TriangleList(idx), q, beta=beta).astype(np.float64)
        e = np.abs(got - w).max()
        print(f"{name} beta {beta}: max |w_gpu - w_exact| = {e:.4e}, E_model = {err[beta]:.4e}, ratio {e / err[beta]:.3f}")
        assert e <= 2.0 * err[beta] + f32_term(tris.shape[0]), beta


@pytest.mark.parametrize("name", ["closed", "holed"])
def test_inside_outside_agrees_with_the_model(cases, name):
    v, idx, q, tris, w, _ = cases[name]
    got = winding_numbers(v, Topology.TriangleList(idx), q)
    decided = np.abs(w - 0.5) > 0.1
    left_out = 1.0 - decided.mean()
    print(f"{name}: {left_out:.4%} of the points lie within 0.1 of w = 1/2")
    assert left_out <= 0.01
    assert np.array_equal(got[decided] >= 0.5, w[decided] >= 0.5)


# ---- signed distances --------------------------------------------------------------------------------------------------------------
def test_signed_distances_closed_mesh(cases):
    v, idx, _, _, _, _ = cases["closed"]
    lo, hi = meshes.extended_bbox(v, 0.2)
    grid = Grid.from_bounding_box(lo, hi, [44, 40, 36])
    topo = Topology.TriangleList(idx)
    sdf = generate_grid_sdf_winding(v, topo, grid)
    ray = generate_grid_sdf(v, topo, grid, SignMethod.Raycast)
    _, _, dist = grid_closest_points(v, topo, grid)
    assert np.array_equal(bits(np.abs(sdf)), bits(dist))
    diag = float(np.linalg.norm(np.asarray(grid.get_cell_size(), np.float64)))
    far = np.abs(ray) > diag
    assert far.mean() > 0.5 and (ray[far] < 0).any()
    assert np.array_equal(sdf[far] < 0, ray[far] < 0)


def test_signed_distances_holed_mesh(cases):
    v, idx, _, tris, _, _ = cases["holed"]
    full = wm.triangles_of(*fixed_case(False)[:2])
    removed = full[full.mean(1)[:, 2] > 0.8].reshape(-1, 3)
    hole_diameter = float(np.linalg.norm(removed.max(0) - removed.min(0)))
    blo, bhi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    lo, hi = meshes.extended_bbox(v, 1.5)
    grid = Grid.from_bounding_box(lo, hi, [40, 40, 40])
    sdf = generate_grid_sdf_winding(v, Topology.TriangleList(idx), grid)
    _, _, dist = grid_closest_points(v, Topology.TriangleList(idx), grid)
    assert np.array_equal(bits(np.abs(sdf)), bits(dist))
    c = grid_centres(grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count()).astype(np.float64)
    outside_box = np.linalg.norm(np.maximum(np.maximum(blo - c, c - bhi), 0.0), axis=1)
    far = outside_box > hole_diameter
    assert far.sum() > 1000 and (sdf < 0).any()
    assert not (sdf[far] < 0).any()


# ---- consistency on one Mesh ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
def test_one_mesh_gives_the_same_bits_however_it_is_asked(cases, device):
    import torch

    v, idx, q, tris, w, err = cases["holed"]
    lo, hi = meshes.extended_bbox(v, 0.3)
    grid = Grid.from_bounding_box(lo, hi, [37, 29, 43])
    other = Grid.from_bounding_box(lo, hi, [90, 100, 80])
    centres = grid_centres(grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count())
    if device:
        mv, mi = torch.as_tensor(v, device="cuda"), torch.as_tensor(idx.astype(np.int64), device="cuda")
        pts = torch.as_tensor(centres, device="cuda")
    else:
        mv, mi, pts = v, idx, centres
    n = grid.get_total_cell_count()
    with Mesh(mv, Topology.TriangleList(mi)) as m:
        for beta in (_lib.WINDING_BETA_DEFAULT, 2.0, INF):
            g0 = _np(m.grid_winding_numbers(grid, beta=beta))
            assert np.array_equal(bits(m.winding_numbers(pts, beta=beta)), bits(g0)), ("points", beta)
            # x-slabs = the whole grid, and only the slab is written
            out = torch.full((n,), -9.0, device="cuda") if device else np.full(n, -9.0, F)
            m.grid_winding_numbers(grid, beta=beta, x_slab=(5, 18), out=out)
            row = 29 * 43
            assert (_np(out)[: 5 * row] == -9.0).all() and (_np(out)[18 * row:] == -9.0).all()
            m.grid_winding_numbers(grid, beta=beta, x_slab=(0, 5), out=out)
            m.grid_winding_numbers(grid, beta=beta, x_slab=(18, 37), out=out)
            assert np.array_equal(bits(out), bits(g0)), ("slabs", beta)
            # other calls in between re-mark the tree's leaves
            m.generate_grid_sdf(other, SignMethod.Raycast)
            m.grid_winding_numbers(other, beta=2.0)
            m.generate_sdf(pts[:5000])
            assert np.array_equal(bits(m.grid_winding_numbers(grid, beta=beta)), bits(g0)), ("repeat", beta)
            s = _np(m.generate_grid_sdf_winding(grid, beta=beta))
            assert np.array_equal(s < 0, g0 >= 0.5), ("sign", beta)
            assert np.array_equal(bits(np.abs(s)), bits(m.grid_closest_points(grid)[2])), ("magnitude", beta)
        w_mesh = _np(m.winding_numbers(q))
    # one-shot calls may build another tree: they agree within the accuracy contract
    b = _lib.WINDING_BETA_DEFAULT
    w_shot = winding_numbers(v, Topology.TriangleList(idx), q)
    assert np.abs(w_shot.astype(np.float64) - w_mesh).max() <= 2.0 * err[b] + f32_term(tris.shape[0])
    assert np.abs(w_mesh.astype(np.float64) - w).max() <= 2.0 * err[b] + f32_term(tris.shape[0])


def test_asynchronous_calls_and_drain(cases):
    import torch

    v, idx, q, _, _, _ = cases["closed"]
    dv, di, dq = (torch.as_tensor(x, device="cuda") for x in (v, idx.astype(np.int64), q))
    lo, hi = meshes.extended_bbox(v, 0.2)
    grid = Grid.from_bounding_box(lo, hi, [32, 32, 32])
    with Mesh(dv, Topology.TriangleList(di)) as m:
        want_q, want_g = _np(m.winding_numbers(dq)), _np(m.generate_grid_sdf_winding(grid))
        m.drain_timings()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            got_q = m.winding_numbers(dq, synchronous=False)
            got_g = m.generate_grid_sdf_winding(grid, synchronous=False)
        t = m.drain_timings()
        assert t.n_units == q.shape[0] + grid.get_total_cell_count() and t.distance_launches == 3 and t.distance_ms > 0
        assert np.array_equal(bits(got_q), bits(want_q)) and np.array_equal(bits(got_g), bits(want_g))


# ---- edge cases ------------------------------------------------------------------------------------------------------------------------
def test_empty_mesh():
    import torch

    q = np.ones((70, 3), F)
    w = winding_numbers(torch.zeros((4, 3), device="cuda"), Topology.TriangleList(torch.zeros(0, dtype=torch.int64, device="cuda")),
                        torch.as_tensor(q, device="cuda"))
    assert w.shape == (70,) and (_np(w) == 0).all()
    with Mesh(np.zeros((2, 3), F), Topology.TriangleList()) as m:
        assert m.triangle_count() == 0
        assert (m.winding_numbers(q) == 0).all()
        assert (m.grid_winding_numbers(Grid.from_bounding_box([0, 0, 0], [1, 1, 1], [3, 3, 3])) == 0).all()
        with pytest.raises(M2SPanic) as e:
            m.generate_sdf_winding(q)
        assert e.value.code == _lib.ERR_EMPTY_MESH


def test_one_triangle():
    R = 0.7
    ang = np.deg2rad([90.0, 210.0, 330.0])
    v = np.stack([R * np.cos(ang), R * np.sin(ang), np.zeros(3)], -1).astype(F)
    heights = np.array([0.05, 0.5, 1.0, 7.0])
    q = np.concatenate([np.stack([0 * heights, 0 * heights, -heights], -1), [[0.1, 0.1, 0.0], [3.0, 0.2, 0.0], [0.3, -0.2, 0.4]]]).astype(F)
    tris = wm.triangles_of(v, None)
    want = wm.exact_winding(tris, q)
    for beta in (_lib.WINDING_BETA_DEFAULT, INF):
        e_model = np.abs(wm.tree_winding(wm.Tree(tris), q, beta) - want).max()   # 0 for beta = inf; the far points take the expansion
        got = winding_numbers(v, Topology.TriangleList(), q, beta=beta)
        assert np.abs(got - want).max() <= 2.0 * e_model + f32_term(1)
        for h, g in zip(heights, got):
            assert abs(g - wm.single_triangle_on_axis(R, h)) <= 2.0 * e_model + 1e-5   # 1e-5: the heights and corners are f32
        assert got[4] == 0.0 and got[5] == 0.0   # in the triangle's plane: no contribution
    d = generate_sdf_winding(v, Topology.TriangleList(), q)
    assert (d > 0).all() and np.array_equal(bits(d), bits(closest_points(v, Topology.TriangleList(), q)[2]))


def test_degenerate_triangles_change_nothing(cases):
    v, idx, q, tris, w, err = cases["closed"]
    rng = np.random.default_rng(5)
    nv = v.shape[0]
    a, b = rng.integers(0, nv, 300), rng.integers(0, nv, 300)
    extra = np.concatenate([np.stack([a, a, a], -1), np.stack([a, b, b], -1), np.stack([a, a, b], -1)]).astype(np.uint32)   # points and segments
    mixed = np.concatenate([idx.reshape(-1, 3), extra])
    mixed = mixed[rng.permutation(mixed.shape[0])].reshape(-1)
    T = mixed.size // 3
    for kw in ({"beta": INF}, {"algorithm": 1}):
        got = winding_numbers(v, Topology.TriangleList(mixed), q, **kw)
        assert np.abs(got.astype(np.float64) - w).max() <= f32_term(T), kw
    b3 = _lib.WINDING_BETA_DEFAULT
    got = winding_numbers(v, Topology.TriangleList(mixed), q)
    assert np.abs(got.astype(np.float64) - w).max() <= 2.0 * err[b3] + f32_term(T)


def test_nan_query_is_nan_and_alone(cases):
    v, idx, q, _, _, _ = cases["closed"]
    q2 = q.copy()
    q2[[7, 64, 1500]] = [[np.nan, 0, 0], [0, np.nan, 0], [np.nan, np.nan, np.nan]]
    ok = np.ones(q.shape[0], bool)
    ok[[7, 64, 1500]] = False
    for kw in ({}, {"beta": INF}, {"algorithm": 1}):
        got = winding_numbers(v, Topology.TriangleList(idx), q2, **kw)
        assert np.isnan(got[~ok]).all() and np.isfinite(got[ok]).all(), kw
    with Mesh(v, Topology.TriangleList(idx)) as m:   # a lane's sum does not depend on its wave-mates
        for beta in (_lib.WINDING_BETA_DEFAULT, INF):
            assert np.array_equal(bits(m.winding_numbers(q2, beta=beta)[ok]), bits(m.winding_numbers(q, beta=beta)[ok]))


def test_strips_and_u16_indices():
    v, idx = meshes.blob(16, 17)
    lo, hi = meshes.extended_bbox(v, 0.4)
    q = meshes.uniform_queries(lo, hi, 700)
    i16 = idx.astype(np.uint16)
    for topology, topo in ((0, Topology.TriangleList(i16)), (1, Topology.TriangleStrip(i16)), (1, Topology.TriangleStrip(idx))):
        tris = wm.triangles_of(v, idx, topology)
        want = wm.exact_winding(tris, q)
        tol = f32_term(tris.shape[0])
        assert np.abs(winding_numbers(v, topo, q, beta=INF).astype(np.float64) - want).max() <= tol, topology
        assert np.abs(winding_numbers(v, topo, q, algorithm=1).astype(np.float64) - want).max() <= tol, topology
    strip = v[idx.astype(np.int64)[:300]]   # no indices: the vertices themselves as a strip
    want = wm.exact_winding(wm.triangles_of(strip, None, 1), q)
    assert np.abs(winding_numbers(strip, Topology.TriangleStrip(), q, beta=INF).astype(np.float64) - want).max() <= f32_term(298)


def test_host_and_device_memory(cases):
    import torch

    v, idx, q, tris, w, err = cases["holed"]
    dv, di, dq = (torch.as_tensor(x, device="cuda") for x in (v, idx.astype(np.int64), q))
    lo, hi = meshes.extended_bbox(v, 0.2)
    grid = Grid.from_bounding_box(lo, hi, [21, 22, 23])
    centres = grid_centres(grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count())
    wg = wm.exact_winding(tris, centres)
    b = _lib.WINDING_BETA_DEFAULT
    tol = 2.0 * err[b] + f32_term(tris.shape[0])
    t = M2STimings()
    host = winding_numbers(v, Topology.TriangleList(idx), q, timings=t)
    assert t.n_units == q.shape[0] and t.n_triangles == tris.shape[0] and t.seed_ms > 0 and t.distance_ms > 0
    assert t.total_ms >= t.distance_ms and t.distance_launches == 1
    dev = winding_numbers(dv, Topology.TriangleList(di), dq)
    assert hasattr(dev, "is_cuda") and dev.is_cuda
    for got in (host, _np(dev)):
        assert np.abs(got.astype(np.float64) - w).max() <= tol
    t = M2STimings()
    hs = generate_grid_sdf_winding(v, Topology.TriangleList(idx), grid, timings=t)
    assert t.distance_launches == 2 and t.n_units == grid.get_total_cell_count()
    ds = _np(generate_grid_sdf_winding(dv, Topology.TriangleList(di), grid))
    assert np.array_equal(bits(np.abs(hs)), bits(np.abs(ds)))
    sure = np.abs(wg - 0.5) > 0.1
    assert np.array_equal((hs < 0)[sure], wg[sure] >= 0.5) and np.array_equal((ds < 0)[sure], wg[sure] >= 0.5)
    # the threshold is the caller's
    lax = generate_grid_sdf_winding(v, Topology.TriangleList(idx), grid, threshold=-1.0)
    assert (lax <= 0).all()


def test_c_and_cpp_programs_run(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["-L", os.path.join(root, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
              "-Wl,-rpath," + os.path.join(root, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib"]
    for cc, std, src in [("gcc", "-std=c99", "tests/c/winding_smoke.c"), ("g++", "-std=c++17", "tests/cpp/winding_tests.cpp")]:
        exe = str(tmp_path / os.path.basename(src).split(".")[0])
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(root, "include"), os.path.join(root, src)] + common
                              + (["-lm"] if cc == "gcc" else []) + ["-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
