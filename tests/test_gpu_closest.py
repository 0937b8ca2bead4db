"""Closest-point queries on the MI355X (include/m2s.h m2s_closest_points & co.): triangle, closest point and distance of every point equal
to the test oracle of test_closest_cpu.py bit for bit, the distances equal to the generate calls', and every way of calling gives the same
bits.  Run with `-m gpu`."""
import numpy as np
import pytest

import oracle as orc
from mesh_to_sdf_amd import (AccelerationMethod, Grid, M2SPanic, M2STimings, Mesh, SignMethod, Topology, _lib, closest_points,
                             generate_grid_sdf, generate_sdf, grid_closest_points, meshes)
from test_closest_cpu import NO_TRIANGLE, assert_same_closest, closest_oracle, grid_centres, np_dist2

F = np.float32
pytestmark = pytest.mark.gpu
SUZ_QUERIES = [[0.01, 0.01, 0.5], [1.0, 1.0, 1.0], [0.1, 0.2, 0.2], [1.1, 2.2, 5.2], [-0.1, 0.2, -0.2], [0.0, 0.0, 0.0]]


def _np(res):
    return tuple(x.cpu().numpy() if hasattr(x, "cpu") else x for x in res)


def check_queries(v, idx, q, topology=0, what=""):
    topo = Topology.TriangleList(idx) if topology == 0 else Topology.TriangleStrip(idx)
    got = closest_points(v, topo, q)
    want = closest_oracle(v, idx, q, topology)
    assert_same_closest(got, want, what)
    return got


def check_grid(v, idx, grid, topology=0, what=""):
    topo = Topology.TriangleList(idx) if topology == 0 else Topology.TriangleStrip(idx)
    got = grid_closest_points(v, topo, grid)
    pts = grid_centres(grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count())
    want = closest_oracle(v, idx, pts, topology)
    assert_same_closest(got, want, what)
    return got


@pytest.fixture(scope="module")
def suz16(suzanne):
    v, idx = suzanne
    return v, idx.astype(np.uint16)


def test_suzanne_survey_queries(suz16):
    v, idx = suz16
    tri, pts, d = check_queries(v, idx, np.array(SUZ_QUERIES, F), what="six queries")
    assert (tri != NO_TRIANGLE).all()
    assert np.array_equal(d.view(np.uint32), np.abs(orc.generate_sdf(v, idx.astype(np.uint32), np.array(SUZ_QUERIES, F))).view(np.uint32))


def test_suzanne_uniform_queries(suz16):
    v, idx = suz16
    lo, hi = meshes.extended_bbox(v, 0.3)
    check_queries(v, idx, meshes.uniform_queries(lo, hi, 20000), what="20 k queries")


@pytest.mark.parametrize("topology", [0, 1])
def test_suzanne_grid_64(suz16, topology):
    v, idx = suz16
    lo, hi = meshes.extended_bbox(v, 0.1)
    grid = Grid.from_bounding_box(lo, hi, [64, 64, 64])
    check_grid(v, idx if topology == 0 else idx[:1500], grid, topology, f"suzanne 64^3 topology {topology}")


def test_blob_11k_grid_48():
    v, idx = meshes.named("blob-11k")
    lo, hi = meshes.extended_bbox(v, 0.1)
    check_grid(v, idx, Grid.from_bounding_box(lo, hi, [48, 48, 48]), what="blob-11k 48^3")


# ---- ties -------------------------------------------------------------------------------------------------------------------------
def test_pole_axis_fans():
    v, idx = meshes.blob(40, 31, rotate=False)
    c = v.mean(0)
    poles = [int(np.argmax(v[:, k])) for k in range(3)] + [int(np.argmin(v[:, k])) for k in range(3)]
    q = np.concatenate([(v[p] + (v[p] - c) * F(s)).astype(F)[None] for p in poles for s in (0.0, 0.01, 0.1, 0.5, 2.0)])
    tri, pts, d = check_queries(v, idx, q, what="pole fans")
    assert len(set(tri.tolist())) > 1


def test_duplicated_and_reversed_triangles():
    v, idx = meshes.blob(12, 9)
    t = idx.reshape(-1, 3)
    dup = np.concatenate([t, t[:, ::-1], t]).reshape(-1).astype(np.uint32)
    lo, hi = meshes.extended_bbox(v, 0.3)
    q = np.concatenate([meshes.uniform_queries(lo, hi, 3000), v])
    tri, _, _ = check_queries(v, dup, q, what="duplicates")
    assert (tri < 2 * t.shape[0]).all()   # an exact copy never beats the first (the reversed one may round lower)
    check_grid(v, dup, Grid.from_bounding_box(lo, hi, [20, 24, 28]), what="duplicates, grid")


def test_cube_corner_diagonals():
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], F)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    idx = np.array([[a, b, c, a, c, d] for a, b, c, d in quads], np.uint32).reshape(-1)
    s = np.array([-2.0, -0.5, 0.0, 0.25, 0.5, 0.75, 1.0, 1.5, 3.0], F)
    q = np.concatenate([(k + (F(1) - 2 * k) * s[:, None]).astype(F) for k in corners])   # along the four space diagonals
    check_queries(corners, idx, q, what="cube diagonals")
    check_grid(corners, idx, Grid.from_bounding_box([-0.5] * 3, [1.5] * 3, [9, 9, 9]), what="cube grid")


def test_zero_area_and_collinear_triangles():
    rng = np.random.default_rng(5)
    v = rng.uniform(-1, 1, (60, 3)).astype(F)
    v[10:20] = (v[0:10] + (v[20:30] - v[0:10]) * F(0.5)).astype(F)   # collinear with (i, i + 20)
    tris = [[i, i + 10, i + 20] for i in range(10)] + [[i, i, i + 20] for i in range(30, 40)] + [[i, i, i] for i in range(40, 45)]
    tris += [[i, i + 1, i + 2] for i in range(45, 57)]
    idx = np.array(tris, np.uint32).reshape(-1)
    q = rng.uniform(-1.5, 1.5, (4000, 3)).astype(F)
    check_queries(v, idx, q, what="degenerate")


# ---- slivers: distinct, nearly collinear vertices, whose face normal is rounding noise -------------------------------------------
def _sliver_meshes():
    rng = np.random.default_rng(5)
    v = rng.uniform(-1, 1, (60, 3)).astype(F)
    v[10:20] = (v[0:10] + (v[20:30] - v[0:10]) * F(0.5)).astype(F)
    idx = np.array([[i, i + 10, i + 20] for i in range(10)] + [[i, i + 1, i + 2] for i in range(30, 57)], np.uint32).reshape(-1)
    yield "random slivers", v, idx
    # a closed surface with a sliver along one edge of every third triangle (a, mid(a, c), c): the tessellation pattern of CAD exports
    bv, bi = meshes.blob(60, 51)
    t = bi.reshape(-1, 3)[::3]
    mid = (bv[t[:, 0]] + (bv[t[:, 2]] - bv[t[:, 0]]) * F(0.5)).astype(F)
    m = np.arange(bv.shape[0], bv.shape[0] + t.shape[0], dtype=np.uint32)
    sl = np.stack([t[:, 0], m, t[:, 2]], 1).astype(np.uint32)
    yield "blob with slivers", np.concatenate([bv, mid]), np.concatenate([bi, sl.reshape(-1)])


@pytest.mark.parametrize("brute_max", [None, 0])
def test_sliver_mesh_walks(brute_max):
    """Slivers must not be pruned by their leaf pre-test: with walks for the first pass (M2S_BRUTE_MAX=0 forces them for the small mesh;
    the blob's sets are large enough to walk anyway) the closest calls and the generate calls' distances equal the CPU oracle."""
    for name, v, idx in _sliver_meshes():
        lo, hi = meshes.extended_bbox(v, 0.2)
        q = np.concatenate([meshes.uniform_queries(lo, hi, 40000), v])
        grid = Grid.from_bounding_box(lo, hi, [40, 44, 48])
        centres = grid_centres(grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count())
        with _lib.knobs(**({} if brute_max is None else {"M2S_BRUTE_MAX": brute_max})):
            got_q = closest_points(v, Topology.TriangleList(idx), q)
            got_g = grid_closest_points(v, Topology.TriangleList(idx), grid)
            sdf = generate_sdf(v, Topology.TriangleList(idx), q, AccelerationMethod.RtreeBvh)
            gsdf = generate_grid_sdf(v, Topology.TriangleList(idx), grid, SignMethod.Raycast)
        assert_same_closest(got_q, closest_oracle(v, idx, q), f"{name}: queries")
        assert_same_closest(got_g, closest_oracle(v, idx, centres), f"{name}: grid")
        want_q = np.abs(orc.generate_sdf(v, idx, q, accel=3, fast=True))
        want_g = np.abs(orc.generate_sdf(v, idx, centres, accel=3, fast=True))
        assert np.array_equal(np.abs(sdf).view(np.uint32), want_q.view(np.uint32)), f"{name}: generate_sdf distances"
        assert np.array_equal(np.abs(gsdf).view(np.uint32), want_g.view(np.uint32)), f"{name}: generate_grid_sdf distances"


# ---- blob-100k --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blob100k():
    return meshes.named("blob-100k")


def test_blob_100k_grid_256_stride7(blob100k):
    import torch

    v, idx = blob100k
    lo, hi = meshes.extended_bbox(v, 0.1)
    grid = Grid.from_bounding_box(lo, hi, [256, 256, 256])
    tri, pts, d = grid_closest_points(torch.as_tensor(v, device="cuda"), Topology.TriangleList(torch.as_tensor(idx.astype(np.int64), device="cuda")), grid)
    sub = np.arange(0, 256, 7)
    cells = np.stack(np.meshgrid(sub, sub, sub, indexing="ij"), -1).reshape(-1, 3)
    flat = torch.as_tensor((cells[:, 0] * 256 + cells[:, 1]) * 256 + cells[:, 2], device="cuda")
    got = (tri.view(torch.int32)[flat].cpu().numpy().view(np.uint32), pts[flat].cpu().numpy(), d[flat].cpu().numpy())
    want = closest_oracle(v, idx, grid_centres(grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count(), cells))
    assert_same_closest(got, want, "blob-100k 256^3 / 7")


def test_blob_100k_million_queries(blob100k):
    import torch

    v, idx = blob100k
    lo, hi = meshes.extended_bbox(v, 0.2)
    q = meshes.uniform_queries(lo, hi, 1_000_000)
    dv, di = torch.as_tensor(v, device="cuda"), torch.as_tensor(idx.astype(np.int64), device="cuda")
    got = _np(closest_points(dv, Topology.TriangleList(di), torch.as_tensor(q, device="cuda")))
    sample = np.random.default_rng(3).choice(q.shape[0], 20000, replace=False)
    brute = _np(closest_points(dv, Topology.TriangleList(di), torch.as_tensor(q[sample], device="cuda"), algorithm=1))
    assert_same_closest(tuple(x[sample] for x in got), brute, "1 M queries vs the all-pairs kernel")
    few = sample[:2000]
    assert_same_closest(tuple(x[few] for x in got), closest_oracle(v, idx, q[few]), "1 M queries vs the CPU oracle")


# ---- agreement with the generate calls, and between the ways of calling ----------------------------------------------------------
def test_distances_equal_the_generate_calls(suz16):
    v, idx = suz16
    lo, hi = meshes.extended_bbox(v, 0.3)
    q = meshes.uniform_queries(lo, hi, 30000)
    tri, pts, d = closest_points(v, Topology.TriangleList(idx), q)
    sdf = generate_sdf(v, Topology.TriangleList(idx), q, AccelerationMethod.RtreeBvh)
    assert np.array_equal(d.view(np.uint32), np.abs(sdf).view(np.uint32))
    assert np.array_equal(np.sqrt(np_dist2(q, pts)).view(np.uint32), d.view(np.uint32))
    grid = Grid.from_bounding_box(lo, hi, [40, 52, 36])
    gtri, gpts, gd = grid_closest_points(v, Topology.TriangleList(idx), grid)
    gsdf = generate_grid_sdf(v, Topology.TriangleList(idx), grid, SignMethod.Raycast)
    assert np.array_equal(gd.view(np.uint32), np.abs(gsdf).view(np.uint32))
    centres = grid_centres(grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count())
    assert np.array_equal(np.sqrt(np_dist2(centres, gpts)).view(np.uint32), gd.view(np.uint32))


def test_host_device_mesh_async_identical(suz16):
    import torch

    v, idx = suz16
    lo, hi = meshes.extended_bbox(v, 0.2)
    q = meshes.uniform_queries(lo, hi, 50000)
    grid = Grid.from_bounding_box(lo, hi, [33, 47, 29])
    host_q = closest_points(v, Topology.TriangleList(idx), q)
    host_g = grid_closest_points(v, Topology.TriangleList(idx), grid)
    dv, di, dq = (torch.as_tensor(x, device="cuda") for x in (v, idx.astype(np.int64), q))
    dev_q = _np(closest_points(dv, Topology.TriangleList(di), dq))
    dev_g = _np(grid_closest_points(dv, Topology.TriangleList(di), grid))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        async_q = closest_points(dv, Topology.TriangleList(di), dq)
        async_g = grid_closest_points(dv, Topology.TriangleList(di), grid)
    s.synchronize()
    with Mesh(v, Topology.TriangleList(idx)) as m:
        mesh_q, mesh_g = m.closest_points(q), m.grid_closest_points(grid)
    with Mesh(dv, Topology.TriangleList(di)) as m:
        dmesh_q, dmesh_g = _np(m.closest_points(dq)), _np(m.grid_closest_points(grid))
    for what, r in [("device", dev_q), ("async", _np(async_q)), ("mesh", mesh_q), ("device mesh", dmesh_q)]:
        for a, b in zip(host_q, r):
            assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)), what
    for what, r in [("device", dev_g), ("async", _np(async_g)), ("mesh", mesh_g), ("device mesh", dmesh_g)]:
        for a, b in zip(host_g, r):
            assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)), what
    t = M2STimings()
    closest_points(v, Topology.TriangleList(idx), q, timings=t)
    assert t.n_units == q.shape[0] and t.distance_ms > 0 and 0 < t.seed_ms <= t.distance_ms <= t.total_ms


def test_x_slab_writes_only_its_slab(suz16):
    v, idx = suz16
    lo, hi = meshes.extended_bbox(v, 0.1)
    grid = Grid.from_bounding_box(lo, hi, [24, 20, 28])
    full = grid_closest_points(v, Topology.TriangleList(idx), grid)
    n = grid.get_total_cell_count()
    out = (np.full(n, 0xDEADBEEF, np.uint32), np.full((n, 3), 7.5, F), np.full(n, -3.0, F))
    grid_closest_points(v, Topology.TriangleList(idx), grid, x_slab=(5, 13), out=out)
    row = 20 * 28
    inside = np.zeros(n, bool)
    inside[5 * row:13 * row] = True
    assert (out[0][~inside] == 0xDEADBEEF).all() and (out[1][~inside] == 7.5).all() and (out[2][~inside] == -3.0).all()
    for a, b in zip(full, out):
        assert np.array_equal(a[inside].view(np.uint32), b[inside].view(np.uint32))


def test_mesh_generate_calls_unchanged_after_closest(suz16):
    v, idx = suz16
    lo, hi = meshes.extended_bbox(v, 0.2)
    q = meshes.uniform_queries(lo, hi, 40000)
    grid = Grid.from_bounding_box(lo, hi, [48, 40, 44])
    with Mesh(v, Topology.TriangleList(idx)) as m:
        g0 = m.generate_grid_sdf(grid, SignMethod.Raycast)
        s0 = m.generate_sdf(q, AccelerationMethod.RtreeBvh)
        m.closest_points(q)
        m.grid_closest_points(grid)
        m.closest_points(q[:100], algorithm=1)
        assert np.array_equal(m.generate_grid_sdf(grid, SignMethod.Raycast).view(np.uint32), g0.view(np.uint32))
        assert np.array_equal(m.generate_sdf(q, AccelerationMethod.RtreeBvh).view(np.uint32), s0.view(np.uint32))


def test_empty_mesh(suz16):
    v, _ = suz16
    with pytest.raises(M2SPanic):
        closest_points(v, Topology.TriangleList(np.zeros(0, np.uint32)), np.zeros((3, 3), F))
    with Mesh(v[:2], Topology.TriangleList()) as m:
        assert m.triangle_count() == 0
        with pytest.raises(M2SPanic) as e:
            m.closest_points(np.zeros((3, 3), F))
        assert e.value.code == _lib.ERR_EMPTY_MESH


def test_c_and_cpp_programs_run(tmp_path):
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["-L", os.path.join(root, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
              "-Wl,-rpath," + os.path.join(root, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib"]
    for cc, std, src in [("gcc", "-std=c99", "tests/c/closest_smoke.c"), ("g++", "-std=c++17", "tests/cpp/closest_tests.cpp")]:
        exe = str(tmp_path / os.path.basename(src).split(".")[0])
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(root, "include"), os.path.join(root, src)] + common
                              + (["-lm"] if cc == "gcc" else []) + ["-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
