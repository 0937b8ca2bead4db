"""Closest-point queries (include/m2s.h m2s_closest_points & co.) without a GPU: the test oracle the GPU tests compare against, checked
against full brute force and against the CPU oracle's closest_point_triangle; the host probe of the device closest point; the argument
checks that fail before any device work; the C and C++ declarations compile with -Wall -Werror."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle as orc
from mesh_to_sdf_amd import M2SPanic, Topology, _lib, closest_points, grid_closest_points, meshes
from mesh_to_sdf_amd.api import Grid

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_TRIANGLE = 0xFFFFFFFF


# ---- the test oracle -----------------------------------------------------------------------------------------------------------
def np_closest_point(p, a, b, c):
    """geo.rs:70-138 (the oracle's closest_point_triangle) over arrays of (n, 3) float32, the reference's operation order, no FMA."""
    def dot(u, v):
        return u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1] + u[:, 2] * v[:, 2]

    def seg(p, a, b):
        ab = b - a
        m = dot(ab, ab)
        s = dot(ab, p - a) / m
        s = np.where(s < 0, F(0), np.where(s > 1, F(1), s)).astype(F)   # f32::clamp, NaN passes through
        return a + ab * s[:, None]

    with np.errstate(all="ignore"):
        p, a, b, c = (np.asarray(x, F) for x in (p, a, b, c))
        ab_eq, bc_eq, ac_eq = (a == b).all(1), (b == c).all(1), (a == c).all(1)
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = dot(ab, ap), dot(ac, ap)
        bp = p - b
        d3, d4 = dot(ab, bp), dot(ac, bp)
        cp = p - c
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        r_e_ab = a + ab * (d1 / (d1 - d3))[:, None]
        r_e_ac = a + ac * (d2 / (d2 - d6))[:, None]
        r_e_bc = b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None]
        denom = F(1) / (va + vb + vc)
        r_in = (a + ab * (vb * denom)[:, None]) + ac * (vc * denom)[:, None]
        out = r_in
        conds = [
            (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), (vb <= 0) & (d2 >= 0) & (d6 <= 0), (vc <= 0) & (d1 >= 0) & (d3 <= 0),
            (d6 >= 0) & (d5 <= d6), (d3 >= 0) & (d4 <= d3), (d1 <= 0) & (d2 <= 0)]
        for cond, val in zip(conds, [r_e_bc, r_e_ac, r_e_ab, c, b, a]):   # last assignment wins = the first test of geo.rs
            out = np.where(cond[:, None], val, out)
        out = np.where((ac_eq & ~ab_eq & ~bc_eq)[:, None], seg(p, a, b), out)
        out = np.where((bc_eq & ~ab_eq)[:, None], seg(p, a, b), out)
        out = np.where((ab_eq & ~(bc_eq & ac_eq))[:, None], seg(p, a, c), out)
        out = np.where((ab_eq & bc_eq & ac_eq)[:, None], a, out)
        return out.astype(F)


def np_dist2(p, q):
    with np.errstate(all="ignore"):
        d = np.asarray(p, F) - q
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(F)


def _pick(n, pi, ti, d2, cp):
    """Lexicographic minimum (d2, t) per point over the pairs (pi, ti); NaN never wins."""
    tri = np.full(n, NO_TRIANGLE, np.uint32)
    pts = np.full((n, 3), np.nan, F)
    ok = ~np.isnan(d2)
    pi, ti, d2, cp = pi[ok], ti[ok], d2[ok], cp[ok]
    order = np.lexsort((ti, d2, pi))
    first = np.ones(order.size, bool)
    first[1:] = pi[order][1:] != pi[order][:-1]
    w = order[first]
    tri[pi[w]] = ti[w]
    pts[pi[w]] = cp[w]
    return tri, pts


def closest_oracle(vertices, indices, points, topology=0, dist=None, brute=False):
    """(triangle, closest point, distance) per point.  |d| per point comes from the CPU oracle's exact generate_sdf (unless given);
    the candidates are the triangles whose padded box (geo.rs:4-22) lies within |d| (1 + 1e-5) plus a small absolute slack; they are
    evaluated with the reference's closest point and the lexicographic minimum (d2, t) is taken.  brute=True: every triangle."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    pts = np.asarray(points, F).reshape(-1, 3)
    tris = orc.get_triangles(v.shape[0], indices, topology).astype(np.int64)
    n, T = pts.shape[0], tris.shape[0]
    A, B, Cc = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    if dist is None:
        dist = orc.generate_sdf(v, indices, pts, accel=3, topology=topology, fast=True)
    d = np.abs(np.asarray(dist, F)).astype(np.float64)
    lo = np.minimum(np.minimum(A, B), Cc).astype(np.float64) - 1e-4
    hi = np.maximum(np.maximum(A, B), Cc).astype(np.float64) + 1e-4
    scale = max(float(np.abs(v).max()), float(np.nanmax(np.abs(pts))) if n else 0.0, 1.0)
    r = d * (1 + 1e-5) + 1e-5 * scale
    r[~np.isfinite(r)] = np.inf
    pis, tis = [], []
    if brute:
        pi, ti = np.meshgrid(np.arange(n), np.arange(T), indexing="ij")
        pis, tis = [pi.reshape(-1)], [ti.reshape(-1)]
    else:
        # spatial groups of ~64 points; per group the triangles whose box meets the group's box grown by its largest radius
        span = np.nanmax(pts, 0) - np.nanmin(pts, 0) if n else np.ones(3)
        cell = float(np.max(span)) / max(1.0, (n / 64.0) ** (1 / 3)) + 1e-30
        key = np.floor((np.nan_to_num(pts.astype(np.float64)) - np.nanmin(pts, 0)) / cell).astype(np.int64)
        key = (key[:, 0] * 1_000_003 + key[:, 1]) * 1_000_033 + key[:, 2]
        order = np.argsort(key, kind="stable")
        cuts = np.flatnonzero(np.diff(key[order])) + 1
        for g in np.split(order, cuts):
            P = pts[g].astype(np.float64)
            R = r[g].max()
            glo, ghi = P.min(0) - R, P.max(0) + R
            cand = np.flatnonzero(((lo <= ghi) & (hi >= glo)).all(1)) if np.isfinite(R) else np.arange(T)
            if np.isnan(P).any():
                cand = np.arange(T)
            if cand.size == 0:
                continue
            gap = np.maximum(np.maximum(lo[cand][None] - P[:, None], P[:, None] - hi[cand][None]), 0.0)
            bd = np.sqrt((gap * gap).sum(-1))
            keep = ~(bd > r[g][:, None])          # NaN (NaN point) keeps the pair
            gi, ci = np.nonzero(keep)
            pis.append(g[gi])
            tis.append(cand[ci])
    pi = np.concatenate(pis) if pis else np.zeros(0, np.int64)
    ti = np.concatenate(tis) if tis else np.zeros(0, np.int64)
    cp = np_closest_point(pts[pi], A[ti], B[ti], Cc[ti])
    d2 = np_dist2(pts[pi], cp)
    tri, cpt = _pick(n, pi, ti, d2, cp)
    with np.errstate(all="ignore"):
        dd = np.minimum(np.sqrt(np_dist2(pts, np.nan_to_num(cpt))), np.finfo(F).max).astype(F)
    dd[tri == NO_TRIANGLE] = np.finfo(F).max
    return tri, cpt, dd


def grid_centres(grid_first, grid_size, count, cells=None):
    """Grid::get_cell_center (grid.rs:135-141) in f32 for the cells (N, 3) given (all cells in grid order by default)."""
    if cells is None:
        cells = np.stack(np.meshgrid(*[np.arange(c) for c in count], indexing="ij"), -1).reshape(-1, 3)
    cells = np.asarray(cells)
    return (np.asarray(grid_first, F)[None] + cells.astype(F) * np.asarray(grid_size, F)[None]).astype(F)


def assert_same_closest(got, want, what=""):
    (gt, gp, gd), (wt, wp, wd) = got, want
    gt = np.asarray(gt).view(np.uint32).reshape(-1)
    bad = np.flatnonzero(gt != wt)
    assert bad.size == 0, f"{what}: triangle differs at {bad[:5]}: got {gt[bad[:5]]} want {wt[bad[:5]]}"
    gp = np.asarray(gp, F).reshape(-1, 3)
    assert np.array_equal(gp.view(np.uint32), np.asarray(wp, F).view(np.uint32)), f"{what}: closest point bits differ"
    assert np.array_equal(np.asarray(gd, F).view(np.uint32), np.asarray(wd, F).view(np.uint32)), f"{what}: distance bits differ"


# ---- self-checks of the test oracle ----------------------------------------------------------------------------------------------
def _tri_cases(n, seed):
    rng = np.random.default_rng(seed)
    P, A, B, Cc = (rng.uniform(-10, 10, (n, 3)).astype(F) for _ in range(4))
    k = np.arange(n) % 12
    B[k == 6] = A[k == 6]
    Cc[k == 7] = B[k == 7]
    Cc[k == 8] = A[k == 8]
    B[k == 9] = A[k == 9]
    Cc[k == 9] = A[k == 9]
    t = rng.random(n).astype(F)[:, None]
    P[k == 5] = (A * (F(1) - t) + B * t).astype(F)[k == 5]                       # on an edge line
    Cc[k == 10] = (A + (B - A) * F(0.5)).astype(F)[k == 10]                       # collinear
    Cc[k == 11] = (A + rng.uniform(-1e-6, 1e-6, (n, 3)).astype(F))[k == 11]       # near-degenerate
    return P, A, B, Cc


def test_np_closest_point_matches_oracle_bits():
    P, A, B, Cc = _tri_cases(3000, 11)
    got = np_closest_point(P, A, B, Cc)
    for i in range(P.shape[0]):
        want = orc.closest_point_triangle(P[i], A[i], B[i], Cc[i])
        assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32)), (i, P[i], A[i], B[i], Cc[i], got[i], want)
        assert np_dist2(P[i:i + 1], got[i:i + 1])[0].view(np.uint32) == orc.point_triangle_distance2(P[i], A[i], B[i], Cc[i]).view(np.uint32)


@pytest.mark.parametrize("topology", [0, 1])
def test_oracle_candidates_equal_brute_force(suzanne, topology):
    v, idx = suzanne
    idx = idx[:900] if topology == 1 else idx
    lo, hi = meshes.extended_bbox(v, 0.3)
    q = np.concatenate([meshes.uniform_queries(lo, hi, 1500), v[:200], np.zeros((1, 3), F)])   # vertices: fans of exact ties
    fast = closest_oracle(v, idx, q, topology)
    brute = closest_oracle(v, idx, q, topology, brute=True)
    assert_same_closest(fast, brute, "candidates vs all pairs")
    want = orc.generate_sdf(v, idx, q, accel=3, topology=topology, fast=True)
    assert np.array_equal(fast[2].view(np.uint32), np.abs(want).view(np.uint32))


def test_oracle_ties_pick_lowest_index():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    idx = np.array([0, 1, 2, 0, 2, 1, 0, 1, 2], np.uint32)   # the same triangle three times, once reversed
    q = np.array([[0.2, 0.2, 1.0], [0.2, 0.2, -1.0], [5, 5, 5]], F)
    tri, pts, d = closest_oracle(v, idx, q)
    assert list(tri) == [0, 0, 0]
    assert np.array_equal(pts[0].view(np.uint32), orc.closest_point_triangle(q[0], v[0], v[1], v[2]).view(np.uint32))


# ---- the host build of the device closest point (geo.hip.h) ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    path = os.path.join(os.path.dirname(_lib.SO_PATH), "libm2s_probe.so")
    if not os.path.exists(path):
        _lib.build()
    L = C.CDLL(path)
    L.probe_closest_point.restype = None
    L.probe_closest_point.argtypes = [C.c_void_p] * 5
    return L


def test_probe_closest_point_bits(probe):
    P, A, B, Cc = _tri_cases(4000, 12)
    out = np.zeros(3, F)
    for i in range(P.shape[0]):
        p, a, b, c = (np.ascontiguousarray(x[i]) for x in (P, A, B, Cc))
        probe.probe_closest_point(p.ctypes.data, a.ctypes.data, b.ctypes.data, c.ctypes.data, out.ctypes.data)
        want = orc.closest_point_triangle(p, a, b, c)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), (i, p, a, b, c, out, want)


# ---- argument checks that need no device ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


def _tri_mesh():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    idx = np.array([0, 1, 2, 0, 2, 3], np.uint32)
    return v, idx


def test_new_entry_points_are_exported(lib):
    for name in ("m2s_closest_points", "m2s_grid_closest_points", "m2s_mesh_closest_points", "m2s_mesh_grid_closest_points"):
        assert name in _lib.EXPORTS and hasattr(lib, name)


def test_bad_arguments_fail_before_the_device(lib):
    v, idx = _tri_mesh()
    q = np.zeros((4, 3), F)
    tri, pts, dist = np.zeros(4, np.uint32), np.zeros((4, 3), F), np.zeros(4, F)
    V, I, Q = v.ctypes.data, idx.ctypes.data, q.ctypes.data
    T, P, D = tri.ctypes.data, pts.ctypes.data, dist.ctypes.data
    BAD = _lib.ERR_BAD_ARG
    cp = lib.m2s_closest_points
    assert cp(V, 4, I, 6, 4, 0, Q, 4, None, None, None, None) == BAD                   # no output at all
    assert cp(V, 4, I, 6, 4, 0, None, 4, T, P, D, None) == BAD                         # NULL queries, n > 0
    assert cp(V, 4, I, 6, 3, 0, Q, 4, T, P, D, None) == BAD                            # index_bytes
    assert cp(V, 4, I, 6, 4, 7, Q, 4, T, P, D, None) == BAD                            # topology
    bad_idx = np.array([0, 1, 2, 0, 2, 4], np.uint32)
    assert cp(V, 4, bad_idx.ctypes.data, 6, 4, 0, Q, 4, T, P, D, None) == BAD          # vertex index out of range
    assert cp(V, 4, bad_idx.ctypes.data, 6, 4, 1, Q, 4, T, P, D, None) == BAD          # ... in a strip
    bad16 = np.array([0, 1, 9], np.uint16)
    assert cp(V, 4, bad16.ctypes.data, 3, 2, 0, Q, 4, T, P, D, None) == BAD
    assert "out of range" in _lib.last_error()
    g = Grid.from_bounding_box([0, 0, 0], [1, 1, 1], [4, 4, 4])
    gcp = lib.m2s_grid_closest_points
    assert gcp(V, 4, I, 6, 4, 0, C.byref(g._g), None, None, None, None) == BAD
    assert gcp(V, 4, I, 6, 4, 0, None, T, P, D, None) == BAD                           # NULL grid
    g0 = Grid.from_bounding_box([0, 0, 0], [1, 1, 1], [4, 0, 4])
    assert gcp(V, 4, I, 6, 4, 0, C.byref(g0._g), T, P, D, None) == BAD                 # a zero cell count
    assert gcp(V, 4, I, 6, 8, 0, C.byref(g._g), T, P, D, None) == BAD                  # index_bytes
    assert gcp(V, 4, I, 6, 4, 2, C.byref(g._g), T, P, D, None) == BAD                  # topology
    assert gcp(V, 4, bad_idx.ctypes.data, 6, 4, 0, C.byref(g._g), T, P, D, None) == BAD
    assert lib.m2s_mesh_closest_points(None, Q, 4, T, P, D, None) == BAD
    assert lib.m2s_mesh_grid_closest_points(None, C.byref(g._g), T, P, D, None) == BAD


def test_empty_mesh_is_reported_before_the_device(lib):
    v, _ = _tri_mesh()
    q = np.zeros((2, 3), F)
    d = np.zeros(2, F)
    empty = np.zeros(4, np.uint32)
    rc = lib.m2s_closest_points(v.ctypes.data, 4, empty.ctypes.data, 0, 4, 0, q.ctypes.data, 2, None, None, d.ctypes.data, None)
    assert rc == _lib.ERR_EMPTY_MESH
    g = Grid.from_bounding_box([0, 0, 0], [1, 1, 1], [2, 2, 2])
    rc = lib.m2s_grid_closest_points(v.ctypes.data, 2, None, 0, 4, 0, C.byref(g._g), None, None, np.zeros(8, F).ctypes.data, None)
    assert rc == _lib.ERR_EMPTY_MESH
    with pytest.raises(M2SPanic):
        closest_points(v, Topology.TriangleList(np.zeros(0, np.uint32)), q)
    with pytest.raises(M2SPanic):
        grid_closest_points(v[:2], Topology.TriangleStrip(), g)


# ---- the declarations compile in C and C++ with -Wall -Werror ---------------------------------------------------------------------
def test_c_declarations_compile(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    exe = str(tmp_path / "closest_smoke")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "closest_smoke.c"), "-L", os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip",
                           "-L", "/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert os.path.exists(exe)


def test_cpp_declarations_compile(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "closest_tests")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "closest_tests.cpp"), "-L", os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip",
                           "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert os.path.exists(exe)
