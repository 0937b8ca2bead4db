"""The queued pairs' unsigned evaluation (csrc/geo.hip.h point_triangle_pair_dist2: every lane its own triangle, read as three vertices and a
class, the edge vectors formed in place, the degenerate classes in a cold block behind the regular body) against the evaluation every other
path uses (point_triangle_dist2 with the edges tri_edges forms at build time, as the records store them), through the host build of both in the
CPU probe library: the same f32 bits for every case, or both NaN."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from mesh_to_sdf_amd import _lib

PROBE = os.path.join(os.path.dirname(_lib.SO_PATH), "libm2s_probe.so")


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        pytest.fail(f"{PROBE} missing: run __graft_entry__.build()")
    L = C.CDLL(PROBE)
    L.probe_pair_dist2_n.restype = None
    L.probe_pair_dist2_n.argtypes = [C.c_size_t] + [C.c_void_p] * 6
    return L


def both(probe, p, a, b, c):
    p, a, b, c = (np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in (p, a, b, c))
    n = p.shape[0]
    assert a.shape[0] == b.shape[0] == c.shape[0] == n
    want, got = np.empty(n, np.float32), np.empty(n, np.float32)
    probe.probe_pair_dist2_n(n, p.ctypes.data, a.ctypes.data, b.ctypes.data, c.ctypes.data, want.ctypes.data, got.ctypes.data)
    return want, got


def assert_same(want, got, what):
    same = (want.view(np.uint32) == got.view(np.uint32)) | (np.isnan(want) & np.isnan(got))
    bad = np.flatnonzero(~same)
    assert bad.size == 0, f"{what}: {bad.size}/{want.size} differ, first {bad[:5]}: want {want[bad[:5]]} got {got[bad[:5]]}"


def degenerate(a, b, c, kind):
    """kind 0: as it is; 1: a == b; 2: b == c; 3: a == c; 4: all equal."""
    a, b, c = a.copy(), b.copy(), c.copy()
    b[kind == 1] = a[kind == 1]
    c[kind == 2] = b[kind == 2]
    c[kind == 3] = a[kind == 3]
    b[kind == 4] = a[kind == 4]
    c[kind == 4] = a[kind == 4]
    return a, b, c


def test_a_million_seeded_cases(probe):
    # triangles of every size against points near and far, a sixth of them of the degenerate classes; half of the points are placed by
    # barycentric coordinates in and around their triangle, so that every region is hit often, the other half anywhere
    rng = np.random.default_rng(20261020)
    n = 1 << 20
    scale = (10.0 ** rng.uniform(-3, 3, (n, 1))).astype(np.float32)
    centre = rng.uniform(-2, 2, (n, 3)).astype(np.float32) * scale
    a, b, c = (centre + rng.normal(0, 1, (n, 3)).astype(np.float32) * scale * np.float32(0.3) for _ in range(3))
    kind = rng.integers(0, 30, n)
    a, b, c = degenerate(a, b, c, np.where(kind < 5, kind, 0))
    w = rng.uniform(-0.7, 1.7, (n, 2)).astype(np.float32)
    nrm = np.cross(b - a, c - a).astype(np.float32)
    near = a + (b - a) * w[:, :1] + (c - a) * w[:, 1:] + nrm * rng.normal(0, 0.5, (n, 1)).astype(np.float32)
    far = centre + rng.normal(0, 3, (n, 3)).astype(np.float32) * scale
    p = np.where(rng.random((n, 1)) < 0.5, near, far).astype(np.float32)
    want, got = both(probe, p, a, b, c)
    assert np.isfinite(want).mean() > 0.99          # the comparison is about numbers
    assert_same(want, got, "seeded cases")


def test_every_region_and_boundary_of_every_class(probe):
    # points at barycentric (u, v) on a grid that holds 0 and 1 — the vertices, the edge lines and their extensions, all seven regions —,
    # in the plane and off it on both sides, for triangles in general position, axis-aligned (exact arithmetic: the region tests meet their
    # equalities) and needle-shaped, each as it is and in the four degenerate forms
    tris = [((0.1, 0.2, 0.3), (1.3, 0.1, 0.5), (0.4, 1.2, 0.2)),
            ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
            ((-2.0, 4.0, 1.0), (2.0, 4.0, 1.0), (0.0, 8.0, 1.0)),
            ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.5, 1e-4, 0.0)),
            ((1000.0, 1000.0, 1000.0), (1000.5, 1000.25, 1000.0), (1000.25, 1000.5, 1000.125))]
    uv = np.array([-1.0, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0], np.float32)
    hs = np.array([0.0, 0.5, -0.5, 1e-6], np.float32)
    P, A, B, Cc = [], [], [], []
    for (a, b, c), kind in itertools.product(tris, range(5)):
        a, b, c = (np.array(x, np.float32)[None] for x in (a, b, c))
        n = np.cross(b - a, c - a).astype(np.float32)      # of the regular form: the degenerate ones get the same points
        u, v, h = (g.ravel()[:, None] for g in np.meshgrid(uv, uv, hs, indexing="ij"))
        p = (a + (b - a) * u + (c - a) * v + n * h).astype(np.float32)
        da, db, dc = degenerate(a, b, c, np.array([kind]))
        for lst, x in ((P, p), (A, da), (B, db), (Cc, dc)):
            lst.append(np.broadcast_to(x, p.shape))
        for vtx in (da, db, dc):                           # the point ON each vertex
            for lst, x in ((P, vtx), (A, da), (B, db), (Cc, dc)):
                lst.append(x)
    want, got = both(probe, *(np.concatenate(x) for x in (P, A, B, Cc)))
    assert want.size == 5 * 5 * (11 * 11 * 4 + 3)
    assert_same(want, got, "regions and boundaries")


SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, 1e-30, -1e-30, 1e30, -1e30, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.5], np.float32)


def test_special_values(probe):
    # one special coordinate in an otherwise ordinary case, at each of the twelve places and for every class (the NaN / inf vertex of a
    # real mesh), then every coordinate drawn from the special values (mostly NaN results: both must be)
    rng = np.random.default_rng(7)
    base = np.array([[0.3, 0.4, 0.9], [0.1, 0.2, 0.3], [1.3, 0.1, 0.5], [0.4, 1.2, 0.2]], np.float32)   # p, a, b, c
    rows, kinds = [], []
    for place, s, kind in itertools.product(range(12), SPECIAL, range(5)):
        x = base.copy()
        x.reshape(-1)[place] = s
        rows.append(x)
        kinds.append(kind)
    x = np.stack(rows)
    a, b, c = degenerate(x[:, 1], x[:, 2], x[:, 3], np.array(kinds))
    want, got = both(probe, x[:, 0], a, b, c)
    assert_same(want, got, "one special coordinate")
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()

    n = 200000
    x = SPECIAL[rng.integers(0, SPECIAL.size, (n, 4, 3))]
    a, b, c = degenerate(x[:, 1], x[:, 2], x[:, 3], rng.integers(0, 5, n))
    want, got = both(probe, x[:, 0], a, b, c)
    assert_same(want, got, "all coordinates special")
    # ... and special values times ordinary ones: denormal and huge triangles with finite results
    x = (SPECIAL[[2, 4, 5, 7, 12]][rng.integers(0, 5, (n, 1, 1))] * rng.uniform(-2, 2, (n, 4, 3)).astype(np.float32)).astype(np.float32)
    a, b, c = degenerate(x[:, 1], x[:, 2], x[:, 3], rng.integers(0, 5, n))
    want, got = both(probe, x[:, 0], a, b, c)
    assert_same(want, got, "scaled cases")
