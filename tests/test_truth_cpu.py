"""Ray casts and closest points against float64 geometry (tests/geometry_f64.py), without a GPU.

The other tests pin the kernels to numpy float32 twins of the contract (tests/ray_model.py, test_closest_cpu.np_closest_point, the CPU
oracle).  Here the twins themselves are held against geometry that shares no code with them: which triangles a ray meets, where, and
how far a point is from the mesh.  The cases, the assertions and the recorded figures (tests/golden/truth_error.json) are shared with
tests/test_gpu_truth.py, which applies them to what the device returns.

Rays.  A (ray, triangle) pair is a CLEAR hit or miss when its float64 edge functions decide it by more than M L^2 (M = 2^-18, four times
the 2^-20 = 16 u that DESIGN.md 4.10 grants a computed edge function; L = the largest term of the image's coordinates), ambiguous
otherwise.  Clear pairs must be reported as they are, ambiguous ones may go either way, and the conditions on the inputs (how many pairs
are ambiguous, how many rays are clear throughout) are asserted on the reference alone.

Closest points.  The returned point lies on the returned triangle, its distance from the query is the returned distance, that
distance is never below the true one, and it exceeds it by a bounded amount, all in units of u x the coordinate scale.  The constants
are measured on the reference arithmetic (the oracle and its numpy twin) and recorded with twice their value (at least 1 u s) as the bound:
`python tests/test_truth_cpu.py` rewrites the file.
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))] + ([] if ROOT in sys.path else [ROOT])
import geometry_f64 as g64  # noqa: E402
import oracle as orc  # noqa: E402
import ray_model as rm  # noqa: E402
from mesh_to_sdf_amd import Grid, meshes  # noqa: E402
from test_closest_cpu import closest_oracle, grid_centres  # noqa: E402
from test_gpu_closest import _sliver_meshes  # noqa: E402
from test_gpu_rays import RANGE, _rays  # noqa: E402

F = np.float32
U = 2.0 ** -24
M = 2.0 ** -18
INF = float("inf")
GOLDEN = os.path.join(ROOT, "tests", "golden", "truth_error.json")
RANGES = ((0.0, INF), RANGE)


# ---- ray cases ------------------------------------------------------------------------------------------------------------------------
def soup(n=300, seed=77):
    """A seeded soup of n triangles: every tenth a needle (its third vertex within 1e-5 of an edge), two spanning +-50."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-1, 1, (n, 1, 3)) + 0.15 * rng.normal(size=(n, 3, 3))
    k = np.arange(0, n, 10)
    s = rng.uniform(0, 1, (k.size, 1))
    t[k, 2] = t[k, 0] + s * (t[k, 1] - t[k, 0]) + rng.uniform(-1e-5, 1e-5, (k.size, 3))
    t[[5, n // 2 + 5]] = rng.uniform(-50, 50, (2, 3, 3))
    return t.reshape(-1, 3).astype(F), np.arange(3 * n, dtype=np.uint32)


def _blob12(offset=(0, 0, 0), scale=(1, 1, 1)):
    v, idx = meshes.blob(12, 9)
    return ((v * np.asarray(scale, F)).astype(F) + np.asarray(offset, F)).astype(F), idx


# name -> (mesh, (radial, box, inside, axis) rays, closed, the share of ambiguous pairs allowed)
RAY_CASES = {
    "cube": (meshes.cube, (64, 1500, 500, 900), True, 0.10),   # its axis rays are snapped onto vertex coordinates: they lie in face planes
    "blob-192": (_blob12, (4000, 2000, 500, 500), True, 0.01),
    "blob-192-far": (lambda: _blob12(offset=(1e4, -1e4, 1e4)), (4000, 2000, 500, 500), True, 0.01),
    "blob-192-scaled": (lambda: _blob12(scale=(100, 1, 0.01)), (4000, 2000, 500, 500), True, 0.01),
    "soup-300": (soup, (900, 2000, 500, 500), False, 0.01),
    "blob-6144": (lambda: meshes.blob(48, 65), (100, 100, 100, 100), True, 0.01),
}
_ray_cache = {}


def ray_case(name):
    """(vertices, indices, origins, directions, reference) of a named case; the reference (see `ray_reference`) is computed once per
    process for the most recent case only: its arrays are R x T f64."""
    if name not in _ray_cache:
        _ray_cache.clear()
        maker, sizes, closed, limit = RAY_CASES[name]
        v, idx = maker()
        o, d = _rays(v, idx, 1000 + 7 * list(RAY_CASES).index(name), *sizes)
        _ray_cache[name] = (v, idx, o, d, ray_reference(name, v, idx, o, d))
    return _ray_cache[name]


def ray_reference(name, v, idx, o, d):
    """The f64 side of a case, with the conditions on the inputs asserted on it alone."""
    _, _, closed, limit = RAY_CASES[name]
    tris = rm.triangles_of(v, idx)
    pairs = g64.ray_pairs(tris, o, d)
    assert pairs["valid"].all()
    hit, miss = g64.classify(pairs, M)
    tb, wb = g64.ray_bounds(pairs)
    ambiguous = ~hit & ~miss
    share, clear_rays = ambiguous.mean(), (~ambiguous.any(1)).mean()
    print(f"{name}: {o.shape[0]} rays x {tris.shape[0]} triangles, ambiguous pairs {100 * share:.3f} %, fully clear rays {100 * clear_rays:.1f} %")
    assert share <= limit, f"{name}: {100 * share:.2f} % of the pairs are ambiguous"
    assert clear_rays >= 0.5, f"{name}: only {100 * clear_rays:.1f} % of the rays are clear throughout"
    ref = {"tris": tris, "pairs": pairs, "hit": hit, "miss": miss, "tb": tb, "wb": wb, "closed": closed}
    if closed:   # the reference against itself: on rays clear throughout, crossings in front of the origin have the winding number's parity
        inside, outside = g64.range_classes(pairs, tb, 0.0, INF)
        sure = ~ambiguous.any(1) & ~(hit & ~inside & ~outside).any(1)
        w = g64.solid_angle_winding(tris, o[sure])
        assert np.abs(w - np.round(w)).max() < 1e-6 and set(np.abs(np.round(w)).astype(int)) == {0, 1}
        crossings = (hit & inside)[sure].sum(1)
        assert sure.mean() >= 0.5 and np.array_equal(crossings % 2, np.abs(np.round(w)).astype(int) % 2), name
        ref["enters_by"] = surface_crossed_by(tris, o, d, pairs, miss)
        print(f"{name}: {100 * np.isfinite(ref['enters_by']).mean():.1f} % of the rays provably cross the surface")
        assert np.isfinite(ref["enters_by"]).mean() >= 0.2, name
    return ref


def surface_crossed_by(tris, o, d, pairs, miss):
    """Watertightness, from the solid itself and no pair: per ray of a closed mesh a parameter m by which the ray has provably crossed the
    surface, +inf where nothing is claimed.  m lies behind the first group of triangles the ray may touch (pairs that are no clear
    miss, within 1 % of the mesh's smallest extent of the first of them) and in front of the next one; where the solid-angle winding number at
    o + m d differs from the origin's, the ray has passed from outside to inside or back, whatever it met on the way: a vertex, an edge
    or a face.  A cast over [0, inf] must report a hit with t <= m there."""
    tris64 = np.asarray(tris, np.float64)
    o64, d64 = np.asarray(o, np.float64), np.asarray(d, np.float64)
    size = (tris64.reshape(-1, 3).max(0) - tris64.reshape(-1, 3).min(0)).min()
    step = 0.01 * size / np.abs(d64).max(1)   # (|d| within sqrt(3) of its largest component)
    with np.errstate(invalid="ignore"):
        tt = np.where(~miss & (pairs["t"] > 0) & np.isfinite(pairs["t"]), pairs["t"], np.inf)
    first = tt.min(1)
    edge = (first + step)[:, None]
    ta, tn = np.where(tt <= edge, tt, -np.inf).max(1), np.where(tt > edge, tt, np.inf).min(1)
    with np.errstate(invalid="ignore"):
        m = np.where(np.isfinite(tn), 0.5 * (ta + tn), ta + step)
        ok = np.isfinite(first) & (np.where(np.isfinite(tn), tn - ta, step) > 1e-4 * step)
    rows = np.flatnonzero(ok)
    w0 = g64.solid_angle_winding(tris64, o64[rows])
    w1 = g64.solid_angle_winding(tris64, o64[rows] + m[rows, None] * d64[rows])
    whole = (np.abs(w0 - np.round(w0)) < 1e-6) & (np.abs(w1 - np.round(w1)) < 1e-6)
    crossed = whole & (np.round(w0) != np.round(w1))
    out = np.full(o64.shape[0], np.inf)
    out[rows[crossed]] = m[rows[crossed]]
    return out


def check_rays(ref, got, t_min, t_max, what):
    """Every ray assertion, for one call's outputs `got` (t, triangle, uv, count, occluded as numpy) over [t_min, t_max].  Returns the
    largest |t - t64| / tb and |uv - uv64| / wb over reported clear hits."""
    pairs, hit, miss, tb, wb = (ref[k] for k in ("pairs", "hit", "miss", "tb", "wb"))
    R, T = hit.shape
    t, tri, uv = np.asarray(got["t"], np.float64), np.asarray(got["triangle"]).astype(np.int64), np.asarray(got["uv"], np.float64)
    count, occluded = np.asarray(got["count"]).astype(np.int64), np.asarray(got["occluded"]).astype(np.int64)
    inside, outside = g64.range_classes(pairs, tb, t_min, t_max)
    sure, maybe = hit & inside, ~miss & ~outside
    lo, hi = sure.sum(1), maybe.sum(1)

    def rays(mask):
        return f"{what}: {int(mask.sum())} rays, first {np.flatnonzero(mask)[:5]}"

    # count and occlusion
    assert not (count < lo).any(), "clear hits in range not counted, " + rays(count < lo)
    assert not (count > hi).any(), "more counted than clear and ambiguous pairs in range, " + rays(count > hi)
    assert not ((lo > 0) & (occluded != 1)).any(), "a clear hit in range, not occluded, " + rays((lo > 0) & (occluded != 1))
    assert not ((hi == 0) & (occluded != 0)).any(), "occluded by nothing, " + rays((hi == 0) & (occluded != 0))
    # the reported triangle
    rep = tri != int(rm.NONE)
    assert np.array_equal(rep, np.isfinite(t)) and np.array_equal(rep, ~np.isnan(uv).any(1)), what
    assert not ((lo > 0) & ~rep).any(), "a clear hit in range, nothing reported, " + rays((lo > 0) & ~rep)
    assert not ((hi == 0) & rep).any(), "a hit reported where nothing can be hit, " + rays((hi == 0) & rep)
    r = np.flatnonzero(rep)
    k = tri[r]
    assert (k < T).all() and (t[r] >= F(t_min)).all() and (t[r] <= F(t_max)).all(), what
    bad = miss[r, k] | outside[r, k]
    assert not bad.any(), f"{what}: a clear miss or a pair clearly out of range reported on rays {r[bad][:5]}, triangles {k[bad][:5]}"
    c = hit[r, k]
    rc, kc = r[c], k[c]
    et, ew = np.abs(t[rc] - pairs["t"][rc, kc]) / tb[rc, kc], np.abs(uv[rc] - np.stack([pairs["u"][rc, kc], pairs["v"][rc, kc]], -1)).max(1) / wb[rc, kc]
    assert rc.size > 0
    assert (et <= 1).all(), f"{what}: |t - t64| up to {et.max():.3g} tb, ray {rc[et.argmax()]} triangle {kc[et.argmax()]}"
    assert (ew <= 1).all(), f"{what}: |uv - uv64| up to {ew.max():.3g} wb, ray {rc[ew.argmax()]} triangle {kc[ew.argmax()]}"
    if "enters_by" in ref and t_min == 0.0 and t_max == INF:   # a closed mesh lets no ray through, at a vertex or an edge either
        leak = ~(t <= ref["enters_by"]) & np.isfinite(ref["enters_by"])
        assert not leak.any(), "the ray crosses the closed surface and no hit is reported by then, " + rays(leak)
        assert not ((count == 0) | (occluded != 1))[np.isfinite(ref["enters_by"])].any(), what
    # never beyond the first clear hit, and that hit itself where nothing else is near it
    with np.errstate(invalid="ignore"):
        limit = np.where(sure, pairs["t"] + tb, np.inf).min(1)
        assert not (t > limit).any(), "t beyond the first clear hit, " + rays(t > limit)
        t_sure = np.where(sure, pairs["t"], np.inf)
        first = t_sure.argmin(1)
        rows = np.arange(R)
        tf, tbf = t_sure[rows, first], tb[rows, first]
        other = maybe.copy()
        other[rows, first] = False
        apart = pairs["t"] - tf[:, None] > 2 * np.maximum(tb, tbf[:, None])   # NaN (an ambiguous pair without a t or a tb) is not apart
        alone = (lo > 0) & ~(other & ~apart).any(1)
    assert alone.any(), f"{what}: none of {(lo > 0).sum()} first hits stands alone"
    wrong = alone & (tri != first)
    assert not wrong.any(), "the first clear hit stands alone and another triangle is reported, " + rays(wrong)
    return float(et.max()), float(ew.max())


# ---- rays: the model --------------------------------------------------------------------------------------------------------------------
def test_ray_frame_is_right_handed():
    """The contract's (kx, ky, kz): kz the dominant axis, and e_kx x e_ky along the ray, so that the edge functions have the sign of
    d . (C x B) whichever way the ray points.  This pins a CONVENTION of the contract (include/m2s.h: "kx and ky swapped if d[kz] < 0"),
    not geometry: a mirrored frame negates U, V, W and det together and leaves every hit, t and uv as they are, bit for bit, so no
    float64 assertion on the outputs can see kx and ky exchanged; only this look at ray_setup does."""
    rng = np.random.default_rng(3)
    d = rng.normal(size=(4000, 3)).astype(F)
    d[:600, 0] = 0
    d[300:900, 1] = 0
    d[::7] *= F(-1)
    d = d[np.abs(d).max(1) > 0]
    kx, ky, kz, Sx, Sy, Sz, valid = rm.ray_setup(np.zeros_like(d), d)
    assert valid.all() and np.array_equal(np.abs(d)[np.arange(d.shape[0]), kz], np.abs(d).max(1))
    eye = np.eye(3)
    assert ((np.cross(eye[kx], eye[ky]) * d.astype(np.float64)).sum(1) > 0).all()
    assert (np.sign(Sz) == np.sign(d[np.arange(d.shape[0]), kz])).all()


def test_xy_margin_keeps_hits_whose_edge_functions_round_to_zero():
    """the XY clause's 2^-20 L "keeps every hit of a non-degenerate image".  On the ray sets of this file, and on two
    million rays aimed at vertices and edges, the clause never fires at all, with its margin or without, so what the margin is for has
    to be built: a well-shaped triangle whose vertex image lies one denormal off the axis, so that the two edge functions at that vertex
    underflow to zero (the sheared coordinates are exact for a ray along z from the origin).  The paper's test reports the hit; the
    axis is outside the bare rectangle of the image (by 1.4e-45) and inside the widened one.  In float64 the pair is ambiguous, as it
    must be, and the axis is within 2^-20 L of the triangle.  The contract's test and the host build of ray.hip.h keep the hit."""
    import ctypes as C

    from mesh_to_sdf_amd import _lib

    tiny = np.float32(1.4e-45)
    assert tiny > 0 and tiny * F(0.25) == 0
    base = np.array([[tiny, tiny, 1], [0.25, 0.1, 1], [0.1, 0.25, 1]], F)
    tris = np.stack([(base * np.array([sx, sy, 1], F))[order] for sx in (1, -1) for sy in (1, -1) for order in ([0, 1, 2], [0, 2, 1], [1, 2, 0])])
    n = tris.shape[0]
    o, d = np.zeros((n, 3), F), np.tile(np.array([0, 0, 1], F), (n, 1))
    setup = rm.ray_setup(o, d)[:6]
    bare = rm.line_test(setup, o, tris[:, 0], tris[:, 1], tris[:, 2], bare=True)[0]
    assert bare.all()   # the case is what it claims to be
    assert (np.abs(tris[:, :, 0]).min(1) > 0).all() and (np.sign(tris[:, :, 0]).min(1) == np.sign(tris[:, :, 0]).max(1)).all()   # the axis is off the bare rectangle
    pairs = g64.ray_pairs(tris, o[:1], d[:1])
    hit, miss = g64.classify(pairs, M)
    assert not hit.any() and not miss.any()
    image = tris.astype(np.float64)
    image[:, :, 2] = 0
    off = g64.point_triangle(np.zeros((n, 3)), image[:, 0], image[:, 1], image[:, 2])[1]
    assert (off <= 2.0 ** -20 * pairs["L"][0]).all() and (np.abs(pairs["det"][0]) > 0.01 * pairs["L"][0] ** 2).all()   # near, and not degenerate
    meets, t, _, _ = rm.line_test(setup, o, tris[:, 0], tris[:, 1], tris[:, 2])
    assert meets.all() and (t == 1).all()
    probe = C.CDLL(os.path.join(os.path.dirname(_lib.SO_PATH), "libm2s_probe.so"))
    probe.probe_ray_triangle.restype = C.c_int
    probe.probe_ray_triangle.argtypes = [C.c_void_p] * 5 + [C.c_float, C.c_float, C.c_void_p]
    for i in range(n):
        tuv = np.zeros(3, F)
        a, b, c = (np.ascontiguousarray(tris[i, k]) for k in range(3))
        assert probe.probe_ray_triangle(o[i].ctypes.data, d[i].ctypes.data, a.ctypes.data, b.ctypes.data, c.ctypes.data, 0.0, INF, tuv.ctypes.data) == 1, i
        assert tuv[0] == 1


@pytest.mark.parametrize("name", list(RAY_CASES))
def test_ray_model_against_f64(name):
    v, idx, o, d, ref = ray_case(name)
    tris = ref["tris"]
    # pair by pair, without a range: the model's line test reports every clear hit and no clear miss, with the sign of the f64 det
    setup = rm.ray_setup(o, d)
    for s in range(0, o.shape[0], 256):
        e = slice(s, s + 256)
        meets, t, u, w = rm.line_test(tuple(x[e, None] for x in setup[:6]), o[e, None, :], tris[None, :, 0], tris[None, :, 1], tris[None, :, 2])
        assert not (ref["hit"][e] & ~meets).any(), f"{name}: clear hits missed, rays {s + np.flatnonzero((ref['hit'][e] & ~meets).any(1))[:5]}"
        assert not (ref["miss"][e] & meets).any(), f"{name}: clear misses reported, rays {s + np.flatnonzero((ref['miss'][e] & meets).any(1))[:5]}"
        c = ref["hit"][e] & meets
        with np.errstate(invalid="ignore"):
            et = np.abs(t.astype(np.float64) - ref["pairs"]["t"][e])[c] / ref["tb"][e][c]
            ew = np.maximum(np.abs(u - ref["pairs"]["u"][e]), np.abs(w - ref["pairs"]["v"][e]))[c] / ref["wb"][e][c]
        assert (et <= 1).all() and (ew <= 1).all(), f"{name}: a clear hit's t off by {et.max():.3g} tb, uv by {ew.max():.3g} wb"
    for t_min, t_max in RANGES:
        et, ew = check_rays(ref, rm.cast(tris, o, d, t_min, t_max), t_min, t_max, f"{name} [{t_min}, {t_max}]")
        print(f"{name} [{t_min}, {t_max}]: first hits' |t - t64| <= {et:.3f} tb, |uv - uv64| <= {ew:.3f} wb")


# ---- closest-point cases -------------------------------------------------------------------------------------------------------------------
def strip():
    """A generically rotated 10 x 0.01 strip of two triangles."""
    q = np.array([[0, 0, 0], [10, 0, 0], [10, 0.01, 0], [0, 0.01, 0]], np.float64) - [5, 0.005, 0]
    return (q @ meshes._rotation().T).astype(F), np.array([0, 1, 2, 0, 2, 3], np.uint32)


def _suzanne():
    d = np.load(os.path.join(ROOT, "tests", "golden", "suzanne.npz"))
    return d["vertices"].astype(F), d["indices"].astype(np.uint32)


def _blob24_far():
    v, idx = meshes.blob(24, 17)
    return (v + np.array([1e4, -1e4, 1e4], F)).astype(F), idx


# name -> (mesh, well shaped: the excess over the true distance is bounded by k_up; otherwise it is the reference's arithmetic, recorded)
CLOSEST_CASES = {
    "cube": (meshes.cube, True),
    "blob-768": (lambda: meshes.blob(24, 17), True),
    "suzanne": (_suzanne, True),
    "blob-768-far": (_blob24_far, True),
    "random slivers": (lambda: list(_sliver_meshes())[0][1:], False),
    "blob with slivers": (lambda: list(_sliver_meshes())[1][1:], False),
    "strip": (strip, False),
}
GRID = (24, 21, 19)
N_QUERIES = 3000


def closest_case(name):
    """(vertices, indices, queries [3000, 3], grid): uniform queries in the 0.3-extended box, the first 200 vertices, 200 points within
    1e-3 of the surface; a 24 x 21 x 19 grid over the 0.1-extended box."""
    v, idx = CLOSEST_CASES[name][0]()
    rng = np.random.default_rng(500 + list(CLOSEST_CASES).index(name))
    tris = rm.triangles_of(v, idx).astype(np.float64)
    k = rng.integers(0, tris.shape[0], 200)
    w = rng.dirichlet((1, 1, 1), 200)
    near = (tris[k] * w[:, :, None]).sum(1) + rng.uniform(-1e-3, 1e-3, (200, 3)) / np.sqrt(3)
    verts = v[:200]
    lo, hi = meshes.extended_bbox(v, 0.3)
    q = np.concatenate([meshes.uniform_queries(lo, hi, N_QUERIES - 200 - verts.shape[0]), verts, near.astype(F)])
    return v, idx, q, Grid.from_bounding_box(*meshes.extended_bbox(v, 0.1), list(GRID))


def grid_points(grid):
    return grid_centres(grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count())


def closest_figures(v, idx, p, tri, cp, d, truth=None):
    """The four ratios and the excess of one closest-point result (triangle [N], point [N, 3], distance [N]) for the points p, each the
    maximum over the points, in units of u s, s = the largest |coordinate| among the point and the mesh's vertices:
      k_on   the f64 distance of the returned point from the returned triangle
      k_len  | |p - cp| - d |
      k_low  D64 - d, how far the distance is BELOW the true distance to the mesh
      k_up   d - D64, and k_tri: the f64 distance of p from the returned triangle, less D64
    plus `excess`, `excess_p999`: max and 99.9th percentile of d - D64 in the mesh's own units.  truth: (D64, near) to reuse."""
    tris = rm.triangles_of(v, idx).astype(np.float64)
    p, cp, d = np.asarray(p, np.float64), np.asarray(cp, np.float64), np.asarray(d, np.float64)
    tri = np.asarray(tri).astype(np.int64)
    assert (tri >= 0).all() and (tri < tris.shape[0]).all() and np.isfinite(cp).all() and np.isfinite(d).all()
    D64 = g64.mesh_distance(p, tris)[0] if truth is None else truth
    us = U * np.maximum(np.abs(p).max(1), float(np.abs(v).max()))
    a, b, c = tris[tri, 0], tris[tri, 1], tris[tri, 2]
    on = g64.point_triangle(cp, a, b, c)[1]
    own = g64.point_triangle(p, a, b, c)[1]
    return {"k_on": float((on / us).max()), "k_len": float((np.abs(np.sqrt(((p - cp) ** 2).sum(1)) - d) / us).max()),
            "k_low": float(((D64 - d) / us).max()), "k_up": float(((d - D64) / us).max()), "k_tri": float(((own - D64) / us).max()),
            "excess": float((d - D64).max()), "excess_p999": float(np.percentile(d - D64, 99.9))}


KS = ("k_on", "k_len", "k_low", "k_up", "k_tri")


def assert_within_file(name, fig, what):
    """A result's figures against the recorded bounds of its mesh: k_on, k_len, k_low everywhere; k_up and k_tri on the well-shaped
    meshes; on the others the recorded maximum excess itself."""
    want = json.load(open(GOLDEN))["closest"][name]
    well = CLOSEST_CASES[name][1]
    for k in KS if well else KS[:3]:
        assert fig[k] <= want[k]["bound"], f"{what}: {k} = {fig[k]:.4g} u s, recorded maximum {want[k]['max']:.4g}, bound {want[k]['bound']:.4g}"
    if not well:
        assert fig["excess"] <= want["excess"]["max"], f"{what}: excess {fig['excess']:.4g} over the recorded maximum {want['excess']['max']:.4g}"


def oracle_figures(name):
    """The figures of the reference arithmetic on a case's queries and grid centres together."""
    v, idx, q, grid = closest_case(name)
    p = np.concatenate([q, grid_points(grid)])
    signed = orc.generate_sdf(v, idx, p, accel=3, fast=True)
    tri, cp, d = closest_oracle(v, idx, p, dist=signed)
    assert np.array_equal(np.abs(signed).view(np.uint32), d.view(np.uint32))
    return closest_figures(v, idx, p, tri, cp, d), int(idx.size // 3), int(p.shape[0])


def bound_of(measured):
    """Twice the measured maximum, and at least 1 u s: a result is made of f32 numbers, a single rounding of one coordinate of size s
    moves it by up to u s, so a maximum that happens to be smaller (0 on the cube, whose coordinates are exact) bounds nothing once the
    query set is re-seeded."""
    return max(2.0 * measured, 1.0)


def record(fig, triangles, points, well):
    out = {"triangles": triangles, "points": points}
    for k in KS if well else KS[:3]:
        out[k] = {"max": fig[k], "bound": bound_of(fig[k])}
    if not well:
        out["excess"] = {"max": fig["excess"], "p999": fig["excess_p999"], "max_in_u_s": fig["k_up"]}
    return out


# ---- closest points: the f64 reference on known answers, then the oracle -----------------------------------------------------------------
def test_f64_point_triangle_known_answers():
    a, b, c = np.array([[0.0, 0, 0]]), np.array([[2.0, 0, 0]]), np.array([[0.0, 2, 0]])
    for p, q in (([0.5, 0.5, 3], [0.5, 0.5, 0]), ([-1, -1, 1], [0, 0, 0]), ([1, -2, 0], [1, 0, 0]), ([2, 2, 0], [1, 1, 0]), ([5, -1, 0], [2, 0, 0])):
        got, dist = g64.point_triangle([p], a, b, c)
        assert np.allclose(got[0], q, atol=1e-15) and abs(dist[0] - np.linalg.norm(np.subtract(p, q))) < 1e-15
    # degenerate: collinear (a segment) and a point
    got, dist = g64.point_triangle([[1.0, 1, 0]], a, b, np.array([[1.0, 0, 0]]))
    assert np.allclose(got[0], [1, 0, 0]) and dist[0] == 1
    got, dist = g64.point_triangle([[3.0, 4, 0]], a, a, a)
    assert np.allclose(got[0], 0) and dist[0] == 5
    # against dense sampling of random triangles and slivers: never above the nearest sample, below it by at most the sample spacing
    rng = np.random.default_rng(8)
    p, a, b, c = (rng.uniform(-1, 1, (300, 3)) for _ in range(4))
    c[::3] = a[::3] + 0.5 * (b[::3] - a[::3]) + 1e-7 * rng.normal(size=c[::3].shape)
    _, dist = g64.point_triangle(p, a, b, c)
    s = np.linspace(0, 1, 65)
    w = np.array([(x, y, 1 - x - y) for x in s for y in s if x + y <= 1 + 1e-12])
    samples = w[None, :, 0, None] * a[:, None] + w[None, :, 1, None] * b[:, None] + w[None, :, 2, None] * c[:, None]
    nearest = np.sqrt(((samples - p[:, None]) ** 2).sum(-1)).min(1)
    span = np.maximum(np.maximum(np.linalg.norm(b - a, axis=1), np.linalg.norm(c - a, axis=1)), np.linalg.norm(c - b, axis=1))
    assert (dist <= nearest + 1e-12).all() and (dist >= nearest - span / 64).all()


def test_f64_mesh_distance_equals_all_pairs():
    v, idx = meshes.blob(12, 9)
    tris = rm.triangles_of(v, idx).astype(np.float64)
    p = meshes.uniform_queries(*meshes.extended_bbox(v, 0.3), 400).astype(np.float64)
    P, T = np.repeat(p, tris.shape[0], 0), np.tile(tris, (p.shape[0], 1, 1))
    every = g64.point_triangle(P, T[:, 0], T[:, 1], T[:, 2])[1].reshape(p.shape[0], -1)
    dist, (pi, ti) = g64.mesh_distance(p, tris, tol=0.01)
    assert np.array_equal(dist, every.min(1))
    want = every <= every.min(1)[:, None] + 0.01
    got = np.zeros_like(want)
    got[pi, ti] = True
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", list(CLOSEST_CASES))
def test_closest_oracle_against_f64(name):
    """The reference arithmetic's figures stay within the recorded bounds, and the file holds what it says: bound = 2 x maximum."""
    fig, triangles, points = oracle_figures(name)
    print(name, json.dumps(fig))
    want = json.load(open(GOLDEN))["closest"][name]
    assert want["triangles"] == triangles and want["points"] == points
    for k, rec in want.items():
        if isinstance(rec, dict) and "bound" in rec:
            assert rec["bound"] == bound_of(rec["max"])
    assert_within_file(name, fig, f"{name}, oracle")


def test_np_closest_point_single_triangles_against_f64():
    """The numpy twin of the reference's closest point on single triangles: the point is on the triangle and never nearer than the true
    closest point, on random triangles, slivers and at an offset of 1e4 (figures recorded under "single_triangles")."""
    from test_closest_cpu import np_closest_point

    fig = single_triangle_figures(np_closest_point)
    print(json.dumps(fig))
    want = json.load(open(GOLDEN))["single_triangles"]
    for name, f in fig.items():
        for k in ("k_on", "k_low"):
            assert f[k] <= want[name][k]["bound"], f"{name}: {k} = {f[k]:.4g}, recorded {want[name][k]}"


def single_triangle_figures(closest_point):
    """k_on, k_low, k_up (in u x the scale, the largest |p - vertex|) of a closest-point function on 20 000 single triangles per class."""
    out = {}
    for name, off, sliver in (("random", 0.0, False), ("slivers", 0.0, True), ("random at 1e4", 1e4, False)):
        rng = np.random.default_rng(21)
        p, a, b, c = (rng.uniform(-1, 1, (20000, 3)) + off for _ in range(4))
        if sliver:
            c = a + rng.uniform(0, 1, (20000, 1)) * (b - a) + 1e-6 * rng.normal(size=a.shape)
        p, a, b, c = (x.astype(F) for x in (p, a, b, c))
        cp = closest_point(p, a, b, c).astype(np.float64)
        P, A, B, C = (x.astype(np.float64) for x in (p, a, b, c))
        scale = U * np.sqrt(np.maximum(np.maximum(((P - A) ** 2).sum(1), ((P - B) ** 2).sum(1)), ((P - C) ** 2).sum(1)))
        on = g64.point_triangle(cp, A, B, C)[1]
        true = g64.point_triangle(P, A, B, C)[1]
        d = np.sqrt(((P - cp) ** 2).sum(1))
        out[name] = {"k_on": float((on / scale).max()), "k_low": float(((true - d) / scale).max()), "k_up": float(((d - true) / scale).max())}
    return out


if __name__ == "__main__":   # rewrite tests/golden/truth_error.json from the reference arithmetic
    from test_closest_cpu import np_closest_point

    doc = {"units": "k_*: u s, u = 2^-24, s = the largest |coordinate| among the point and the mesh's vertices; excess: the mesh's units",
           "closest": {}, "single_triangles": {}}
    for case, (_, well_shaped) in CLOSEST_CASES.items():
        doc["closest"][case] = record(*oracle_figures(case), well_shaped)
        print(case, doc["closest"][case])
    for case, f in single_triangle_figures(np_closest_point).items():
        doc["single_triangles"][case] = {"k_on": {"max": f["k_on"], "bound": bound_of(f["k_on"])}, "k_low": {"max": f["k_low"], "bound": bound_of(f["k_low"])},
                                         "k_up": {"max": f["k_up"]}}
    with open(GOLDEN, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
