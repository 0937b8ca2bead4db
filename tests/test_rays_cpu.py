"""Ray casting without a GPU: properties of the numpy model of the contract (tests/ray_model.py), the host build of csrc/ray.hip.h against
that model bit for bit, the exports, and the argument checks that happen before any device work."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_model as rm  # noqa: E402
from mesh_to_sdf_amd import M2SPanic, Topology, _lib, cast_rays, meshes  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(os.path.dirname(_lib.SO_PATH), "libm2s_probe.so")
INF = float("inf")


def _bits(x):
    return np.asarray(x, F).view(np.uint32)


# ---- the model itself -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slices, stacks", [(12, 9), (48, 65)])
def test_model_is_watertight_on_radial_rays(slices, stacks):
    """Rays from outside at vertices and edge midpoints of a closed mesh: every one hits, and none slips through the front face (the
    first hit is not beyond the target at t = 1; Moeller-Trumbore in f32 fails both on these meshes)."""
    v, idx = meshes.blob(slices, stacks)
    o, d = rm.radial_rays(v, idx, 4000)
    r = rm.cast(rm.triangles_of(v, idx), o, d)
    assert o.shape[0] == min(4000, v.shape[0] + 3 * idx.size // 6)
    assert (r["count"] > 0).all()
    assert r["t"].max() <= 1.001
    assert (r["triangle"] < idx.size // 3).all() and np.isfinite(r["uv"]).all()


def test_model_hits_the_shared_edge_of_a_cube_face():
    v, idx = meshes.cube()
    tris = rm.triangles_of(v, idx)
    # the +z face is the quad (1, 5, 7, 3) cut along 1-7: (-1, -1, 1) .. (1, 1, 1).  Rays straight down onto points of that diagonal
    s = np.array([-0.75, -0.5, 0.0, 0.25, 0.625], F)
    o = np.stack([s, s, np.full_like(s, 3)], -1)
    d = np.tile(np.array([0, 0, -1], F), (s.size, 1))
    r = rm.cast(tris, o, d)
    assert (r["t"] == 2).all()
    assert (r["count"] == 4).all()               # both triangles of the +z face and both of the -z face: an edge hit counts each
    assert (r["triangle"] == 10).all()           # the lower index of the two that tie at t = 2
    first = rm.cast(tris, o, d, 0.0, 3.0)
    assert (first["count"] == 2).all()


def test_model_swapping_b_and_c_keeps_the_hit_and_t_up_to_rounding():
    """The hit decision is the same bit for bit; t is summed in another order (det and the numerator), so it agrees only to rounding."""
    rng = np.random.default_rng(5)
    o, d, a, b, c = (rng.uniform(-2, 2, (3000, 3)).astype(F) for _ in range(5))
    o *= 3
    d = (a + b + c) / 3 - o + rng.normal(size=o.shape).astype(F) * 0.3
    kx, ky, kz, Sx, Sy, Sz, valid = rm.ray_setup(o, d)
    m1, t1, u1, v1 = rm.line_test((kx, ky, kz, Sx, Sy, Sz), o, a, b, c)
    m2, t2, u2, v2 = rm.line_test((kx, ky, kz, Sx, Sy, Sz), o, a, c, b)
    assert (m1 == m2).all() and m1.sum() > 300
    close = np.abs(t1[m1] - t2[m1]) <= 1e-5 * np.maximum(np.abs(t1[m1]), 1)   # det and the numerator are summed in another order
    assert close.all()


def test_model_degenerate_triangles_and_bad_rays_never_hit():
    rng = np.random.default_rng(6)
    n = 4000
    o, a, c = (rng.uniform(-2, 2, (n, 3)).astype(F) for _ in range(3))
    for b2, c2 in ((a, c), (c, c), (c, a), (a, a)):   # a == b, b == c, c == a, a point
        d = ((a + c2) * F(0.5) - o).astype(F)          # aimed at the segment: the hardest case
        setup = rm.ray_setup(o, d)
        meets, *_ = rm.line_test(setup[:6], o, a, b2, c2)
        assert not meets.any()
    v, idx = meshes.cube()
    tris = rm.triangles_of(v, idx)
    o = np.array([[0, 0, 3]] * 6, F)
    d = np.array([[0, 0, 0], [np.nan, 0, -1], [0, 0, -np.inf], [0, 0, -1], [0, 0, -1], [0, 0, -1]], F)
    o[3, 1] = np.nan
    o[4, 0] = np.inf
    r = rm.cast(tris, o, d)
    assert r["count"].tolist() == [0, 0, 0, 0, 0, 4]
    assert np.isinf(r["t"][:5]).all() and (r["triangle"][:5] == rm.NONE).all() and np.isnan(r["uv"][:5]).all()
    assert r["occluded"].tolist() == [0, 0, 0, 0, 0, 1]


def test_model_range_ends_are_inclusive():
    v, idx = meshes.cube()
    tris = rm.triangles_of(v, idx)
    o, d = np.array([[0.25, 0.5, 3]], F), np.array([[0, 0, -1]], F)     # hits z = 1 at t = 2 and z = -1 at t = 4
    assert rm.cast(tris, o, d)["count"][0] == 2
    assert rm.cast(tris, o, d, 2.0, 4.0)["count"][0] == 2
    assert rm.cast(tris, o, d, np.nextafter(F(2), F(3)), 4.0)["t"][0] == 4
    assert rm.cast(tris, o, d, 2.0, np.nextafter(F(4), F(0)))["count"][0] == 1
    assert rm.cast(tris, o, d, np.nextafter(F(2), F(3)), np.nextafter(F(4), F(0)))["occluded"][0] == 0
    assert rm.cast(tris, o, d, 4.0, 4.0)["t"][0] == 4
    half = rm.cast(tris, o, (d * F(0.5)).astype(F))                      # t is in units of |d|
    assert half["t"][0] == 4 and half["count"][0] == 2


# ---- the bounding clauses and the walk's box test ---------------------------------------------------------------------------------------
def _mixed_rays(v, idx, seed, n):
    parts = [rm.radial_rays(v, idx, n), rm.box_rays(v, n, seed), rm.inside_rays(v, n // 2, seed + 1), rm.axis_rays(v, n // 2, seed + 2)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def test_bounding_clauses_change_nothing_off_degenerate_images_and_decide_those():
    """On a closed mesh under radial, random, inner and axis rays the definition equals the paper's bare test in every bit.  On triangles
    strung along a blob's meridians (its index list read as a strip) the radial rays lie in the triangles' planes: there the bare test
    reports rounding-noise hits far from the triangles, and the clauses remove them."""
    v, idx = meshes.blob(12, 9)
    o, d = _mixed_rays(v, idx, 40, 400)
    tris = rm.triangles_of(v, idx)
    full, bare = rm.cast(tris, o, d), rm.cast(tris, o, d, bare=True)
    for k in full:
        assert np.array_equal(full[k].view(np.uint32) if full[k].dtype == F else full[k], bare[k].view(np.uint32) if bare[k].dtype == F else bare[k]), k
    v, idx = meshes.blob(16, 17)
    o, d = rm.radial_rays(v, idx, 300)
    strip = rm.triangles_of(v, idx, 1)
    full, bare = rm.cast(strip, o, d), rm.cast(strip, o, d, bare=True)
    assert (bare["count"] >= full["count"]).all() and (bare["count"] > full["count"]).any()
    assert (full["count"] > 0).all()   # the strip still holds every triangle of the list: no ray gets through


@pytest.mark.parametrize("shift, scale", [(0.0, 1.0), (1.0e4, 1.0), (0.0, 1.0e-15)])
def test_box_test_is_conservative_against_the_model(shift, scale):
    """rays.hip ray_box_accept, restated in ray_model.box_accept: every box that contains a triangle the definition reports in range is
    accepted — for boxes of 1, 2, 8 and 64 triangles and of the whole mesh, bare min / max boxes and ones padded by 1e-4, over the
    whole range and against the hit's own t as the limit (the first-hit walk's pruning must keep ties).  Edge-on strips included; far
    coordinates (the padding is below an ulp) and tiny ones (products underflow) too."""
    v, idx = meshes.blob(16, 17)
    v = ((v + F(shift)).astype(F) * F(scale)).astype(F)
    o, d = _mixed_rays(v, idx, 50, 250)
    kx, ky, kz, Sx, Sy, Sz, valid = rm.ray_setup(o, d)
    assert valid.all()
    setup = tuple(x[:, None] for x in (kx, ky, kz, Sx, Sy, Sz))
    n_hits = 0
    for topology in (0, 1):
        tris = rm.triangles_of(v, idx, topology)
        tris = tris[np.argsort(tris.mean(1)[:, 0], kind="stable")]   # neighbours in x share a box, as sorted triangles share a leaf
        meets, t, _, _ = rm.line_test(setup, o[:, None, :], tris[None, :, 0], tris[None, :, 1], tris[None, :, 2])
        for t_min, t_max in ((0.0, INF), (0.9, 1.6)):
            with np.errstate(invalid="ignore"):
                hit = meets & (t >= F(t_min)) & (t <= F(t_max))
            n_hits += int(hit.sum())
            for group in (1, 2, 8, 64, tris.shape[0]):
                starts = np.arange(0, tris.shape[0], group)
                lo = np.minimum.reduceat(tris.min(1), starts)
                hi = np.maximum.reduceat(tris.max(1), starts)
                any_hit = np.logical_or.reduceat(hit, starts, axis=1)
                t_first = np.minimum.reduceat(np.where(hit, t, np.inf), starts, axis=1)
                for pad in (F(0), F(1.0e-4)):
                    L, H = (lo - pad).astype(F)[None], (hi + pad).astype(F)[None]
                    for limit in (F(t_max), t_first):
                        ok = rm.box_accept(setup, o[:, None, :], L, H, t_min, limit)
                        assert ok[any_hit].all(), (topology, t_min, group, float(pad))
    assert n_hits > 1000


# ---- the host build of ray.hip.h against the model -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        _lib.build()
    L = C.CDLL(PROBE)
    L.probe_ray_setup.restype = C.c_int
    L.probe_ray_setup.argtypes = [C.c_void_p] * 4
    L.probe_ray_triangle.restype = C.c_int
    L.probe_ray_triangle.argtypes = [C.c_void_p] * 5 + [C.c_float, C.c_float, C.c_void_p]
    return L


def _probe_cases(n, seed):
    """(o, d, a, b, c) [n, 3] each: random, with the degenerate patterns of test_device_math_host._cases, directions with one and two zero
    components, negative dominant axes, ties of |d_k|, rays aimed at vertices, edges and interiors, rays in the triangle's plane, and bad rays."""
    rng = np.random.default_rng(seed)
    o, a, b, c = (rng.uniform(-10, 10, (n, 3)).astype(F) for _ in range(4))
    w = rng.dirichlet([1, 1, 1], n).astype(F)
    aim = rng.integers(0, 4, n)
    w[aim == 1, 2] = 0            # at the edge ab
    w[aim == 2] = [1, 0, 0]       # at the vertex a
    target = (w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c).astype(F)
    target[aim == 3] = rng.uniform(-10, 10, ((aim == 3).sum(), 3)).astype(F)
    d = ((target - o) * rng.uniform(0.2, 3.0, (n, 1)).astype(F)).astype(F)
    i = np.arange(n)
    k = i % 16
    # rays in the triangle's plane, from and towards points of it far outside the triangle: edge-on, where the bounding clauses decide
    w1, w2 = rng.uniform(-3, 3, (n, 2)).astype(F), rng.uniform(-3, 3, (n, 2)).astype(F)
    p1 = (a + w1[:, :1] * (b - a) + w1[:, 1:] * (c - a)).astype(F)
    p2 = (a + w2[:, :1] * (b - a) + w2[:, 1:] * (c - a)).astype(F)
    o[k == 5], d[k == 5] = p1[k == 5], (p2 - p1).astype(F)[k == 5]
    b[k == 6] = a[k == 6]
    c[k == 7] = b[k == 7]
    c[k == 8] = a[k == 8]
    b[k == 9] = a[k == 9]
    c[k == 9] = a[k == 9]
    for kk, zero in ((10, (0,)), (11, (1,)), (12, (2,)), (13, (0, 1)), (14, (1, 2)), (15, (0, 2))):
        for z in zero:
            d[k == kk, z] = 0
            o[k == kk, z] = target[k == kk, z]      # still aimed at the target where that is possible
    tie = (i % 97) == 0
    d[tie, 1] = -d[tie, 0]        # |d_x| == |d_y|: the lowest index wins
    tie3 = (i % 193) == 0
    d[tie3] = np.abs(d[tie3, :1]) * np.array([-1, 1, -1], F)
    bad = (i % 211) == 0
    d[bad] = 0
    d[(i % 223) == 0, 2] = np.nan
    o[(i % 227) == 0, 0] = np.inf
    return [np.ascontiguousarray(x) for x in (o, d, a, b, c)]


def test_host_build_matches_the_model_bit_for_bit(probe):
    n = 6000
    o, d, a, b, c = _probe_cases(n, 11)
    kx, ky, kz, Sx, Sy, Sz, valid = rm.ray_setup(o, d)
    meets, t, u, v = rm.line_test((kx, ky, kz, Sx, Sy, Sz), o, a, b, c)
    assert (d[valid, :][np.arange(valid.sum()), kz[valid]] < 0).sum() > n // 4          # negative dominant axes are well represented
    assert (meets & valid).sum() > n // 8 and (~meets & valid).sum() > n // 8
    bare = rm.line_test((kx, ky, kz, Sx, Sy, Sz), o, a, b, c, bare=True)[0]
    assert (bare & ~meets & valid).sum() >= 10                                            # cases that only the bounding clauses reject
    ranges = ((0.0, INF), (0.5, 1.5))
    for i in range(n):
        k3, s3 = np.zeros(3, np.int32), np.zeros(3, F)
        ok = probe.probe_ray_setup(o[i].ctypes.data, d[i].ctypes.data, k3.ctypes.data, s3.ctypes.data)
        assert bool(ok) == bool(valid[i]), i
        if not valid[i]:
            for lo, hi in ranges:
                tuv = np.zeros(3, F)
                assert probe.probe_ray_triangle(o[i].ctypes.data, d[i].ctypes.data, a[i].ctypes.data, b[i].ctypes.data, c[i].ctypes.data, lo, hi,
                                                tuv.ctypes.data) == 0
            continue
        assert k3.tolist() == [kx[i], ky[i], kz[i]], i
        assert _bits(s3).tolist() == _bits([Sx[i], Sy[i], Sz[i]]).tolist(), i
        for lo, hi in ranges:
            tuv = np.full(3, np.nan, F)
            hit = probe.probe_ray_triangle(o[i].ctypes.data, d[i].ctypes.data, a[i].ctypes.data, b[i].ctypes.data, c[i].ctypes.data, lo, hi,
                                           tuv.ctypes.data)
            with np.errstate(invalid="ignore"):
                want = bool(meets[i] and t[i] >= F(lo) and t[i] <= F(hi))
            assert bool(hit) == want, i
            if meets[i]:
                assert _bits(tuv).tolist() == _bits([t[i], u[i], v[i]]).tolist(), i


# ---- the library: exports and argument checks that need no device ------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


def test_new_entry_points_are_exported(lib):
    for name in ("m2s_cast_rays", "m2s_mesh_cast_rays"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    hdr = open(os.path.join(ROOT, "include", "m2s.h")).read()
    assert "typedef struct m2s_ray_opts" in hdr
    assert "#define M2S_VERSION_MINOR 5" in hdr
    assert C.sizeof(_lib.M2SRayOpts) == 12


def _opts(**kw):
    o = _lib.M2SOpts()
    o.struct_size = C.sizeof(_lib.M2SOpts)
    o.device = -1
    o.synchronous = 1
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_bad_arguments_fail_before_the_device(lib):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    idx = np.array([0, 1, 2, 0, 2, 3], np.uint32)
    org, dirs = np.zeros((4, 3), F), np.ones((4, 3), F)
    t, tri, uv, cnt, occ = np.zeros(4, F), np.zeros(4, np.uint32), np.zeros(8, F), np.zeros(4, np.uint32), np.zeros(4, np.uint8)
    V, I, O, D = v.ctypes.data, idx.ctypes.data, org.ctypes.data, dirs.ctypes.data
    outs = [x.ctypes.data for x in (t, tri, uv, cnt, occ)]
    BAD = _lib.ERR_BAD_ARG
    cr = lib.m2s_cast_rays
    assert cr(V, 4, I, 6, 4, 0, O, D, 4, None, None, None, None, None, None, None) == BAD          # every output NULL
    assert "NULL" in _lib.last_error()
    assert cr(V, 4, I, 6, 4, 0, None, D, 4, None, *outs, None) == BAD                              # NULL origins, n > 0
    assert cr(V, 4, I, 6, 4, 0, O, None, 4, None, *outs, None) == BAD                              # NULL directions, n > 0
    assert cr(V, 4, I, 6, 3, 0, O, D, 4, None, *outs, None) == BAD                                 # index_bytes
    assert cr(V, 4, I, 6, 4, 7, O, D, 4, None, *outs, None) == BAD                                 # topology
    assert cr(None, 4, I, 6, 4, 0, O, D, 4, None, *outs, None) == BAD                              # NULL vertices
    bad_idx = np.array([0, 1, 2, 0, 2, 4], np.uint32)
    assert cr(V, 4, bad_idx.ctypes.data, 6, 4, 0, O, D, 4, None, *outs, None) == BAD               # vertex index out of range
    assert "out of range" in _lib.last_error()
    assert cr(V, 4, bad_idx.ctypes.data, 6, 4, 1, O, D, 0, None, *outs, None) == BAD               # ... also with no rays, and as a strip
    for lo, hi in ((1.0, 0.5), (float("nan"), 1.0), (0.0, float("nan")), (INF, 0.0)):
        ro = _lib.M2SRayOpts(C.sizeof(_lib.M2SRayOpts), lo, hi)
        assert cr(V, 4, I, 6, 4, 0, O, D, 4, C.byref(ro), *outs, None) == BAD, (lo, hi)
        assert "t_min" in _lib.last_error()
        assert lib.m2s_mesh_cast_rays(None, O, D, 4, C.byref(ro), *outs, None) == BAD
    ro = _lib.M2SRayOpts(4, 0.0, 1.0)
    assert cr(V, 4, I, 6, 4, 0, O, D, 4, C.byref(ro), *outs, None) == BAD                          # struct_size
    for field, value in (("x_begin", 1), ("x_end", 2), ("x_period", 4), ("n_peer_out", 1), ("mem_kind", 5), ("algorithm", 2)):
        assert cr(V, 4, I, 6, 4, 0, O, D, 4, None, *outs, C.byref(_opts(**{field: value}))) == BAD, field
    assert cr(V, 4, I, 6, 4, 0, O, D, 0, None, *outs, None) == _lib.M2S_OK                         # no rays: nothing to do, no device needed
    assert cr(V, 4, I, 6, 4, 0, None, None, 0, None, *outs, None) == _lib.M2S_OK
    assert cr(V, 4, I, 6, 4, 0, None, None, 0, None, None, None, None, None, None, None) == _lib.M2S_OK   # ... nor any output
    h = cast_rays(v, Topology.TriangleList(idx), np.zeros((0, 3), F), np.zeros((0, 3), F))
    assert h.t.shape == (0,) and h.triangle.shape == (0,) and h.uv.shape == (0, 2)
    assert lib.m2s_mesh_cast_rays(None, O, D, 4, None, *outs, None) == BAD                         # NULL mesh
    with pytest.raises(M2SPanic):
        cast_rays(v, Topology.TriangleList(idx), org, dirs, t_min=2.0, t_max=1.0)
    with pytest.raises(M2SPanic):
        cast_rays(v, Topology.TriangleList(idx), org, dirs[:3])
