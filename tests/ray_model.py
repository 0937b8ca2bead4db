"""Test oracle of the ray calls (include/m2s.h m2s_cast_rays): the header's contract restated in numpy float32, every operation rounded
on its own (numpy fuses nothing), sums left to right, all rays against all triangles in chunks.  Also the ray sets the CPU and GPU
tests share.
"""
import numpy as np

F = np.float32
NONE = np.uint32(0xFFFFFFFF)


def triangles_of(vertices, indices, topology=0):
    """[T, 3, 3] f32 corner positions in Topology order (0 = TriangleList, 1 = TriangleStrip as lib.rs:175-193 walks it)."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    idx = np.arange(v.shape[0], dtype=np.int64) if indices is None else np.asarray(indices).astype(np.int64).reshape(-1)
    if topology == 0:
        idx = idx[: idx.size // 3 * 3].reshape(-1, 3)
    else:
        n = max(idx.size - 2, 0)
        idx = np.stack([idx[0:n], idx[1:n + 1], idx[2:n + 2]], -1) if n else np.zeros((0, 3), np.int64)
    return v[idx]


def ray_setup(o, d):
    """o, d: [R, 3] f32.  Returns kx, ky, kz (int [R]), Sx, Sy, Sz (f32 [R]) and valid (bool [R])."""
    o, d = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
    ad = np.abs(d)
    kz = np.zeros(d.shape[0], np.int64)
    am = ad[:, 0].copy()
    for k in (1, 2):   # the lowest index on ties: only a strictly larger component takes over (a NaN never does)
        take = ad[:, k] > am
        kz[take] = k
        am[take] = ad[take, k]
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    rows = np.arange(d.shape[0])
    dz = d[rows, kz]
    swap = dz < 0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    with np.errstate(all="ignore"):
        Sx, Sy, Sz = d[rows, kx] / dz, d[rows, ky] / dz, F(1) / dz
    valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (am > 0)
    return kx, ky, kz, Sx.astype(F), Sy.astype(F), Sz.astype(F), valid


def _axis(v, k):
    """v [..., 3], k broadcastable to v[..., 0]: v[..., k]."""
    return np.take_along_axis(v, np.broadcast_to(k[..., None], v.shape[:-1] + (1,)), -1)[..., 0]


XY_REL = F(2.0 ** -20)   # ray.hip.h RAY_XY_REL
Z_REL = F(2.0 ** -21)    # ray.hip.h RAY_Z_REL


def _sheared(setup, o, p):
    """A point p as the test sees it from the ray: (Px, Py, Pz) f32."""
    kx, ky, kz, Sx, Sy, Sz = setup
    P = (p - o).astype(F)
    Pz = _axis(P, np.broadcast_to(kz, P.shape[:-1]))
    Px = (_axis(P, np.broadcast_to(kx, P.shape[:-1])) - (Sx * Pz).astype(F)).astype(F)
    Py = (_axis(P, np.broadcast_to(ky, P.shape[:-1])) - (Sy * Pz).astype(F)).astype(F)
    return Px, Py, (Sz * Pz).astype(F)


def line_test(setup, o, a, b, c, bare=False):
    """The triangle test without the range: o [R, 1, 3] (or [N, 3]) against a, b, c [1, T, 3] (or [N, 3]); setup entries shaped like
    o[..., 0].  Returns (meets, t, u, v); t, u, v are meaningful where `meets`.  bare: without the two bounding clauses (the paper's test)."""
    with np.errstate(all="ignore"):
        (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = (_sheared(setup, o, p) for p in (a, b, c))
        U = ((Cx * By).astype(F) - (Cy * Bx).astype(F)).astype(F)
        V = ((Ax * Cy).astype(F) - (Ay * Cx).astype(F)).astype(F)
        W = ((Bx * Ay).astype(F) - (By * Ax).astype(F)).astype(F)
        neg = (U < 0) | (V < 0) | (W < 0)
        pos = (U > 0) | (V > 0) | (W > 0)
        det = ((U + V).astype(F) + W).astype(F)
        meets = ~(neg & pos) & ((det < 0) | (det > 0))
        num = (((U * Az).astype(F) + (V * Bz).astype(F)).astype(F) + (W * Cz).astype(F)).astype(F)
        t, u, v = (num / det).astype(F), (V / det).astype(F), (W / det).astype(F)
        if not bare:   # (fmin / fmax skip a NaN as fminf / fmaxf do, and a NaN bound excludes nothing)
            xl, xh = np.fmin(np.fmin(Ax, Bx), Cx), np.fmax(np.fmax(Ax, Bx), Cx)
            yl, yh = np.fmin(np.fmin(Ay, By), Cy), np.fmax(np.fmax(Ay, By), Cy)
            mxy = (XY_REL * np.fmax(np.fmax(np.abs(xl), np.abs(xh)), np.fmax(np.abs(yl), np.abs(yh)))).astype(F)
            meets &= ~((xl > mxy) | (xh < -mxy) | (yl > mxy) | (yh < -mxy))
            zl, zh = np.fmin(np.fmin(Az, Bz), Cz), np.fmax(np.fmax(Az, Bz), Cz)
            mz = (Z_REL * np.fmax(np.abs(zl), np.abs(zh))).astype(F)
            meets &= ~((t < (zl - mz).astype(F)) | (t > (zh + mz).astype(F)))
    return meets, t, u, v


def box_accept(setup, o, lo, hi, t_min, limit):
    """rays.hip ray_box_accept: whether the walk descends into a node with the box [lo, hi] (shaped like o).  It must hold for every
    box that contains a triangle `line_test` reports in [t_min, limit]."""
    kx, ky, kz, Sx, Sy, Sz = setup
    with np.errstate(all="ignore"):
        L, H = (lo - o).astype(F), (hi - o).astype(F)
        k = np.broadcast_to(kz, L.shape[:-1])
        zl, zh = _axis(L, k), _axis(H, k)
        sx0, sx1, sy0, sy1 = (Sx * zl).astype(F), (Sx * zh).astype(F), (Sy * zl).astype(F), (Sy * zh).astype(F)
        z0, z1 = (Sz * zl).astype(F), (Sz * zh).astype(F)
        kxb, kyb = np.broadcast_to(kx, L.shape[:-1]), np.broadcast_to(ky, L.shape[:-1])
        Xlo, Xhi = (_axis(L, kxb) - np.fmax(sx0, sx1)).astype(F), (_axis(H, kxb) - np.fmin(sx0, sx1)).astype(F)
        Ylo, Yhi = (_axis(L, kyb) - np.fmax(sy0, sy1)).astype(F), (_axis(H, kyb) - np.fmin(sy0, sy1)).astype(F)
        Zlo, Zhi = np.fmin(z0, z1), np.fmax(z0, z1)
        mxy = (XY_REL * np.fmax(np.fmax(np.abs(Xlo), np.abs(Xhi)), np.fmax(np.abs(Ylo), np.abs(Yhi)))).astype(F)
        mz = (Z_REL * np.fmax(np.abs(Zlo), np.abs(Zhi))).astype(F)
        return (~(Xlo > mxy) & ~(Xhi < -mxy) & ~(Ylo > mxy) & ~(Yhi < -mxy) & ~((Zhi + mz).astype(F) < F(t_min))
                & ~((Zlo - mz).astype(F) > limit))


def cast(tris, origins, directions, t_min=0.0, t_max=np.inf, chunk=128, bare=False):
    """Every output of m2s_cast_rays for rays (origins, directions) [R, 3] against tris [T, 3, 3]: dict of t f32[R], triangle u32[R],
    uv f32[R, 2], count u32[R], occluded u8[R].  bare: the test without its bounding clauses (for comparison only)."""
    tris = np.asarray(tris, F).reshape(-1, 3, 3)
    o, d = np.ascontiguousarray(origins, F).reshape(-1, 3), np.ascontiguousarray(directions, F).reshape(-1, 3)
    R, T = o.shape[0], tris.shape[0]
    t_min, t_max = F(t_min), F(t_max)
    res = {"t": np.full(R, np.inf, F), "triangle": np.full(R, NONE, np.uint32), "uv": np.full((R, 2), np.nan, F),
           "count": np.zeros(R, np.uint32), "occluded": np.zeros(R, np.uint8)}
    if T == 0 or R == 0:
        return res
    kx, ky, kz, Sx, Sy, Sz, valid = ray_setup(o, d)
    a, b, c = tris[None, :, 0], tris[None, :, 1], tris[None, :, 2]
    for s in range(0, R, chunk):
        e = slice(s, min(s + chunk, R))
        setup = tuple(x[e, None] for x in (kx, ky, kz, Sx, Sy, Sz))
        meets, t, u, v = line_test(setup, o[e, None, :], a, b, c, bare)
        with np.errstate(invalid="ignore"):
            hit = meets & valid[e, None] & (t >= t_min) & (t <= t_max)
        cnt = hit.sum(1)
        tm = np.where(hit, t, np.inf).min(1)
        first = (hit & (t == tm[:, None])).argmax(1)   # the lowest index among the triangles that attain the smallest t
        rows = np.arange(hit.shape[0])
        any_hit = cnt > 0
        res["count"][e] = cnt
        res["occluded"][e] = any_hit
        res["t"][e] = np.where(any_hit, t[rows, first], np.inf)
        res["triangle"][e] = np.where(any_hit, first, NONE)
        res["uv"][e, 0] = np.where(any_hit, u[rows, first], np.nan)
        res["uv"][e, 1] = np.where(any_hit, v[rows, first], np.nan)
    return res


# ---- ray sets -----------------------------------------------------------------------------------------------------------------------
def radial_rays(vertices, indices, limit=4000):
    """Rays from outside through the mesh's vertices and edge midpoints, the hardest targets for a leaky test: o = c + 3 (target - c) with
    c the vertex mean, d = target - o, so the target sits at t = 1.  The first `limit` of [vertices, edge midpoints]."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    tri = np.asarray(indices).astype(np.int64).reshape(-1, 3)
    edges = np.unique(np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), 1), axis=0)
    mid = ((v[edges[:, 0]] + v[edges[:, 1]]).astype(F) * F(0.5)).astype(F)
    target = np.concatenate([v, mid])[:limit]
    c = v.mean(0).astype(F)
    o = (c + (F(3) * (target - c).astype(F)).astype(F)).astype(F)
    return o, (target - o).astype(F)


def box_rays(vertices, n, seed, spread=1.8):
    """Uniform random origins in `spread` x the mesh's box with random directions (not normalised)."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    mid, half = (v.max(0) + v.min(0)) * 0.5, (v.max(0) - v.min(0)) * 0.5
    o = (mid + half * spread * rng.uniform(-1, 1, (n, 3))).astype(F)
    return o, rng.normal(size=(n, 3)).astype(F)


def inside_rays(vertices, n, seed):
    """Origins near the vertex mean (inside a star-shaped mesh), random directions."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    c, half = v.mean(0), (v.max(0) - v.min(0)) * 0.5
    o = (c + half * 0.2 * rng.uniform(-1, 1, (n, 3))).astype(F)
    return o, rng.normal(size=(n, 3)).astype(F)


def axis_rays(vertices, n, seed):
    """Axis-parallel rays with exact zeros in two components, both signs, from outside the box; origins partly snapped onto vertex
    coordinates so that rays run exactly through vertices and along edges' planes."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0), v.max(0)
    o = (lo + (hi - lo) * rng.uniform(0, 1, (n, 3))).astype(F)
    snap = rng.integers(0, v.shape[0], n)
    o[: n // 2] = v[snap[: n // 2]]
    axis, sign = rng.integers(0, 3, n), rng.choice([-1.0, 1.0], n).astype(F)
    d = np.zeros((n, 3), F)
    rows = np.arange(n)
    d[rows, axis] = sign * rng.uniform(0.5, 2.0, n).astype(F)
    o[rows, axis] = np.where(sign > 0, lo[axis] - F(1), hi[axis] + F(1))
    return o, d
