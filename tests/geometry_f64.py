"""Float64 geometry the ray and closest-point results are checked against (tests/test_truth_cpu.py, tests/test_gpu_truth.py).

Plain numpy float64, all pairs, chunked.  It shares no code with ray_model.py, np_closest_point, the oracle or any .hip.h, and it is
written from the geometry, not from the contract's operation order: edge functions are scalar triple products, t comes from the
triangle's plane, closest points are a minimum over three segments and the plane projection (no region tests).  Inputs are f32 values
held in f64, so differences of coordinates are exact and every result here is good to ~1e-15 of the magnitudes involved, eight decimal
digits below anything the f32 code is asked for.
"""
import numpy as np

D = np.float64


# ---- rays ---------------------------------------------------------------------------------------------------------------------------
def ray_pairs(tris, o, d, chunk=256):
    """Every (ray, triangle) pair of rays (o, d) [R, 3] and triangles [T, 3, 3], as a dict of f64 arrays [R, T] (`e`: [R, T, 3]):
      e            the edge functions of the triangle's image in the plane across the ray (the coordinate plane of the ray's dominant
                   axis k, reached along the ray): e0 = d . (C x B) / |d_k| with A, B, C the vertices seen from the origin, e1 and e2
                   cyclically.  The ray's line meets the triangle iff they share a sign; zeros are its edges.
      det          e0 + e1 + e2 = -d . n / |d_k|, n = (b - a) x (c - a)
      t            the parameter at which the ray meets the triangle's plane, n . (a - o) / n . d (NaN for a ray in the plane)
      u, v         e1 / det, e2 / det: the meeting point is a + u (b - a) + v (c - a)
      L            the largest magnitude among the terms of the image's coordinates, |P[i]|, |P[j]|, |d_i / d_k P[k]|, |d_j / d_k P[k]|
                   over the three vertices P (i, j the other two axes): the scale rounding errors of the image come in
      zmin, zmax, zabs   least, greatest and greatest magnitude of the three vertices' parameters along the ray, P[k] / d_k
    and `valid` [R]: finite origin, finite non-zero direction.  Pairs of other rays hold NaN."""
    tris = np.asarray(tris, D).reshape(-1, 3, 3)
    o, d = np.asarray(o, D).reshape(-1, 3), np.asarray(d, D).reshape(-1, 3)
    R, T = o.shape[0], tris.shape[0]
    valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (np.abs(d).max(1, initial=0.0) > 0)
    out = {k: np.full((R, T), np.nan) for k in ("det", "t", "u", "v", "L", "zmin", "zmax", "zabs")}
    out["e"] = np.full((R, T, 3), np.nan)
    out["valid"] = valid
    n = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])   # [T, 3]
    rows = np.flatnonzero(valid)
    for s in range(0, rows.size, chunk):
        r = rows[s:s + chunk]
        oo, dd = o[r], d[r]
        k = np.abs(dd).argmax(1)
        i, j = (k + 1) % 3, (k + 2) % 3
        pick = np.arange(r.size)
        dk = dd[pick, k]
        P = tris[None] - oo[:, None, None, :]                         # [r, T, 3 vertices, 3]
        A, B, C = P[:, :, 0], P[:, :, 1], P[:, :, 2]
        dn = dd[:, None, :] / np.abs(dk)[:, None, None]
        e = np.stack([(dn * np.cross(C, B)).sum(-1), (dn * np.cross(A, C)).sum(-1), (dn * np.cross(B, A)).sum(-1)], -1)
        det = e.sum(-1)
        with np.errstate(all="ignore"):
            t = (n[None] * A).sum(-1) / (n[None] * dd[:, None, :]).sum(-1)
            u, v = e[..., 1] / det, e[..., 2] / det
        Pk = np.take_along_axis(P, np.broadcast_to(k[:, None, None, None], P.shape[:3] + (1,)), -1)[..., 0]   # [r, T, 3]
        Pi = np.take_along_axis(P, np.broadcast_to(i[:, None, None, None], P.shape[:3] + (1,)), -1)[..., 0]
        Pj = np.take_along_axis(P, np.broadcast_to(j[:, None, None, None], P.shape[:3] + (1,)), -1)[..., 0]
        si, sj = (dd[pick, i] / dk)[:, None, None], (dd[pick, j] / dk)[:, None, None]
        L = np.maximum(np.maximum(np.abs(Pi), np.abs(Pj)), np.maximum(np.abs(si * Pk), np.abs(sj * Pk))).max(-1)
        z = Pk / dk[:, None, None]
        out["e"][r], out["det"][r], out["t"][r], out["u"][r], out["v"][r], out["L"][r] = e, det, t, u, v, L
        out["zmin"][r], out["zmax"][r], out["zabs"][r] = z.min(-1), z.max(-1), np.abs(z).max(-1)
    return out


def classify(pairs, m):
    """(clear_hit, clear_miss) [R, T] for the margin m L^2: clear hit = all three edge functions beyond it on one side, clear miss = one
    beyond it on each side.  Everything else is ambiguous; pairs of invalid rays are neither (they are outside the comparison)."""
    e, lim = pairs["e"], m * pairs["L"] ** 2
    with np.errstate(invalid="ignore"):
        above, below = e > lim[..., None], e < -lim[..., None]
    return above.all(-1) | below.all(-1), above.any(-1) & below.any(-1)


def ray_bounds(pairs):
    """(tb, wb) [R, T]: the error granted to a reported t and to u, v of a clear hit.  werr = 2^-20 L^2 / |det| is the relative error of
    the normalised weights (2^-20 = 16 u of L^2 per edge function); t is their mean of the vertex parameters, so it
    moves by werr (zmax - zmin), plus 2^-21 max |z| for the roundings of the parameters and the sum; the factor 2 is the allowance."""
    with np.errstate(all="ignore"):
        werr = 2.0 ** -20 * pairs["L"] ** 2 / np.abs(pairs["det"])
        tb = 2.0 * (werr * (pairs["zmax"] - pairs["zmin"]) + 2.0 ** -21 * pairs["zabs"])
        wb = 2.0 * (werr + 2.0 ** -23)
    return tb, wb


def range_classes(pairs, tb, t_min, t_max):
    """(inside, outside) [R, T]: t lies inside [t_min, t_max] by more than tb / outside it by more than tb.  NaN is neither."""
    t = pairs["t"]
    with np.errstate(invalid="ignore"):
        inside = (t - t_min > tb) & (t_max - t > tb)
        outside = (t_min - t > tb) | (t - t_max > tb)
    return inside, outside


def solid_angle_winding(tris, p, chunk=512):
    """Winding number of the triangles around the points p [N, 3] (van Oosterom and Strackee), f64 [N]."""
    tris, p = np.asarray(tris, D).reshape(-1, 3, 3), np.asarray(p, D).reshape(-1, 3)
    w = np.zeros(p.shape[0])
    for s in range(0, p.shape[0], chunk):
        P = tris[None] - p[s:s + chunk, None, None, :]
        A, B, C = P[:, :, 0], P[:, :, 1], P[:, :, 2]
        la, lb, lc = (np.sqrt((X * X).sum(-1)) for X in (A, B, C))
        num = (A * np.cross(B, C)).sum(-1)
        den = la * lb * lc + (A * B).sum(-1) * lc + (B * C).sum(-1) * la + (C * A).sum(-1) * lb
        w[s:s + chunk] = np.arctan2(num, den).sum(1) / (2 * np.pi)
    return w


# ---- closest points -------------------------------------------------------------------------------------------------------------------
def _segment(p, a, b):
    ab = b - a
    m = (ab * ab).sum(-1)
    with np.errstate(all="ignore"):
        s = np.where(m > 0, ((p - a) * ab).sum(-1) / m, 0.0)
    q = a + ab * np.clip(s, 0.0, 1.0)[..., None]
    return q, ((p - q) ** 2).sum(-1)


def point_triangle(p, a, b, c):
    """Closest point on the triangle (a, b, c) to p and its distance, all [N, 3] f64 -> ([N, 3], [N]): the minimum over the three edges
    as segments and the foot of the perpendicular on the plane where that lies in the triangle.  A degenerate triangle has no usable plane
    and is served by its segments."""
    p, a, b, c = (np.asarray(x, D).reshape(-1, 3) for x in (p, a, b, c))
    q, d2 = _segment(p, a, b)
    for x, y in ((b, c), (c, a)):
        q2, e2 = _segment(p, x, y)
        take = e2 < d2
        q, d2 = np.where(take[:, None], q2, q), np.where(take, e2, d2)
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    with np.errstate(all="ignore"):
        h = ((p - a) * n).sum(-1) / nn
        f = p - h[:, None] * n
        w0 = (n * np.cross(c - b, f - b)).sum(-1)
        w1 = (n * np.cross(a - c, f - c)).sum(-1)
        w2 = (n * np.cross(b - a, f - a)).sum(-1)
        inside = (nn > 0) & (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
        f2 = h * h * nn
    take = inside & (f2 < d2)
    q, d2 = np.where(take[:, None], f, q), np.where(take, f2, d2)
    return q, np.sqrt(d2)


def mesh_distance(p, tris, tol=0.0, chunk=256):
    """Distance of every point p [N, 3] to the mesh tris [T, 3, 3], f64 [N], and the pairs (point index, triangle index) of the triangles
    within tol (a scalar or [N]) of it.  All pairs, except that a triangle is not evaluated for a point when its bounding sphere alone puts it
    farther away than the point's nearest vertex by more than tol."""
    p, tris = np.asarray(p, D).reshape(-1, 3), np.asarray(tris, D).reshape(-1, 3, 3)
    N = p.shape[0]
    tol = np.broadcast_to(np.asarray(tol, D), (N,))
    centre = tris.mean(1)
    radius = np.sqrt(((tris - centre[:, None]) ** 2).sum(-1)).max(1) * (1 + 1e-12)
    dist = np.full(N, np.inf)
    near_p, near_t = [], []
    # the cull only: distances to the sphere centres by |q|^2 + |c|^2 - 2 q . c about the mesh's middle, whose cancellation (below
    # 1e-7 of the extent in the distance) the slack covers ten times over
    middle = centre.mean(0)
    cc = centre - middle
    cc2 = (cc * cc).sum(1)
    for s in range(0, N, chunk):
        q = p[s:s + chunk]
        qc = q - middle
        to_centre = np.sqrt(np.maximum((qc * qc).sum(1)[:, None] + cc2[None] - 2.0 * (qc @ cc.T), 0.0))
        slack = 1e-6 * (np.abs(qc).max() + np.abs(cc).max())
        lower, upper = to_centre - radius[None] - slack, (to_centre + radius[None]).min(1) + slack
        pi, ti = np.nonzero(lower <= (upper + tol[s:s + chunk])[:, None] * (1 + 1e-12))
        _, dd = point_triangle(q[pi], tris[ti, 0], tris[ti, 1], tris[ti, 2])
        best = np.full(q.shape[0], np.inf)
        np.minimum.at(best, pi, dd)
        dist[s:s + chunk] = best
        keep = dd <= best[pi] + tol[s:s + chunk][pi]
        near_p.append(pi[keep] + s)
        near_t.append(ti[keep])
    return dist, (np.concatenate(near_p) if near_p else np.zeros(0, np.int64), np.concatenate(near_t) if near_t else np.zeros(0, np.int64))
