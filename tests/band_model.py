"""numpy restatement of the candidate predicate of m2s_narrow_band_sdf (mesh_to_sdf_amd/csrc/band.hip.h): which cells of a grid lie within
reach of some triangle's box.  IEEE binary32 throughout, sums left to right, as the header fixes them.  The model states the predicate per
cell; the library reaches the same set through per-axis and per-column interval searches."""
import numpy as np

F = np.float32
BAND_REL = F(4.0e-6)


def centres(first, size, n):
    return (F(first) + np.arange(n, dtype=np.uint32).astype(F) * F(size)).astype(F)


def grid_scale(first, size, count):
    """Largest |coordinate| of any cell centre."""
    return F(max(abs(float(centres(first[m], size[m], count[m])[e])) for m in range(3) for e in (0, -1)))


def box(tri):
    """(lo[3], hi[3], amax, any) over the vertices of `tri` (3 x 3) whose three coordinates are all finite."""
    tri = np.asarray(tri, F).reshape(3, 3)
    ok = np.isfinite(tri).all(axis=1)
    if not ok.any():
        return np.zeros(3, F), np.zeros(3, F), F(0), False
    p = tri[ok]
    return p.min(axis=0), p.max(axis=0), F(np.abs(p).max()), True


def reach(r, scale):
    with np.errstate(over="ignore"):
        grown = F(r) * (F(1.0) + BAND_REL)
        return F(grown + BAND_REL * F(scale))


def plane(tri, rch, first, size, count):
    """(a, n, rhs, use) of the plane test: a cell is dropped for the triangle when |(n.x w.x + n.y w.y) + n.z w.z| > rhs, w = q - a."""
    a, b, c = np.asarray(tri, F).reshape(3, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        e0, e1 = (b - a).astype(F), (c - a).astype(F)
        n = np.array([F(e0[1] * e1[2]) - F(e0[2] * e1[1]), F(e0[2] * e1[0]) - F(e0[0] * e1[2]), F(e0[0] * e1[1]) - F(e0[1] * e1[0])], F)
        dot = lambda x, y: F(F(F(x[0] * y[0]) + F(x[1] * y[1])) + F(x[2] * y[2]))        # noqa: E731
        nlen, E = np.sqrt(dot(n, n)), F(np.sqrt(dot(e0, e0)) * np.sqrt(dot(e1, e1)))
        W = F(0)
        for m in range(3):
            q = centres(first[m], size[m], count[m])
            W = F(W + max(abs(F(q[0] - a[m])), abs(F(q[-1] - a[m]))))
        rhs = F(F(F(rch) * F(nlen + F(F(2.0 ** -20) * E))) + F(F(2.0 ** -19) * F(E * W)))
    return a, n, rhs, bool(np.isfinite(tri).all() and dot(n, n) >= F(1.0e-30))


def gap(lo, hi, q):
    with np.errstate(invalid="ignore", over="ignore"):
        below, above = (F(lo) - q).astype(F), (q - F(hi)).astype(F)
        g = np.zeros_like(q)
        g = np.where(below > g, below, g)
        return np.where(above > g, above, g).astype(F)


def candidates(tris, first, size, count, r):
    """uint8[nx, ny, nz]: 1 where, for some triangle, (gx*gx + gy*gy) + gz*gz <= reach * reach and the plane test does not drop the cell."""
    first, size = np.asarray(first, F), np.asarray(size, F)
    occ = np.zeros(count, bool)
    if np.isinf(r):
        return np.ones(count, np.uint8)
    gs = grid_scale(first, size, count)
    q = [centres(first[m], size[m], count[m]) for m in range(3)]
    for tri in np.asarray(tris, F).reshape(-1, 3, 3):
        lo, hi, amax, any_ = box(tri)
        if not any_:
            continue
        rch = reach(r, max(amax, gs))
        a, n, rhs, use = plane(tri, rch, first, size, count)
        with np.errstate(over="ignore", invalid="ignore"):
            r2 = F(rch * rch)
            gx, gy, gz = (gap(lo[m], hi[m], q[m]) for m in range(3))
            s = ((gx * gx)[:, None] + (gy * gy)[None, :]).astype(F)
            near = (s[:, :, None] + (gz * gz)[None, None, :]).astype(F) <= r2
            if use:
                w = [(q[m] - a[m]).astype(F) for m in range(3)]
                sxy = ((n[0] * w[0])[:, None] + (n[1] * w[1])[None, :]).astype(F)
                t = (sxy[:, :, None] + (n[2] * w[2])[None, None, :]).astype(F)
                near &= ~((t > rhs) | (t < -rhs))
            occ |= near
    return occ.astype(np.uint8)
