"""Test oracle of the grid queries (include/m2s.h m2s_sample_grid / m2s_raymarch_grid): the reference client's shader
mesh_to_sdf_client/shaders/draw_raymarching.wgsl restated in numpy float32, vectorised over points and rays.  Every expression is
one correctly rounded f32 operation in the shader's order (numpy never fuses), so the GPU results must equal these bit for bit.

`d` is anything indexable by an int64 array of cell offsets (z + y*nz + x*ny*nz): the grid's flat float32 distances, or an object
that computes them (the 4 GiB test grid)."""
import numpy as np

F = np.float32
QNAN = np.array([0x7FC00000], np.uint32).view(F)[0]   # what a NaN input produces (grid_query.hip kQNaN)
SNAP, TRILINEAR, TETRAHEDRAL = 0, 1, 2                # MODE_* (:43-45)


class GridQ:
    """The shader's uniforms (sdf.rs:74-81): start = first_cell, end = get_last_cell (grid.rs:82-88), cell_size, cell_count."""

    def __init__(self, first_cell, cell_size, cell_count):
        self.start = np.array(first_cell, F)
        self.cs = np.array(cell_size, F)
        self.n = np.array(cell_count, np.int64)
        self.end = (self.start + self.n.astype(F) * self.cs).astype(F)
        self.eps = F(0.01) * max(self.cs[0], max(self.cs[1], self.cs[2]))   # EPSILON * max(..) (:203, :255-257)

    @classmethod
    def of(cls, grid):
        return cls(grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count())


def cell_off(q, ix, iy, iz):
    """get_distance (:92-99) without the read: indices clamped to [0, count - 1]."""
    x, y, z = (np.clip(i, 0, q.n[k] - 1) for k, i in enumerate((ix, iy, iz)))
    return z + y * q.n[2] + x * q.n[1] * q.n[2]


def _state(q, p):
    nan = np.isnan(p).any(1)
    out = (p < q.start).any(1) | (p > q.end).any(1)   # :121
    return np.where(nan, 2, np.where(out, 1, 0))


def tetra_cases(fx, fy, fz):
    """compute_tetrahedral_barycenter (:585-640), (r, g, b) = (x, y, z): the six cases in order, the last match wins.
    -> (bary0..3, vert2 bits, vert3 bits, case number 1..6) with bits x = 1, y = 2, z = 4."""
    z = np.zeros_like(fx)
    b0, b1, b2, b3 = z.copy(), z.copy(), z.copy(), z.copy()
    v2, v3, case = (np.zeros(fx.shape, np.int64) for _ in range(3))
    one = F(1)
    for c, (m, bary, a, b) in enumerate([
        ((fy >= fz) & (fz >= fx), (one - fy, fy - fz, fz - fx, fx), 2, 6),
        ((fz > fx) & (fx > fy), (one - fz, fz - fx, fx - fy, fy), 4, 5),
        ((fz > fy) & (fy >= fx), (one - fz, fz - fy, fy - fx, fx), 4, 6),
        ((fx >= fy) & (fy > fz), (one - fx, fx - fy, fy - fz, fz), 1, 3),
        ((fy > fx) & (fx >= fz), (one - fy, fy - fx, fx - fz, fz), 2, 3),
        ((fx >= fz) & (fz >= fy), (one - fx, fx - fz, fz - fy, fy), 1, 5),
    ], start=1):
        b0, b1, b2, b3 = (np.where(m, new, old) for new, old in zip(bary, (b0, b1, b2, b3)))
        v2, v3, case = np.where(m, a, v2), np.where(m, b, v3), np.where(m, c, case)
    return (b0, b1, b2, b3), v2, v3, case


def sample(q, d, p, mode=TRILINEAR, iso=0.0, outside=100.0):
    """sdf_grid (:118-200) at the points p (n, 3); NaN for a NaN coordinate."""
    p = np.asarray(p, F).reshape(-1, 3)
    iso, outside = F(iso), F(outside)
    st = _state(q, p)
    pp = np.where((st != 0)[:, None], q.start, p).astype(F)   # rows that are not read
    with np.errstate(all="ignore"):
        if mode == SNAP:
            g = q.start - q.cs * F(0.5)                              # :130
            idx = np.floor((pp - g) / q.cs).astype(np.int64)         # :133
            val = d[cell_off(q, idx[:, 0], idx[:, 1], idx[:, 2])] - iso
        else:
            c = (pp - q.start) / q.cs                                # :159 / :181
            fl = np.floor(c)
            f = c - fl                                               # fract
            i = fl.astype(np.int64)
            fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]

            def g(dx, dy, dz):
                return d[cell_off(q, i[:, 0] + dx, i[:, 1] + dy, i[:, 2] + dz)] - iso

            if mode == TRILINEAR:                                    # :164-172
                ox, oy, oz = F(1) - fx, F(1) - fy, F(1) - fz
                c_x00 = g(0, 0, 0) * ox + g(1, 0, 0) * fx
                c_x01 = g(0, 0, 1) * ox + g(1, 0, 1) * fx
                c_x10 = g(0, 1, 0) * ox + g(1, 1, 0) * fx
                c_x11 = g(0, 1, 1) * ox + g(1, 1, 1) * fx
                c_xy0 = c_x00 * oy + c_x10 * fy
                c_xy1 = c_x01 * oy + c_x11 * fy
                val = c_xy0 * oz + c_xy1 * fz
            else:                                                    # :181-196
                (b0, b1, b2, b3), v2, v3, _ = tetra_cases(fx, fy, fz)
                s0 = g(0, 0, 0)
                s1 = g(v2 & 1, (v2 >> 1) & 1, v2 >> 2)
                s2 = g(v3 & 1, (v3 >> 1) & 1, v3 >> 2)
                s3 = g(1, 1, 1)
                val = b0 * s0 + b1 * s1 + b2 * s2 + b3 * s3
    return np.where(st == 2, QNAN, np.where(st == 1, outside, val)).astype(F)


def normal(q, d, p, mode=TRILINEAR, iso=0.0, outside=100.0):
    """estimate_normal (:202-209): (0, 0, 0) where the length is 0, NaN x 3 for a NaN point."""
    p = np.asarray(p, F).reshape(-1, 3)
    e = q.eps
    s = []
    for k in range(3):
        for sign in (1, -1):
            pk = p.copy()
            pk[:, k] = p[:, k] + e if sign > 0 else p[:, k] - e
            s.append(sample(q, d, pk, mode, iso, outside))
    v = np.stack([s[0] - s[1], s[2] - s[3], s[4] - s[5]], 1)
    with np.errstate(all="ignore"):
        ln = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        n = v / ln[:, None]
    n = np.where((ln == 0)[:, None], F(0), n)
    return np.where(np.isnan(p).any(1)[:, None], QNAN, n).astype(F)


def raymarch(q, d, o, r, mode=TRILINEAR, iso=0.0, outside=100.0, max_steps=100, normals=False):
    """sdf_3d (:265-287) -> (hit (n, 4) = (position, dist), steps u32, is_hit bool[, normals (n, 3)])."""
    o = np.asarray(o, F).reshape(-1, 3)
    r = np.asarray(r, F).reshape(-1, 3)
    n = o.shape[0]
    eps = q.eps
    nan = np.isnan(o).any(1) | np.isnan(r).any(1)
    outb = (o < q.start).any(1) | (o > q.end).any(1)
    with np.errstate(all="ignore"):
        t0 = (q.start - o) / r                                       # intersectAABB (:245-253), fmin / fmax
        t1 = (q.end - o) / r
        t_1, t_2 = np.fmin(t0, t1), np.fmax(t0, t1)
        tn = np.fmax(np.fmax(t_1[:, 0], t_1[:, 1]), t_1[:, 2])
        tf = np.fmin(np.fmin(t_2[:, 0], t_2[:, 1]), t_2[:, 2])
        miss = ~nan & outb & (tn > tf)
        enter = ~nan & outb & ~miss
        pos = o.copy()
        t = tn + eps
        pos[enter] = o[enter] + t[enter][:, None] * r[enter]        # :280
        dist = np.zeros(n, F)
        steps = np.zeros(n, np.uint32)
        march = ~nan & ~miss
        active = np.flatnonzero(march)
        for _ in range(int(max_steps)):                              # :283-289
            if active.size == 0:
                break
            dd = sample(q, d, pos[active], mode, iso, outside)
            dist[active] = dd
            go = ~(dd < eps)
            adv = active[go]
            pos[adv] = pos[adv] + r[adv] * dd[go][:, None]
            steps[adv] += 1
            active = adv
    pos[miss] = 0
    dist[miss] = 1
    pos[nan] = QNAN
    dist[nan] = QNAN
    hit = march & (dist < eps)
    out = np.concatenate([pos, dist[:, None]], 1).astype(F)
    if not normals:
        return out, steps, hit
    nrm = np.zeros((n, 3), F)
    if hit.any():
        nrm[hit] = normal(q, d, pos[hit], mode, iso, outside)
    return out, steps, hit, nrm


def same_bits(a, b):
    """Bit equality, with every NaN counted as one value (a NaN made by arithmetic may carry another payload on the host)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))
