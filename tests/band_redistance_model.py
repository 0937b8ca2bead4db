"""The definition of m2s_band_redistance (include/m2s.h) in numpy: a narrow band turned back into a distance field with the same zero
set and the half-widths the caller asks for, per grid point and to the bit.  Everything is built densely, so it is for the small grids of
the tests; the library does the same with no array sized by the grid.

`redistance` takes a `Band` of tests/band_csg_model.py and returns (Band, Info).  All arithmetic is IEEE binary32 without FMA, every
operation in the order written here; the sweep is Jacobi (every new value from the previous sweep's values only), which the bits depend on."""
from typing import NamedTuple

import numpy as np

from band_csg_model import F, Band, dense, pack_bits, same  # noqa: F401  (same: re-exported for the tests)

INF = F(np.inf)
AXES = ((0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1))


class Info(NamedTuple):
    sweeps: int
    converged: int
    n_frozen: int
    n_open: int
    n_candidates: int


def reach(width, h, n):
    """K_a = min(ceil(W / h_a) + 1, n_a): the division in binary32, the ceil of that quotient."""
    with np.errstate(over="ignore"):
        c = np.ceil(F(width) / F(h))
    return int(n) if c >= n else int(c) + 1


def default_sweeps(exterior, interior, cell_size, shape):
    w = max(F(exterior), F(interior))
    return 2 * sum(reach(w, cell_size[a], shape[a]) for a in range(3)) + 8


def shifted(a, axis, step, fill):
    """out[L] = a[L + step along axis], `fill` where that neighbour is off the grid."""
    out = np.full_like(a, fill)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    if step > 0:
        src[axis], dst[axis] = slice(step, None), slice(None, -step)
    else:
        src[axis], dst[axis] = slice(None, step), slice(-step, None)
    if a.shape[axis] > abs(step):
        out[tuple(dst)] = a[tuple(src)]
    return out


def frozen_set(act, s):
    """-> (F bool, n_open): active points with an active axis neighbour of the other sign; the pairs whose other end is inactive."""
    frozen = np.zeros_like(act)
    n_open = 0
    for axis, step in AXES:
        there = shifted(np.ones_like(act), axis, step, False)
        differs = there & (shifted(s, axis, step, False) != s)
        m_act = shifted(act, axis, step, False)
        frozen |= act & differs & m_act
        n_open += int((act & differs & ~m_act).sum())
    return frozen, n_open


def box_dilate(a, reach3):
    """a dilated by the box |di| <= Kx, |dj| <= Ky, |dk| <= Kz, clipped to the grid."""
    out = a
    for axis, K in enumerate(reach3):
        n = a.shape[axis]
        pad = [(0, 0)] * 3
        pad[axis] = (K + 1, K)
        c = np.cumsum(np.pad(out.astype(np.int64), pad), axis=axis)
        hi = [slice(None)] * 3
        lo = [slice(None)] * 3
        hi[axis], lo[axis] = slice(2 * K + 1, 2 * K + 1 + n), slice(0, n)
        out = (c[tuple(hi)] - c[tuple(lo)]) > 0
    return out


def sweep(u, s, free, W, h):
    """One Jacobi sweep: u^{n+1} from u^n on the points of `free` (C \\ F).  W: the cut-off per point (by its side); h: f32[3]."""
    with np.errstate(all="ignore"):
        cut = np.where(u <= W, u, INF)                      # c(v, M): the neighbour's own W, which is W(L) where s[M] == s[L]
        m = []
        for axis in range(3):
            best = np.full_like(u, INF)
            for step in (1, -1):
                ok = shifted(np.ones_like(s), axis, step, False) & (shifted(s, axis, step, False) == s)
                v = np.where(ok, shifted(cut, axis, step, INF), INF)
                best = np.where(v < best, v, best)
            m.append(best)
        hs = [np.full_like(u, h[a]) for a in range(3)]
        # a stable sort of three: swap only on a strict <, in the order (0,1) (1,2) (0,1)
        for i, j in ((0, 1), (1, 2), (0, 1)):
            sw = m[j] < m[i]
            m[i], m[j] = np.where(sw, m[j], m[i]), np.where(sw, m[i], m[j])
            hs[i], hs[j] = np.where(sw, hs[j], hs[i]), np.where(sw, hs[i], hs[j])
        a1, a2, a3 = m
        h1, h2, h3 = hs
        one = F(1.0)
        w1, w2, w3 = one / (h1 * h1), one / (h2 * h2), one / (h3 * h3)
        t = a1 + h1
        two = t > a2
        d2 = a2 - a1
        A = w1 + w2
        B = w2 * d2
        q2 = w2 * d2 * d2
        C = q2 - one
        disc = B * B - A * C
        disc = np.where(disc > 0, disc, F(0.0))
        t2 = a1 + (B + np.sqrt(disc)) / A
        t = np.where(two, t2, t)
        three = two & (t > a3)
        d3 = a3 - a1
        A3 = A + w3
        B3 = B + w3 * d3
        C3 = (q2 + w3 * d3 * d3) - one
        disc = B3 * B3 - A3 * C3
        disc = np.where(disc > 0, disc, F(0.0))
        t3 = a1 + (B3 + np.sqrt(disc)) / A3
        t = np.where(three, t3, t).astype(F)
        return np.where(free & (t < u), t, u).astype(F)


def redistance(band, cell_size, exterior, interior, max_sweeps=0, background=None):
    """The result of m2s_band_redistance as (Band, Info).  background: (outside, inside) of the result; None is the two widths."""
    exterior, interior = F(exterior), F(interior)
    if not (np.isfinite(exterior) and np.isfinite(interior) and exterior >= 0 and interior >= 0):
        raise ValueError("bad widths")
    h = np.asarray(cell_size, F)
    shape = band.shape
    act, x, s = dense(band)
    frozen, n_open = frozen_set(act, s)
    k_out = tuple(reach(exterior, h[a], shape[a]) for a in range(3))
    k_in = tuple(reach(interior, h[a], shape[a]) for a in range(3))
    cand = np.where(s, box_dilate(frozen, k_in), box_dilate(frozen, k_out))
    W = np.where(s, interior, exterior).astype(F)
    if max_sweeps == 0:
        max_sweeps = default_sweeps(exterior, interior, h, shape)
    u = np.where(frozen, np.abs(x), INF).astype(F)
    free = cand & ~frozen
    sweeps, converged = 0, 0
    for _ in range(max_sweeps):
        new = sweep(u, s, free, W, h)
        if np.array_equal(new.view(np.uint32), u.view(np.uint32)):
            converged = 1
            break
        u = new
        sweeps += 1
    active = frozen | (cand & (u <= W))
    r = np.where(frozen, x, np.where(s, -u, u)).astype(F)
    cells = np.flatnonzero(active.reshape(-1))
    bg_out, bg_in = (exterior, interior) if background is None else background
    out = Band(shape, cells, r.reshape(-1)[cells], pack_bits(shape, s), bg_out, bg_in)
    return out, Info(sweeps, converged, int(frozen.sum()), n_open, int(cand.sum()))


def offset(band, cell_size, distance, exterior, interior, max_sweeps=0):
    """BandField.offset in the model: the values minus `distance` (binary32), the sign mask rebuilt from them on the active cells and
    kept elsewhere, the backgrounds kept, then redistance.  -> (Band, Info)."""
    act, _, s = dense(band)
    moved = (band.distances - F(distance)).astype(F)
    s = s.copy().reshape(-1)
    s[band.cells] = moved < 0
    shiftedb = Band(band.shape, band.cells, moved, pack_bits(band.shape, s.reshape(band.shape)), band.bg_out, band.bg_in)
    return redistance(shiftedb, cell_size, exterior, interior, max_sweeps)


# ---- inputs the tests share: analytic solids sampled at the cell centres ----------------------------------------------------------------
SHAPE = (40, 36, 44)
CELLS = (0.05, 0.04, 0.0625)
FIRST = tuple(-(n - 1) * c / 2 for n, c in zip(SHAPE, CELLS))      # the grid centred on the origin


def centres(first=FIRST, cells=CELLS, shape=SHAPE):
    """The cell centres as m2s_grid_cell_center gives them (first + idx * size in binary32), as three float64 arrays [nx, ny, nz]."""
    ax = [(F(first[a]) + np.arange(shape[a], dtype=F) * F(cells[a])).astype(np.float64) for a in range(3)]
    return np.meshgrid(*ax, indexing="ij")


def sphere(centre, radius, **grid):
    x, y, z = centres(**grid)
    return np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius


def box(half, **grid):
    q = [np.abs(c) - b for c, b in zip(centres(**grid), half)]
    return np.sqrt(sum(np.maximum(v, 0) ** 2 for v in q)) + np.minimum(np.maximum(np.maximum(q[0], q[1]), q[2]), 0)


def band_of(d, width):
    """The band |d| <= width of a dense float64 field as a Band: its binary32 values, the sign mask d < 0 on every point, both
    backgrounds the width."""
    d32 = np.asarray(d).astype(F)
    cells = np.flatnonzero(np.abs(d32.reshape(-1)) <= F(width))
    return Band(d32.shape, cells, d32.reshape(-1)[cells], pack_bits(d32.shape, d32 < 0), width, width)


def fibonacci_sphere(centre, radius, n):
    k = np.arange(n) + 0.5
    z = 1 - 2 * k / n
    r = np.sqrt(1 - z * z)
    phi = k * (np.pi * (3 - 5 ** 0.5))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1) * radius + np.asarray(centre, np.float64)
