"""The definition of m2s_band_filter (include/m2s.h) in numpy: the values of a narrow band smoothed by a mean, a Laplacian or a
mean-curvature flow, on the whole band or inside a region, per grid point and to the bit.  Everything is built densely (the grid D' the
band stands for, padded with its own edge values), so it is for the small grids of the tests; the library does the same with no array
sized by the grid.

`band_filter` takes a `Band` of tests/band_csg_model.py and returns (Band, Info).  All arithmetic is IEEE binary32 without FMA, every
operation in the order written here; every pass is Jacobi (each new value from the previous pass's values only), which the bits depend on."""
from typing import NamedTuple

import numpy as np

from band_csg_model import F, Band, dense, pack_bits, same  # noqa: F401  (same: re-exported for the tests)

MEAN, LAPLACIAN, MEAN_CURVATURE = 0, 1, 2
KINDS = (MEAN, LAPLACIAN, MEAN_CURVATURE)


class Info(NamedTuple):
    passes: int
    max_change: float          # a binary32 value (np.float32); +inf is possible
    n_changed: int
    n_sign_flips: int
    n_nonfinite: int


class Constants(NamedTuple):
    r: tuple
    w: tuple
    dt: np.float32


def constants(cell_size):
    """The host constants: r_a = 1 / h_a, w_a = r_a * r_a, dt = 1 / (2 * ((w_i + w_j) + w_k)), all in binary32."""
    h = [F(v) for v in cell_size]
    r = tuple(F(1) / v for v in h)
    w = tuple(v * v for v in r)
    dt = F(1) / (F(2) * ((w[0] + w[1]) + w[2]))
    return Constants(r, w, dt)


def neighbours(v):
    """N(di, dj, dk) of the definition: reads of v clamped to the box, as a function of the three steps."""
    p = np.pad(v, 1, mode="edge")
    nx, ny, nz = v.shape

    def N(di=0, dj=0, dk=0):
        return p[1 + di:1 + di + nx, 1 + dj:1 + dj + ny, 1 + dk:1 + dk + nz]
    return N


def step_of(axis, sign):
    d = [0, 0, 0]
    d[axis] = sign
    return d


def candidate(v, kind, axis, k):
    """cand of one pass on every grid point (the caller keeps it on the active cells of the region).  axis: the axis of a MEAN pass."""
    N = neighbours(v)
    c = v
    with np.errstate(all="ignore"):
        if kind == MEAN:
            return (((N(*step_of(axis, -1)) + c) + N(*step_of(axis, 1))) / F(3)).astype(F)
        t = [((N(*step_of(a, 1)) - c) + (N(*step_of(a, -1)) - c)) * k.w[a] for a in range(3)]
        if kind == LAPLACIAN:
            return (c + k.dt * ((t[0] + t[1]) + t[2])).astype(F)
        g = [(N(*step_of(a, 1)) - N(*step_of(a, -1))) * (F(0.5) * k.r[a]) for a in range(3)]

        def cross(a, b):
            def at(sa, sb):
                d = [0, 0, 0]
                d[a], d[b] = sa, sb
                return N(*d)
            return ((at(1, 1) - at(1, -1)) - (at(-1, 1) - at(-1, -1))) * (F(0.25) * (k.r[a] * k.r[b]))
        xij, xik, xjk = cross(0, 1), cross(0, 2), cross(1, 2)
        q = [g[a] * g[a] for a in range(3)]
        num = (((t[0] * (q[1] + q[2]) + t[1] * (q[0] + q[2])) + t[2] * (q[0] + q[1]))
               - F(2) * (((g[0] * g[1]) * xij + (g[0] * g[2]) * xik) + (g[1] * g[2]) * xjk))
        g2 = (q[0] + q[1]) + q[2]
        flow = c + k.dt * (num / g2)
        return np.where(g2 > 0, flow, c).astype(F)


def band_filter(band, cell_size, kind, iterations=1, where=None, background=None):
    """The result of m2s_band_filter as (Band, Info).  where: a Band on the same grid, whose s is the region, or None for everywhere.
    background: (outside, inside) of the result; None is the input's."""
    if kind not in KINDS or not 1 <= iterations <= 65536:
        raise ValueError("bad kind or iterations")
    if where is not None and where.shape != band.shape:
        raise ValueError("the band's and the region's grids differ")
    k = constants(cell_size)
    act, x, s = dense(band)
    region = act if where is None else act & dense(where)[2]
    v = x.copy()
    passes = iterations * (3 if kind == MEAN else 1)
    n_nonfinite = 0
    if band.cells.size:
        for p in range(passes):
            cand = candidate(v, kind, p % 3, k)
            ok = np.isfinite(cand)
            n_nonfinite += int((region & ~ok).sum())
            v = np.where(region & ok, cand, v).astype(F)
    r = v.reshape(-1)[band.cells]
    x0 = x.reshape(-1)[band.cells]
    with np.errstate(all="ignore"):
        change = np.abs(r - x0)
    info = Info(passes, F(change.max()) if r.size else F(0), int((r.view(np.uint32) != x0.view(np.uint32)).sum()),
                int(((r < 0) != (x0 < 0)).sum()), n_nonfinite)
    bg_out, bg_in = (band.bg_out, band.bg_in) if background is None else background
    return Band(band.shape, band.cells, r, pack_bits(band.shape, np.where(act, v < 0, s)), bg_out, bg_in), info


# ---- measurements the tests and DESIGN.md 4.19 share ----------------------------------------------------------------------------------
def x_crossings(band, first, cells):
    """The zero crossings of D' along x grid lines, linearly interpolated between two ACTIVE neighbours of opposite sign: the crossing
    points as float64 [n, 3]."""
    act, d, _ = dense(band)
    d = d.astype(np.float64)
    ax = [(F(first[a]) + np.arange(band.shape[a], dtype=F) * F(cells[a])).astype(np.float64) for a in range(3)]
    lo, hi = d[:-1], d[1:]
    both = act[:-1] & act[1:] & ((lo < 0) != (hi < 0))
    i, j, kk = np.nonzero(both)
    t = lo[both] / (lo[both] - hi[both])
    return np.stack([ax[0][i] + t * (ax[0][i + 1] - ax[0][i]), ax[1][j], ax[2][kk]], 1)
