"""The definitions of m2s_band_components and m2s_band_select (include/m2s.h) in numpy, to the bit.  Everything is built densely, so it is
for the small grids of the tests; the library does the same with nothing sized by the grid.

A band is a band_csg_model.Band.  `components` returns a Components: labels (uint32, one per cell of the band, in list order), count and
the five statistics per component.  `select` returns (Band, SelectInfo): the kept cells ascending with their distances, a sign mask on
every grid point (bits at k >= nz zero) and the backgrounds."""
from typing import NamedTuple

import numpy as np

from band_csg_model import Band, dense, pack_bits, unpack_bits

F = np.float32
LABEL_NONE = 0xffffffff
CONNECTIVITIES = (6, 18, 26)


class Components(NamedTuple):
    labels: np.ndarray       # uint32[n]
    count: int
    first_cell: np.ndarray   # uint64[count]
    n_cells: np.ndarray      # uint64[count]
    n_negative: np.ndarray   # uint64[count]
    lo: np.ndarray           # uint32[count, 3]
    hi: np.ndarray           # uint32[count, 3]


class SelectInfo(NamedTuple):
    n_cells: int
    n_dropped: int
    n_sign_cleared: int


def backward_steps(connectivity):
    """The steps (di, dj, dk) of the stencil that lead to a smaller L: 3, 9 or 13 of them."""
    axes = {6: 1, 18: 2, 26: 3}[connectivity]
    steps = [(di, dj, dk) for di in (-1, 0, 1) for dj in (-1, 0, 1) for dk in (-1, 0, 1)
             if (di, dj, dk) < (0, 0, 0) and (di != 0) + (dj != 0) + (dk != 0) <= axes]
    assert len(steps) == {6: 3, 18: 9, 26: 13}[connectivity]
    return steps


def edges(band, connectivity):
    """-> (a, b): list places of every pair of joined cells, b the one with the smaller L.  No clamping: a step off the grid is no edge."""
    nx, ny, nz = band.shape
    rank = np.full(band.shape, -1, np.int64)
    rank.reshape(-1)[band.cells] = np.arange(band.cells.size)
    i, j, k = np.unravel_index(band.cells, band.shape)
    ea, eb = [], []
    for di, dj, dk in backward_steps(connectivity):
        ii, jj, kk = i + di, j + dj, k + dk
        on = (ii >= 0) & (ii < nx) & (jj >= 0) & (jj < ny) & (kk >= 0) & (kk < nz)
        q = np.full(i.size, -1, np.int64)
        q[on] = rank[ii[on], jj[on], kk[on]]
        hit = q >= 0
        ea.append(np.flatnonzero(hit))
        eb.append(q[hit])
    return (np.concatenate(ea), np.concatenate(eb)) if ea else (np.zeros(0, np.int64), np.zeros(0, np.int64))


def components(band, connectivity=6):
    """m2s_band_components: an iterated minimum over the edges.  p[r] ends as the smallest list place of r's component; a round hooks
    every root under the smallest root it shares an edge with and then flattens, so the components at least halve per round."""
    n = band.cells.size
    ea, eb = edges(band, connectivity)
    p = np.arange(n, dtype=np.int64)
    while True:
        pa, pb = p[ea], p[eb]
        if np.array_equal(pa, pb):
            break
        np.minimum.at(p, np.maximum(pa, pb), np.minimum(pa, pb))
        while True:
            pp = p[p]
            if np.array_equal(pp, p):
                break
            p = pp
    roots = np.flatnonzero(p == np.arange(n))                  # ascending list place = ascending smallest L: the raster numbering
    labels = np.searchsorted(roots, p).astype(np.uint32)
    count = roots.size
    i, j, k = np.unravel_index(band.cells, band.shape)
    ijk = np.stack([i, j, k], 1).astype(np.uint32).reshape(-1, 3)
    lo = np.full((count, 3), 0xffffffff, np.uint32)
    hi = np.zeros((count, 3), np.uint32)
    for a in range(3):
        np.minimum.at(lo[:, a], labels, ijk[:, a])
        np.maximum.at(hi[:, a], labels, ijk[:, a])
    return Components(labels, count, band.cells[roots].astype(np.uint64), np.bincount(labels, minlength=count).astype(np.uint64),
                      np.bincount(labels, weights=band.distances < 0, minlength=count).astype(np.uint64), lo, hi)


def kept_cells(labels, keep):
    """Cell r is kept iff labels[r] < n_keep and keep[labels[r]] != 0."""
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    keep = np.asarray(keep).astype(np.uint8).reshape(-1)
    ok = labels < keep.size
    out = np.zeros(labels.size, bool)
    out[ok] = keep[labels[ok]] != 0
    return out


def clear_row(active, dropped, inside):
    """The sign rule on one k-row -> the inactive-inside points to clear: the nearest active cell towards +k and the nearest towards
    -k are dropped cells, for every side that has one, and at least one side has one.  (clear_row_plain is the same, point by point.)"""
    nz = active.size
    idx = np.arange(nz)
    down = np.maximum.accumulate(np.where(active, idx, -1))                  # at an inactive k: the nearest active cell below it
    up = np.minimum.accumulate(np.where(active, idx, nz)[::-1])[::-1]
    has_d, has_u = down >= 0, up < nz
    drop_d, drop_u = dropped[np.clip(down, 0, nz - 1)], dropped[np.clip(up, 0, nz - 1)]
    return inside & ~active & (has_d | has_u) & (~has_d | drop_d) & (~has_u | drop_u)


def clear_row_plain(active, dropped, inside):
    nz = active.size
    out = np.zeros(nz, bool)
    for k in range(nz):
        if active[k] or not inside[k]:
            continue
        up = next((m for m in range(k + 1, nz) if active[m]), None)
        down = next((m for m in range(k - 1, -1, -1) if active[m]), None)
        sides = [m for m in (up, down) if m is not None]
        out[k] = len(sides) > 0 and all(dropped[m] for m in sides)
    return out


def select(band, labels, keep, background=None):
    """m2s_band_select -> (Band, SelectInfo).  background: (outside, inside) of the result; None is the input's."""
    kept = kept_cells(labels, keep)
    if kept.size != band.cells.size:
        raise ValueError("one label per cell")
    act, d, _ = dense(band)
    inside = unpack_bits(band.shape, band.bits)
    kept_d = np.zeros(band.total, bool)
    kept_d[band.cells[kept]] = True
    kept_d = kept_d.reshape(band.shape)
    dropped_d = act & ~kept_d
    s = np.zeros(band.shape, bool)
    cleared = 0
    for i in range(band.shape[0]):
        for j in range(band.shape[1]):
            loose = inside[i, j] & ~act[i, j]
            gone = clear_row(act[i, j], dropped_d[i, j], inside[i, j]) if loose.any() else np.zeros(band.shape[2], bool)
            cleared += int(gone.sum())
            s[i, j] = np.where(kept_d[i, j], d[i, j] < 0, loose & ~gone)
    bg_out, bg_in = (band.bg_out, band.bg_in) if background is None else background
    out = Band(band.shape, band.cells[kept], band.distances[kept], pack_bits(band.shape, s), bg_out, bg_in)
    return out, SelectInfo(int(kept.sum()), int((~kept).sum()), cleared)


# ---- the scene of the chain tests: (A | B) | D, then all but the two largest components erased ------------------------------------------
# On band_redistance_model's grid (40 x 36 x 44 cells of 0.05 x 0.04 x 0.0625); a cell is its largest side, as in the other band tests.
# Half-widths of 1.5 cells hold a cut cube's corners (its diagonal is 0.0895), so the bands mesh with n_open == 0.  Every pair of
# surfaces is more than 0.35 apart, above two band widths plus two cells (0.3125).
CHAIN_HALF = 1.5 * 0.0625
CHAIN_SPHERES = {"A": ((0.0, 0.0, -0.75), 0.45), "B": ((0.0, 0.0, 0.55), 0.4), "D": ((0.65, 0.35, -0.12), 0.17)}


def chain_bands():
    """-> (A, B, D, A | B, (A | B) | D) as Bands, by band_redistance_model and band_csg_model."""
    import band_csg_model as cm
    import band_redistance_model as rm

    a, b, d = (rm.band_of(rm.sphere(c, r), CHAIN_HALF) for c, r in (CHAIN_SPHERES[k] for k in "ABD"))
    ab = cm.csg(a, b, cm.UNION)
    return a, b, d, ab, cm.csg(ab, d, cm.UNION)
