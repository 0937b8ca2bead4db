"""Test oracle of m2s_band_isosurface (include/m2s.h): the definition in numpy, built on isosurface_model.extract.

The sparse result is the dense m2s_grid_isosurface of any grid that agrees with the band on its points, kept where the band alone decides
it: the vertices whose edge has both ends active, the triangles whose cell has all 8 corners active (renumbered), and n_open, the number of
active points that own a cell which is incomplete although its active corners lie on both sides of iso.  `extract` follows that literally:
fill the inactive points, extract densely, keep and renumber.

The box form does the same on a box [i0, i1) x [j0, j1) x [k0, k1) of a grid too large to hold: positions come from the full-grid
coordinates (first + (float)i * cs with the absolute i) and the cells are full-grid L = k + j*nz + i*ny*nz.  Within a box the ascending
order of L is the C order of the box, so a band whose cells lie in boxes with disjoint, ascending i ranges has the boxes' outputs one
after the other."""
import numpy as np

import isosurface_model as im

F = np.float32


class _BoxGrid(im.GridI):
    """A box of a grid as a grid of its own shape whose coordinates are the full grid's."""

    def __init__(self, g, lo, shape):
        self.first, self.cs, self.n, self.lo = g.first, g.cs, tuple(int(v) for v in shape), tuple(int(v) for v in lo)

    def coord(self, axis, i):
        return (self.first[axis] + (np.asarray(i, np.int64) + self.lo[axis]).astype(F) * self.cs[axis]).astype(F)


def _corner_sum(x):
    """Per cell (shape - 1 on every axis): how many of its 8 corners have x set."""
    s = np.zeros(tuple(n - 1 for n in x.shape), np.int64)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                s += x[dx:dx + s.shape[0], dy:dy + s.shape[1], dz:dz + s.shape[2]]
    return s


def extract_box(g, box, cells, distances, iso=0.0, fill=0.0):
    """(V, T, n_open) of the band cells `cells` (full-grid L, ascending, all inside `box`) with values `distances`.  Every active point
    must have its +1 neighbours inside the box or beyond the grid, so that no cell it owns is cut off by the box."""
    (i0, i1), (j0, j1), (k0, k1) = box
    ny, nz = g.n[1], g.n[2]
    L = np.asarray(cells).astype(np.int64).reshape(-1)
    assert (np.diff(L) > 0).all(), "cells must ascend strictly"
    i, j, k = L // (ny * nz) - i0, (L // nz) % ny - j0, L % nz - k0
    shape = (i1 - i0, j1 - j0, k1 - k0)
    assert all((0 <= c).all() and (c < n).all() for c, n in zip((i, j, k), shape)), "a cell outside the box"
    d = np.full(shape, fill, F)
    act = np.zeros(shape, bool)
    d[i, j, k] = np.asarray(distances, F).reshape(-1)
    act[i, j, k] = True
    for axis, hi in enumerate((i1, j1, k1)):
        assert hi == g.n[axis] or not np.take(act, -1, axis).any(), "an active point on a face where the box cuts the grid"
    iso = F(iso)
    V, T = im.extract(_BoxGrid(g, (i0, j0, k0), shape), d, iso)
    # the edge of every vertex, in V's order (ascending 3*L + a = the C order of the crossing flags)
    inside = d < iso
    ii, jj, kk, aa = np.nonzero(im._crossings(inside, shape[0], shape[0]))
    assert ii.size == len(V)
    keep_v = act[ii, jj, kk] & act[ii + (aa == 0), jj + (aa == 1), kk + (aa == 2)]
    if min(shape) < 2:
        assert len(T) == 0
        return V[keep_v], T, 0
    # the cell of every triangle, in T's order (cell L, then the table's order)
    case = im._cases(inside, shape[0] - 1)
    n_act = _corner_sum(act)
    ci, cj, ck = np.nonzero(im.TRI_COUNT[case] > 0)
    cell_of_tri = np.repeat(np.arange(ci.size), im.TRI_COUNT[case[ci, cj, ck]])
    assert cell_of_tri.size == len(T)
    keep_t = (n_act[ci, cj, ck] == 8)[cell_of_tri]
    kept = T[keep_t].astype(np.int64)
    assert keep_v[kept].all(), "a complete cell uses an edge with an inactive end"
    new_id = np.cumsum(keep_v) - 1
    n_in = _corner_sum(act & inside)
    is_open = act[:-1, :-1, :-1] & (n_act < 8) & (n_in > 0) & (n_in < n_act)
    return V[keep_v], new_id[kept].astype(np.uint32).reshape(-1, 3), int(is_open.sum())


def extract(g, cells, distances, iso=0.0, fill=0.0):
    """The whole m2s_band_isosurface output on a grid small enough to hold: (V f32 (n, 3), T u32 (m, 3), n_open).  `fill` is the value of
    the inactive points in the dense grid the definition goes through; nothing in the result depends on it."""
    return extract_box(g, tuple((0, n) for n in g.n), cells, distances, iso, fill)


def covered(g, d_dense, active, iso=0.0):
    """The corollary's condition: every cell of the DENSE grid whose 8 corners are not all on one side of iso has all 8 corners active.
    Then the band's result is the dense one, bit for bit.  Needs at least 2 points on every axis."""
    assert min(g.n) >= 2
    d = np.asarray(d_dense, F).reshape(g.n)
    act = np.asarray(active, bool).reshape(g.n)
    n_in = _corner_sum(d < F(iso))
    mixed = (n_in > 0) & (n_in < 8)
    return bool((~mixed | (_corner_sum(act) == 8)).all())


def band_of(d_dense, interior, exterior):
    """The narrow band's filter on a dense grid: (cells uint64 ascending, distances)."""
    d = np.asarray(d_dense, F).reshape(-1)
    with np.errstate(invalid="ignore"):
        active = (F(-interior) <= d) & (d <= F(exterior))
    return np.flatnonzero(active).astype(np.uint64), d[active]
