"""Test oracle of the band queries (include/m2s.h m2s_band_sample / m2s_band_raymarch): grid_query_model's sample, normal and raymarch with
the cell read replaced by a sparse fetch.  The fetch is searchsorted on the band's ascending `cells`; a grid point that is not in the list
reads the background, negative where the sign mask has its bit.  No array sized by the grid is made (the sign mask, one bit per point in
the layout of Voxels.bits, is the caller's), so it works on grids too large for a dense D'.  `support` is computed alongside.

The model takes `cells` as ascending and in range: whether they are is the library's check (m2s_band_create), not the model's."""
import numpy as np

import grid_query_model as gqm

F = np.float32
K_OF = {gqm.SNAP: 1, gqm.TRILINEAR: 8, gqm.TETRAHEDRAL: 4}


class Band:
    """The dense grid D' of include/m2s.h, indexable by int64 cell offsets like grid_query_model's `d`.  Every read adds its active
    entries to `hits` (one counter per row of the index array), which is how support is counted: after clamping, a cell read twice
    counting twice."""

    def __init__(self, cell_count, cells, distances, background_outside, background_inside, inside_bits=None):
        self.n = tuple(int(c) for c in cell_count)
        self.cells = np.asarray(cells).astype(np.int64).reshape(-1)
        self.distances = np.asarray(distances, F).reshape(-1)
        self.bg_out, self.bg_in_neg = F(background_outside), -F(background_inside)
        self.bits = None if inside_bits is None else np.asarray(inside_bits, np.uint32).reshape(self.n[0], self.n[1], (self.n[2] + 31) // 32)
        self.hits = None

    def lookup(self, L):
        """-> (values, active) at the grid points L."""
        L = np.asarray(L, np.int64)
        at = np.searchsorted(self.cells, L)
        at_c = np.minimum(at, max(self.cells.size - 1, 0))
        active = (at < self.cells.size) & (self.cells[at_c] == L) if self.cells.size else np.zeros(L.shape, bool)
        bg = np.full(L.shape, self.bg_out, F)
        if self.bits is not None:
            nyz = self.n[1] * self.n[2]
            i, r = L // nyz, L % nyz
            j, k = r // self.n[2], r % self.n[2]
            inside = (self.bits[i, j, k >> 5] >> (k & 31).astype(np.uint32)) & 1
            bg = np.where(inside == 1, self.bg_in_neg, bg).astype(F)
        val = np.where(active, self.distances[at_c] if self.cells.size else bg, bg).astype(F)
        return val, active

    def __getitem__(self, L):
        val, active = self.lookup(L)
        if self.hits is not None and self.hits.shape == active.shape:
            self.hits += active
        return val

    def dense(self):
        """D' itself, float32[nx, ny, nz]: for the small grids of the tests."""
        total = self.n[0] * self.n[1] * self.n[2]
        return self.lookup(np.arange(total, dtype=np.int64))[0].reshape(self.n)


def sample(q, band, p, mode=gqm.TRILINEAR, iso=0.0, outside=100.0):
    """-> (values f32[n], support u8[n]): grid_query_model.sample reading the band; support is 0 off the box and for a NaN coordinate."""
    p = np.asarray(p, F).reshape(-1, 3)
    band.hits = np.zeros(p.shape[0], np.int64)
    try:
        val = gqm.sample(q, band, p, mode, iso, outside)
        hits = band.hits
    finally:
        band.hits = None
    inside = gqm._state(q, p) == 0
    return val, np.where(inside, hits, 0).astype(np.uint8)


def normal(q, band, p, mode=gqm.TRILINEAR, iso=0.0, outside=100.0):
    return gqm.normal(q, band, p, mode, iso, outside)


def raymarch(q, band, o, r, mode=gqm.TRILINEAR, iso=0.0, outside=100.0, max_steps=100, normals=False):
    """grid_query_model.raymarch reading the band -> (hit (n, 4), steps u32, is_hit bool, support u8[, normals (n, 3)]); support is that of
    the last sample the march evaluated, 0 for a ray that never marched."""
    o = np.asarray(o, F).reshape(-1, 3)
    r = np.asarray(r, F).reshape(-1, 3)
    n = o.shape[0]
    eps = q.eps
    nan = np.isnan(o).any(1) | np.isnan(r).any(1)
    outb = (o < q.start).any(1) | (o > q.end).any(1)
    support = np.zeros(n, np.uint8)
    with np.errstate(all="ignore"):
        t0 = (q.start - o) / r
        t1 = (q.end - o) / r
        t_1, t_2 = np.fmin(t0, t1), np.fmax(t0, t1)
        tn = np.fmax(np.fmax(t_1[:, 0], t_1[:, 1]), t_1[:, 2])
        tf = np.fmin(np.fmin(t_2[:, 0], t_2[:, 1]), t_2[:, 2])
        miss = ~nan & outb & (tn > tf)
        enter = ~nan & outb & ~miss
        pos = o.copy()
        t = tn + eps
        pos[enter] = o[enter] + t[enter][:, None] * r[enter]
        dist = np.zeros(n, F)
        steps = np.zeros(n, np.uint32)
        march = ~nan & ~miss
        active = np.flatnonzero(march)
        for _ in range(int(max_steps)):
            if active.size == 0:
                break
            dd, sup = sample(q, band, pos[active], mode, iso, outside)
            dist[active] = dd
            support[active] = sup
            go = ~(dd < eps)
            adv = active[go]
            pos[adv] = pos[adv] + r[adv] * dd[go][:, None]
            steps[adv] += 1
            active = adv
    pos[miss] = 0
    dist[miss] = 1
    pos[nan] = gqm.QNAN
    dist[nan] = gqm.QNAN
    hit = march & (dist < eps)
    out = np.concatenate([pos, dist[:, None]], 1).astype(F)
    if not normals:
        return out, steps, hit, support
    nrm = np.zeros((n, 3), F)
    if hit.any():
        nrm[hit] = normal(q, band, pos[hit], mode, iso, outside)
    return out, steps, hit, support, nrm
