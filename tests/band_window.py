"""Windows: how the dense numpy models of the band calls (band_csg_model, band_redistance_model, band_filter_model) give expected values on
a grid far too large for them.  The active cells of such a test sit in a few small blocks.  A `Window` is a small box of the big grid
around one block; a model runs on the window as if it were a grid of its own, and its result is placed at the window's position in the
big grid.  That is exact only while nothing the call reads or writes crosses the window's sides, which is one rule per call:

  csg, export   defined per grid point: any window is exact.
  filter        the stencil reaches +-1 with clamped reads at the grid faces.  On every side of the window that is not a face of the big
                grid the outermost layer holds no active point, and its sign bits are the ones the big grid holds just beyond it.  On a
                side that is a face of the big grid the window ends at the same face.  A `where` band follows the same rule.
  redistance    the candidate box reaches K_a = min(ceil(W / h_a) + 1, n_a) from a frozen point.  On every interior side K_a + 1 layers
                hold no active point, the sign bits are uniform outside the box of the active cells, and the window's n_a exceeds K_a so
                that the `min` picks the same branch as on the big grid.
  advect        the filter rule as it stands: the stencil reaches +-1 with clamped reads, an inactive neighbour takes the background of
                its sign bit; there is no `where`.  `embed_field` puts the windows' velocities or speeds into the big grid's list order,
                `sum_advect` adds the infos up.
  components    a step off the grid is no edge and nothing is clamped, so a face of the big grid needs no care: on every side of a
                window that is not a face of the big grid the outermost layer holds no active point.  The windows being disjoint, no
                cell of one is then a 26-neighbour of a cell of another, and `merge_components` renumbers the windows' components by
                their first cell in the big grid.
  select        the sign rule is per k-row and looks to the row's ends, so a window spans whole rows: lo[2] == 0 and shape[2] == nz of
                the big grid, with any (i, j) extent (`row_window`).  Outside the windows no row holds an active cell and nothing is
                cleared: the mask there is the input's with the bits at k >= nz zero.  `sum_select` adds the infos up.

`check_filter`, `check_redistance`, `check_advect`, `check_components` and `check_select` raise LayoutError when a test's layout breaks its rule; tests/test_band_window_cpu.py proves the
rules (the dense model on a whole grid equals the window results embedded, bit for bit) on grids small enough for the dense models.

Everything here is numpy on window-sized arrays plus index arithmetic in Python integers / int64; nothing is sized by the big grid except
`embed_bits`, which the CPU tests alone use.  The large GPU tests patch the device sign mask through `Window.word_slices` / `put_bits`."""
from typing import NamedTuple

import numpy as np

import band_advect_model as am
import band_components_model as ccm
import band_csg_model as cm
import band_filter_model as fm
import band_query_model as bqm
import band_redistance_model as rm
import band_resample_model as rsm
import grid_query_model as gqm

F = np.float32


class LayoutError(AssertionError):
    """A test's layout of blocks and windows violates the rule that makes the window model exact."""


def _need(ok, msg):
    if not ok:
        raise LayoutError(msg)


class Window:
    """The box lo <= (i, j, k) < lo + shape of the grid `big`, as a grid of its own with cells L_w = k' + j' * nz_w + i' * ny_w * nz_w."""

    def __init__(self, big, lo, shape):
        self.big = tuple(int(n) for n in big)
        self.lo = tuple(int(n) for n in lo)
        self.shape = tuple(int(n) for n in shape)
        _need(all(l >= 0 and s >= 1 and l + s <= n for l, s, n in zip(self.lo, self.shape, self.big)), f"window {self.lo} + {self.shape} leaves the grid {self.big}")

    @property
    def hi(self):
        return tuple(l + s for l, s in zip(self.lo, self.shape))

    def at_face(self, axis, side):
        """Whether the window's low (side 0) or high (side 1) end along `axis` is a face of the big grid."""
        return self.lo[axis] == 0 if side == 0 else self.hi[axis] == self.big[axis]

    def ijk(self, cells_w):
        """Window cells -> big-grid (i, j, k), int64."""
        L = np.asarray(cells_w).astype(np.int64)
        _, ny, nz = self.shape
        return L // (ny * nz) + self.lo[0], (L // nz) % ny + self.lo[1], L % nz + self.lo[2]

    def to_big(self, cells_w):
        """Window cells -> big-grid cells L = k + j * nz + i * ny * nz (int64: exact up to 2^63)."""
        i, j, k = self.ijk(cells_w)
        return k + j * self.big[2] + i * (self.big[1] * self.big[2])

    def contains(self, cells):
        L = np.asarray(cells).astype(np.int64)
        _, ny, nz = self.big
        idx = (L // (ny * nz), (L // nz) % ny, L % nz)
        return np.logical_and.reduce([(c >= l) & (c < h) for c, l, h in zip(idx, self.lo, self.hi)])

    def from_big(self, cells):
        """Big-grid cells, all inside the window -> window cells."""
        L = np.asarray(cells).astype(np.int64)
        _need(bool(self.contains(L).all()), "a cell lies outside its window")
        _, ny, nz = self.big
        i, j, k = L // (ny * nz) - self.lo[0], (L // nz) % ny - self.lo[1], L % nz - self.lo[2]
        return k + j * self.shape[2] + i * (self.shape[1] * self.shape[2])

    def word_slices(self):
        """The slices of a sign mask uint32[nx, ny, ceil(nz / 32)] of the big grid that hold the window's bits."""
        return (slice(self.lo[0], self.hi[0]), slice(self.lo[1], self.hi[1]), slice(self.lo[2] >> 5, (self.hi[2] + 31) >> 5))

    def _unpacked(self, words):
        w = np.asarray(words).astype(np.uint32)
        _need(w.shape == tuple(s.stop - s.start for s in self.word_slices()), "the words are not the window's slice of the mask")
        bits = ((w[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).astype(bool)
        return bits.reshape(w.shape[0], w.shape[1], -1), self.lo[2] - ((self.lo[2] >> 5) << 5)

    def get_bits(self, words):
        """words: the mask's `word_slices()` part -> the window's sign bits, bool[shape]."""
        bits, off = self._unpacked(words)
        return bits[:, :, off:off + self.shape[2]].copy()

    def put_bits(self, words, s):
        """words with the window's bits replaced by s (bool[shape]); every other bit of those words is kept."""
        bits, off = self._unpacked(words)
        bits[:, :, off:off + self.shape[2]] = np.asarray(s, bool).reshape(self.shape)
        weights = np.uint64(1) << np.arange(32, dtype=np.uint64)
        return (bits.reshape(bits.shape[0], bits.shape[1], -1, 32).astype(np.uint64) * weights).sum(-1).astype(np.uint32)


def check_disjoint(windows):
    for a in range(len(windows)):
        for b in range(a + 1, len(windows)):
            apart = any(windows[a].hi[x] <= windows[b].lo[x] or windows[b].hi[x] <= windows[a].lo[x] for x in range(3))
            _need(windows[a].big == windows[b].big and apart, f"windows {a} and {b} overlap or are on different grids")


def split(windows, cells):
    """Big-grid cells -> per window the positions (into `cells`) of the cells it holds.  Every cell lies in exactly one window."""
    check_disjoint(windows)
    cells = np.asarray(cells).astype(np.int64)
    parts = [np.flatnonzero(w.contains(cells)) for w in windows]
    _need(sum(p.size for p in parts) == cells.size, "a cell lies in no window")
    return parts


def embed(windows, bands):
    """The window Bands placed in the big grid -> (cells ascending int64, distances float32)."""
    check_disjoint(windows)
    for w, b in zip(windows, bands):
        _need(b.shape == w.shape, "a band is not on its window")
    cells = np.concatenate([w.to_big(b.cells) for w, b in zip(windows, bands)])
    dist = np.concatenate([b.distances for b in bands]).astype(F)
    order = np.argsort(cells, kind="stable")
    return cells[order], dist[order]


def embed_bits(bits, windows, bands):
    """A copy of the big grid's mask uint32[nx, ny, ceil(nz / 32)] with every window's bits replaced by its Band's (None: zeros)."""
    out = np.array(bits, np.uint32)
    for w, b in zip(windows, bands):
        sl = w.word_slices()
        out[sl] = w.put_bits(out[sl], cm.unpack_bits(w.shape, b.bits))
    return out


def embed_band(windows, bands, outside_bits=None, masked=True):
    """The window Bands as one Band on the big grid (for grids the dense models can still hold).  outside_bits: the mask beyond the
    windows, None is zeros; masked False gives a Band without a sign mask.  The backgrounds are the first band's."""
    big = windows[0].big
    cells, dist = embed(windows, bands)
    bits = None
    if masked:
        base = np.zeros((big[0], big[1], (big[2] + 31) // 32), np.uint32) if outside_bits is None else outside_bits
        bits = embed_bits(base, windows, bands)
    return cm.Band(big, cells, dist, bits, bands[0].bg_out, bands[0].bg_in)


def same_as_embedded(got, windows, bands, outside_bits=None):
    """A Band on the big grid against the window Bands embedded: cells, distances and the sign mask on every grid point, bit for bit."""
    cells, dist = embed(windows, bands)
    base = np.zeros((got.shape[0], got.shape[1], (got.shape[2] + 31) // 32), np.uint32) if outside_bits is None else outside_bits
    return (np.array_equal(got.cells, cells) and np.array_equal(got.distances.view(np.uint32), dist.view(np.uint32))
            and got.bits is not None and np.array_equal(got.bits, embed_bits(base, windows, bands)))


# ---- the margin rules ----------------------------------------------------------------------------------------------------------------------
def _layers(a, axis, side, count):
    sl = [slice(None)] * 3
    sl[axis] = slice(0, count) if side == 0 else slice(a.shape[axis] - count, None)
    return a[tuple(sl)]


def check_filter(win, band, where=None, outside=False, call="filter"):
    """The filter rule.  outside: the sign bit the big grid holds on the layer just beyond every interior side of the window."""
    _need(band.shape == win.shape and (where is None or where.shape == win.shape), "a band is not on its window")
    for b, name in ((band, "band"), (where, "where")):
        if b is None:
            continue
        act, _, s = cm.dense(b)
        for axis in range(3):
            for side in (0, 1):
                if win.at_face(axis, side):
                    continue
                _need(not _layers(act, axis, side, 1).any(), f"{call}: the {name}'s outermost layer on axis {axis} side {side} holds an active point")
                _need(bool((_layers(s, axis, side, 1) == bool(outside)).all()), f"{call}: the {name}'s sign bits on axis {axis} side {side} differ from the next layer out")


def check_redistance(win, band, cell_size, exterior, interior, outside=False):
    """The redistance rule for the widths (exterior, interior).  outside: the uniform sign bit around the block, here and beyond the window."""
    _need(band.shape == win.shape, "the band is not on its window")
    act, _, s = cm.dense(band)
    if not act.any():
        _need(bool((s == bool(outside)).all()), "redistance: the sign bits of an empty window are not uniform")
        return
    idx = np.nonzero(act)
    lo, hi = [int(c.min()) for c in idx], [int(c.max()) + 1 for c in idx]
    beyond = np.ones(win.shape, bool)
    beyond[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = False
    _need(bool((s[beyond] == bool(outside)).all()), "redistance: the sign bits outside the block are not uniform")
    for axis in range(3):
        K = max(rm.reach(w, cell_size[axis], win.big[axis]) for w in (exterior, interior))
        _need(win.shape[axis] > K, f"redistance: the window's n = {win.shape[axis]} on axis {axis} does not exceed K = {K}")
        for side, room in ((0, lo[axis]), (1, win.shape[axis] - hi[axis])):
            if not win.at_face(axis, side):
                _need(room >= K + 1, f"redistance: {room} layers without active points on axis {axis} side {side}, K + 1 = {K + 1} are needed")


def check_advect(win, band, outside=False):
    """The advect rule: the filter's, without a `where`."""
    check_filter(win, band, None, outside, call="advect")


def check_components(win, band):
    """The components rule: no active point in the outermost layer of a side that is not a face of the big grid."""
    _need(band.shape == win.shape, "the band is not on its window")
    act = cm.dense(band)[0]
    for axis in range(3):
        for side in (0, 1):
            _need(win.at_face(axis, side) or not _layers(act, axis, side, 1).any(),
                  f"components: the band's outermost layer on axis {axis} side {side} holds an active point")


def check_select(win, band):
    """The select rule: the window spans whole k-rows of the big grid."""
    _need(band.shape == win.shape, "the band is not on its window")
    _need(win.lo[2] == 0 and win.shape[2] == win.big[2], f"select: the window covers k = {win.lo[2]} .. {win.hi[2] - 1} of rows of {win.big[2]}")


def row_window(big, lo, shape):
    """The window of whole k-rows over lo <= (i, j) < lo + shape."""
    return Window(big, (lo[0], lo[1], 0), (shape[0], shape[1], big[2]))


def rehome(band, src, dst, s=None):
    """A Band on the window `src` as a Band on the window `dst` of the same grid, which holds every cell of it.  s: its sign bits,
    bool[dst.shape]; None is the band's own where the windows overlap and clear elsewhere."""
    _need(band.shape == src.shape and src.big == dst.big, "the band is not on its window")
    if s is None:
        s = np.zeros(dst.shape, bool)
        lo = [max(a, b) for a, b in zip(src.lo, dst.lo)]
        hi = [min(a, b) for a, b in zip(src.hi, dst.hi)]
        if all(h > l for l, h in zip(lo, hi)):
            part = cm.unpack_bits(src.shape, band.bits)[tuple(slice(l - o, h - o) for l, h, o in zip(lo, hi, src.lo))]
            s[tuple(slice(l - o, h - o) for l, h, o in zip(lo, hi, dst.lo))] = part
    return cm.Band(dst.shape, dst.from_big(src.to_big(band.cells)), band.distances, cm.pack_bits(dst.shape, s), band.bg_out, band.bg_in)


def embed_field(windows, bands, fields):
    """The windows' velocities float32[n_w, 3] or speeds float32[n_w], each in its band's list order, in the big grid's list order: the
    order of `embed`."""
    check_disjoint(windows)
    for b, f in zip(bands, fields):
        _need(len(f) == b.cells.size, "a field has not one entry per cell")
    cells = np.concatenate([w.to_big(b.cells) for w, b in zip(windows, bands)])
    return np.concatenate([np.asarray(f, F) for f in fields])[np.argsort(cells, kind="stable")]


def _max_bits(values):
    """The largest of binary32 values that are not negative, by their bit patterns (+inf above every finite one)."""
    return np.array([F(v) for v in values], F).view(np.uint32).max().view(F)


def sum_advect(infos):
    """The Info of the big grid from the windows': the steps are the same, the maxima are taken on the bits, the counts add up."""
    _need(len({i.steps for i in infos}) == 1, "the windows ran different numbers of steps")
    return am.Info(infos[0].steps, _max_bits([i.max_change for i in infos]), _max_bits([i.max_cfl for i in infos]), sum(i.n_moving for i in infos),
                   sum(i.n_changed for i in infos), sum(i.n_sign_flips for i in infos), sum(i.n_nonfinite for i in infos))


def sum_select(infos):
    return ccm.SelectInfo(sum(i.n_cells for i in infos), sum(i.n_dropped for i in infos), sum(i.n_sign_cleared for i in infos))


def merge_components(windows, bands, comps):
    """The Components of the big grid from the windows' (`bands` gives each window's cells): the components are numbered by ascending
    first_cell converted to the big grid's L, the labels are renumbered so and put into the big grid's list order, lo and hi are
    shifted by the window's corner, n_cells and n_negative are carried over.  -> (Components, per window the big grid's number of each
    of its components)."""
    check_disjoint(windows)
    for w, b, c in zip(windows, bands, comps):
        _need(b.shape == w.shape and c.labels.size == b.cells.size, "a band is not on its window, or the labels are not the band's")
    first = np.concatenate([w.to_big(c.first_cell.astype(np.int64)) for w, c in zip(windows, comps)])
    order = np.argsort(first, kind="stable")
    number = np.empty(first.size, np.int64)
    number[order] = np.arange(first.size)
    ends = np.cumsum([0] + [c.count for c in comps])
    maps = [number[ends[x]:ends[x + 1]] for x in range(len(comps))]
    cells = np.concatenate([w.to_big(b.cells) for w, b in zip(windows, bands)])
    labels = np.concatenate([m[c.labels.astype(np.int64)] for m, c in zip(maps, comps)]).astype(np.uint32)[np.argsort(cells, kind="stable")]
    cat = lambda parts: np.concatenate(parts)[order]                                        # noqa: E731
    lo = cat([c.lo.astype(np.int64) + np.asarray(w.lo) for w, c in zip(windows, comps)]).astype(np.uint32).reshape(-1, 3)
    hi = cat([c.hi.astype(np.int64) + np.asarray(w.lo) for w, c in zip(windows, comps)]).astype(np.uint32).reshape(-1, 3)
    merged = ccm.Components(labels, int(first.size), first[order].astype(np.uint64), cat([c.n_cells for c in comps]), cat([c.n_negative for c in comps]), lo, hi)
    return merged, maps


def sum_redistance(infos):
    """The Info of the big grid from the windows': the sweeps that changed a value are the longest window's, the rest are sums."""
    return rm.Info(max(i.sweeps for i in infos), int(all(i.converged for i in infos)), sum(i.n_frozen for i in infos),
                   sum(i.n_open for i in infos), sum(i.n_candidates for i in infos))


def sum_filter(infos):
    return fm.Info(infos[0].passes, max(F(i.max_change) for i in infos), sum(i.n_changed for i in infos),
                   sum(i.n_sign_flips for i in infos), sum(i.n_nonfinite for i in infos))


# ---- resample: the sparse expectation -------------------------------------------------------------------------------------------------------
class SparseBits:
    """A sign mask uint32[nx, ny, ceil(nz / 32)] of a big grid that is zero outside a few windows, indexable as band_query_model.Band
    indexes its `bits`: [i, j, kw] with three equal-shaped integer arrays.  Nothing sized by the grid exists."""

    def __init__(self, windows, bands):
        check_disjoint(windows)
        self.parts = []
        for w, b in zip(windows, bands):
            sl = w.word_slices()
            zeros = np.zeros(tuple(x.stop - x.start for x in sl), np.uint32)
            self.parts.append((sl, w.put_bits(zeros, cm.unpack_bits(w.shape, b.bits))))

    def __getitem__(self, idx):
        i, j, kw = (np.asarray(x).astype(np.int64) for x in idx)
        out = np.zeros(i.shape, np.uint32)
        for sl, words in self.parts:
            m = (i >= sl[0].start) & (i < sl[0].stop) & (j >= sl[1].start) & (j < sl[1].stop) & (kw >= sl[2].start) & (kw < sl[2].stop)
            out[m] = words[i[m] - sl[0].start, j[m] - sl[1].start, kw[m] - sl[2].start]
        return out


def sparse_source(shape, cells, distances, bits, bg_out, bg_in):
    """The source of `resample_window`: a band_query_model.Band whose `bits` may be a SparseBits (or a dense array, or None)."""
    x = bqm.Band(shape, cells, distances, bg_out, bg_in, None if isinstance(bits, SparseBits) else bits)
    if isinstance(bits, SparseBits):
        x.bits = bits
    return x


def _sign_at(x, L):
    """s_X of the definition at the source cells L: active ? x < 0 : inside bit, from the sparse band alone."""
    val, active = x.lookup(L)
    inside = np.zeros(L.shape, bool)
    if x.bits is not None:
        nyz = x.n[1] * x.n[2]
        i, r = L // nyz, L % nyz
        j, k = r // x.n[2], r % x.n[2]
        inside = ((x.bits[i, j, k >> 5] >> (k & 31).astype(np.uint32)) & 1) == 1
    return np.where(active, val < 0, inside)


def resample_window(x, source, target, win, to_source=None, value_scale=1.0, mode=rsm.TRILINEAR, background=None):
    """band_resample_model.resample restated without any array sized by the source grid or by the target grid: the result on the window
    `win` of the target grid as (Band on win.shape, Info).  x: `sparse_source`; source, target: GridSpec.  The values and the support
    are band_query_model.sample's on the full-size source grid, the cell centres come from the absolute target indices
    (first + (float)i * size, as m2s_grid_cell_center), and s_X[c] is read sparsely.  The caller shows that no target point outside the
    window can be on the source box (`target_box_of_source`): there the result is inactive with a clear sign bit, and n_open needs the
    window's outermost layer on every interior side to be inactive, which is asserted here."""
    _need(win.big == tuple(int(n) for n in target.shape) and x.n == tuple(int(n) for n in source.shape), "the window or the band is on another grid")
    scale = F(value_scale)
    m = np.asarray(rsm.IDENTITY if to_source is None else to_source, F).reshape(12)
    with np.errstate(all="ignore"):
        bg_out, bg_in = (F(x.bg_out) * scale, F(-x.bg_in_neg) * scale) if background is None else (F(background[0]), F(background[1]))
    q = gqm.GridQ(source.first, source.cell, source.shape)
    ax = [(F(target.first[a]) + np.arange(win.lo[a], win.hi[a]).astype(F) * F(target.cell[a])).astype(F) for a in range(3)]
    centres = np.stack([c.reshape(-1) for c in np.meshgrid(*ax, indexing="ij")], 1)
    pts = rsm.source_points(centres, m)
    v, support = bqm.sample(q, x, pts, mode, 0.0, x.bg_out)
    with np.errstate(all="ignore"):
        r = (v * scale).astype(F)
    full = support == bqm.K_OF[mode]
    finite = np.isfinite(r)
    active = full & finite
    c, on = rsm.snap_cell(q, pts)
    s = np.where(active, r < 0, on & _sign_at(x, c))
    act3, s3 = active.reshape(win.shape), s.reshape(win.shape)
    for axis in range(3):
        for side in (0, 1):
            if not win.at_face(axis, side):
                _need(not _layers(act3, axis, side, 1).any() and not _layers(s3, axis, side, 1).any() and not _layers(on.reshape(win.shape), axis, side, 1).any(),
                      f"resample: the window's outermost layer on axis {axis} side {side} is on the source box")
    n_open = rm.frozen_set(act3, s3)[1]
    cells = np.flatnonzero(active)
    out = cm.Band(win.shape, cells, r[cells], cm.pack_bits(win.shape, s3), bg_out, bg_in)
    return out, rsm.Info(int(cells.size), int((on & (support > 0) & ~full).sum()), int((full & ~finite).sum()), n_open)


def target_box_of_source(source, target, forward, margin=2):
    """The window of the target grid that holds every target point whose source point can be on the source box: the images under the
    forward map (3 x 4, source space -> target space) of the corners of the source box grown by one cell, their bounding box in target
    indices (an affine image of a box lies in the hull of its corners' images), grown by `margin` cells against rounding and cut at the
    grid."""
    lo = [source.first[a] - 1.5 * source.cell[a] for a in range(3)]
    hi = [source.first[a] + (source.shape[a] + 0.5) * source.cell[a] for a in range(3)]
    M = np.asarray(forward, np.float64)
    img = np.array([M[:, :3] @ np.array([(lo, hi)[b][a] for a, b in enumerate(c)]) + M[:, 3] for c in np.ndindex(2, 2, 2)])
    idx = (img - np.asarray(target.first, np.float64)) / np.asarray(target.cell, np.float64)
    wlo = [max(int(np.floor(idx[:, a].min())) - margin, 0) for a in range(3)]
    whi = [min(int(np.ceil(idx[:, a].max())) + margin + 1, int(target.shape[a])) for a in range(3)]
    _need(all(h > l for l, h in zip(wlo, whi)), "the source box misses the target grid")
    return Window(target.shape, wlo, [h - l for l, h in zip(wlo, whi)])


# ---- layouts the CPU and the GPU tests share -----------------------------------------------------------------------------------------------
class Site(NamedTuple):
    """A window and, in its own coordinates, the box that holds every active cell of every band of the site."""
    window: Window
    box_lo: tuple
    box_shape: tuple


def site(big, box_lo, box_shape, margin):
    """The window of a box of the big grid: the box grown by `margin` layers per axis, cut at the grid's faces."""
    lo = tuple(max(b - m, 0) for b, m in zip(box_lo, margin))
    hi = tuple(min(b + s + m, n) for b, s, m, n in zip(box_lo, box_shape, margin, big))
    w = Window(big, lo, tuple(h - l for l, h in zip(lo, hi)))
    return Site(w, tuple(b - l for b, l in zip(box_lo, lo)), tuple(box_shape))


def redistance_margin(big, cell_size, exterior, interior):
    return tuple(max(rm.reach(w, cell_size[a], big[a]) for w in (exterior, interior)) + 1 for a in range(3))


def random_band(rng, st, offset, shape, scale, density=0.7, bg=(0.75, 0.5), force_first=False, force_last=False, half=None):
    """A random Band on the site's window: the points of the sub-box box_lo + offset, `shape` are active with probability `density`, with
    values uniform in [-scale, scale]; the sign bits are random inside the sub-box (on active points too, where no call reads them) and
    clear outside it.  force_first, force_last: the sub-box's first / last point is active.  half: only the sub-box's lower part along i, `half` layers
    thick, has its sign bits set instead of random ones (the region of a `where` band)."""
    w = st.window
    lo = tuple(b + o for b, o in zip(st.box_lo, offset))
    _need(all(o >= 0 and o + s <= bs for o, s, bs in zip(offset, shape, st.box_shape)), "the sub-box leaves the site's box")
    box = (slice(lo[0], lo[0] + shape[0]), slice(lo[1], lo[1] + shape[1]), slice(lo[2], lo[2] + shape[2]))
    act = np.zeros(w.shape, bool)
    act[box] = rng.random(shape) < density
    if force_first:
        act[lo] = True
    if force_last:
        act[lo[0] + shape[0] - 1, lo[1] + shape[1] - 1, lo[2] + shape[2] - 1] = True
    s = np.zeros(w.shape, bool)
    if half is None:
        s[box] = rng.random(shape) < 0.5
    else:
        s[lo[0]:lo[0] + half, box[1], box[2]] = True
    cells = np.flatnonzero(act.reshape(-1))
    values = (rng.uniform(-1, 1, cells.size) * scale).astype(F)
    return cm.Band(w.shape, cells, values, cm.pack_bits(w.shape, s), *bg)


class Layout(NamedTuple):
    big: tuple
    first: tuple
    cell: tuple
    widths: tuple            # ((exterior, interior), ...) of the redistance cases
    sites: tuple
    a: tuple                 # one Band per site: operand A, the input of redistance and filter
    b: tuple                 # operand B
    where: tuple             # the region of the restricted filter
    full: tuple              # nearly every point of the box active: the source of the interpolating resamples

    @property
    def windows(self):
        return [s.window for s in self.sites]

    @property
    def total(self):
        return self.big[0] * self.big[1] * self.big[2]


def layout(big, first, cell, box_los, widths, seed, box_shape=(9, 9, 11)):
    """Sites at `box_los` with margins for redistance at `widths`; A occupies the box less its first layers, B the box less its last
    layers: a box that ends with the grid makes A end with it (the grid's last cell is active in A), one at the origin makes B start with cell 0."""
    margin = tuple(max(m) for m in zip(*(redistance_margin(big, cell, e, i) for e, i in widths)))
    sites = tuple(site(big, lo, box_shape, margin) for lo in box_los)
    check_disjoint([s.window for s in sites])
    rng = np.random.default_rng(seed)
    sub = tuple(n - 1 for n in box_shape)
    scale = 0.8 * min(cell)
    a = tuple(random_band(rng, s, (1, 1, 1), sub, scale, force_last=True) for s in sites)
    b = tuple(random_band(rng, s, (0, 0, 0), sub, scale, density=0.6, bg=(0.5, 0.625), force_first=True) for s in sites)
    where = tuple(random_band(rng, s, (0, 0, 0), box_shape, scale, density=0.2, bg=(0.5, 0.5), half=box_shape[0] // 2) for s in sites)
    full = tuple(random_band(rng, s, (0, 0, 0), box_shape, scale, density=0.97) for s in sites)
    return Layout(tuple(big), tuple(first), tuple(cell), tuple(widths), sites, a, b, where, full)


# ---- components, select and advect: bands of several components and their fields -------------------------------------------------------------
SLABS = ((((0, 2), 0.2), ((3, 6), 0.85), ((7, 9), 0.2)),         # per site: the layers along i of the box that hold cells, and the share
         (((0, 2), 0.2), ((3, 5), 0.25), ((6, 9), 0.5)))         # of their points that is active


def blob_bands(lt, seed=0, slabs=SLABS):
    """One Band per site of many components: three slabs of the box along i with an empty layer between them, so that no two slabs
    touch under any connectivity.  A sparse slab (two points in ten active) falls into dozens of 6-components, about half as many
    18-components and fewer 26-components.  The first site's middle slab, dense and three layers thick, is around the layer of
    L = 2^32 on G33 and holds the largest component of all, with enough complete cells to be meshed and measured; the second site's
    box ends with the grid.  Values uniform in [-0.8, 0.8] min(cell); sign bits random in the box and clear outside it."""
    rng = np.random.default_rng(seed)
    out = []
    for st, layers in zip(lt.sites, slabs):
        w, lo, n = st.window, st.box_lo, st.box_shape
        _need(all(0 <= a < b <= n[0] for (a, b), _ in layers), "a slab leaves the site's box")
        act = np.zeros(w.shape, bool)
        for (a, b), density in layers:
            act[lo[0] + a:lo[0] + b, lo[1]:lo[1] + n[1], lo[2]:lo[2] + n[2]] = rng.random((b - a, n[1], n[2])) < density
        s = np.zeros(w.shape, bool)
        s[lo[0]:lo[0] + n[0], lo[1]:lo[1] + n[1], lo[2]:lo[2] + n[2]] = rng.random(n) < 0.5
        cells = np.flatnonzero(act.reshape(-1))
        out.append(cm.Band(w.shape, cells, (rng.uniform(-1, 1, cells.size) * 0.8 * min(lt.cell)).astype(F), cm.pack_bits(w.shape, s), 0.75, 0.5))
    return tuple(out)


def trig_field(win, band, kind, seed, still=0.25):
    """Velocities float32[n, 3] (am.VELOCITY) or speeds float32[n] for the cells of a Band on `win`: sines of the big grid's (i, j, k),
    in [-1, 1], with the share `still` of the cells, picked by a hash of the big grid's L, exactly zero."""
    rng = np.random.default_rng(seed)
    width = 3 if kind == am.VELOCITY else 1
    c, ph = rng.uniform(0.2, 0.9, (width, 3)), rng.uniform(0, 6, width)
    i, j, k = win.ijk(band.cells)
    f = np.stack([np.sin(c[x, 0] * i + c[x, 1] * j + c[x, 2] * k + ph[x]) for x in range(width)], 1).astype(F)
    h = (win.to_big(band.cells).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(44)
    f[(h % np.uint64(1024)).astype(np.int64) < still * 1024] = 0
    return f if width == 3 else f.reshape(-1)


def select_windows(lt, margin=(3, 3)):
    """Per site the window of whole rows over the box grown by `margin` layers in i and j, cut at the grid."""
    out = []
    for st in lt.sites:
        lo = [max(st.window.lo[a] + st.box_lo[a] - margin[a], 0) for a in range(2)]
        hi = [min(st.window.lo[a] + st.box_lo[a] + st.box_shape[a] + margin[a], lt.big[a]) for a in range(2)]
        out.append(row_window(lt.big, lo, [h - l for l, h in zip(lo, hi)]))
    check_disjoint(out)
    return out


def select_bands(lt, bands, runs, margin=(3, 3)):
    """The Bands of `blob_bands` on the windows of `select_windows`, with sign masks made for select: on every row through the box the
    bits of k in runs[site] = (from, to) are set, a long inside run whose inactive points look for their nearest active cell across
    many mask words (on active points no call reads the bit)."""
    out = []
    for st, band, win, (k0, k1) in zip(lt.sites, bands, select_windows(lt, margin), runs):
        s = np.zeros(win.shape, bool)
        lo = [st.window.lo[a] + st.box_lo[a] - win.lo[a] for a in range(2)]
        s[lo[0]:lo[0] + st.box_shape[0], lo[1]:lo[1] + st.box_shape[1], k0:k1] = True
        out.append(rehome(band, st.window, win, s))
    return out


def box_centre(lt, i):
    """The centre of site i's box in world coordinates (float64)."""
    st = lt.sites[i]
    return np.array([lt.first[a] + (st.window.lo[a] + st.box_lo[a] + (st.box_shape[a] - 1) / 2) * lt.cell[a] for a in range(3)])


def placement(lt, i):
    """Site i's resample case: band_resample_model.move()'s turn and scale about the centre of the box, with a sub-cell shift, as a
    forward map from the big grid's space, and a small grid around the moved centre that covers the moved box.
    -> (forward 3 x 4, its inverse 3 x 4, the small GridSpec)."""
    c = box_centre(lt, i)
    t = np.array([0.3 * lt.cell[0], 0.05 * lt.cell[1], 0.0])
    fwd = rsm.forward(rsm.MOVE_SCALE, rsm.rotation(rsm.MOVE_AXIS, rsm.MOVE_ANGLE), t, about=c)
    inv_a = np.linalg.inv(fwd[:, :3])
    inv = np.concatenate([inv_a, (-inv_a @ fwd[:, 3])[:, None]], 1)
    cell = tuple(0.8 * v for v in lt.cell)
    half = 0.5 * rsm.MOVE_SCALE * np.linalg.norm([n * h for n, h in zip(lt.sites[i].box_shape, lt.cell)])      # the moved box's half diagonal
    shape = tuple(int(np.ceil(2 * half / h)) + 4 for h in cell)
    centre = c + t
    small = rsm.GridSpec(tuple(float(centre[a] - (shape[a] - 1) * cell[a] / 2) for a in range(3)), cell, shape)
    return fwd, inv, small


def small_band(lt, i):
    """A random Band on site i's small grid (`placement`): nine points in ten active, random sign bits."""
    small = placement(lt, i)[2]
    rng = np.random.default_rng(1000 + i)
    total = small.shape[0] * small.shape[1] * small.shape[2]
    cells = np.flatnonzero(rng.random(total) < 0.9)
    bits = cm.pack_bits(small.shape, rng.random(small.shape) < 0.5)
    return cm.Band(small.shape, cells, (rng.uniform(-1, 1, cells.size) * 0.8 * min(lt.cell)).astype(F), bits, 0.75, 0.5)


def sign_band(band):
    """The Band with its sign mask replaced by s of the definition on every point (active ? x < 0 : inside bit)."""
    return cm.Band(band.shape, band.cells, band.distances, cm.pack_bits(band.shape, cm.dense(band)[2]), band.bg_out, band.bg_in)


def open_faces(band):
    """n_open of a Band: the sign changes from an active point towards an inactive axis neighbour."""
    act, _, s = cm.dense(band)
    return rm.frozen_set(act, s)[1]


# 2048 x 2048 x 1100 = 4.61e9 points; L = 2^32 is the point (1906, 1027, 796).  Cell sizes and first cell are dyadic, so that the cell
# centres first + (float)i * size are exact in binary32.
G33 = (2048, 2048, 1100)
G33_FIRST = (-8.0, -16.0, -2.0)
G33_CELL = (2.0 ** -7, 2.0 ** -6, 2.0 ** -8)
G33_WIDTHS = ((2.5 * 2.0 ** -7, 2.0 * 2.0 ** -7), (3.0 * 2.0 ** -7, 0.0))      # two-sided and one-sided, 2 to 3 cells of hx
G33_RUNS = ((200, 1000), (300, 1100))     # `select_bands`: inside runs of 800 points, 9 mask words below the first box and 3 above it, 12 below the second
# 4096 x 4096 x 1100 = 1.845e10 points, above 2^34: 288 358 400 mask words and 587 202 560 sign words, both above 2^28
G34 = (4096, 4096, 1100)
G34_FIRST = (-16.0, -32.0, -2.0)


def layout_g33():
    """One box across L = 2^32 and one that ends with the grid."""
    return layout(G33, G33_FIRST, G33_CELL, ((1902, 1023, 791), (2039, 2039, 1089)), G33_WIDTHS, 33)


def layout_g34():
    """One box at the origin and one that ends with the grid, where L > 2^34."""
    return layout(G34, G34_FIRST, G33_CELL, ((0, 0, 0), (4087, 4087, 1089)), G33_WIDTHS[:1], 34)
