"""The definition of m2s_band_csg (include/m2s.h) in numpy: union, intersection and difference of two narrow bands on one grid, per grid
point and to the bit.  Everything is built densely (act, D' and s of both operands), so it is for the small grids of the tests; the
library does the same with no array sized by the grid.

A band is a `Band`: the grid's shape, its cells (ascending L = k + j*nz + i*ny*nz), their float32 distances, its sign mask in the
caller's layout uint32[nx, ny, ceil(nz / 32)] or None, and its two backgrounds.  `csg` returns the result as a Band: cells ascending,
distances, a sign mask equal to s on every grid point (bits at k >= nz zero) and the backgrounds."""
import numpy as np

F = np.float32
UNION, INTERSECTION, DIFFERENCE = 0, 1, 2


class Band:
    def __init__(self, shape, cells, distances, bits, bg_out, bg_in):
        self.shape = tuple(int(c) for c in shape)
        self.cells = np.asarray(cells).astype(np.int64).reshape(-1)
        self.distances = np.asarray(distances, F).reshape(-1)
        nx, ny, nz = self.shape
        self.bits = None if bits is None else np.asarray(bits).astype(np.uint32).reshape(nx, ny, (nz + 31) // 32)
        self.bg_out, self.bg_in = F(bg_out), F(bg_in)

    @property
    def total(self):
        return self.shape[0] * self.shape[1] * self.shape[2]


def unpack_bits(shape, bits):
    """uint32[nx, ny, ceil(nz / 32)] -> bool[nx, ny, nz]; None is all False."""
    nx, ny, nz = shape
    if bits is None:
        return np.zeros(shape, bool)
    k = np.arange(nz)
    return ((np.asarray(bits, np.uint32).reshape(nx, ny, -1)[:, :, k >> 5] >> (k & 31).astype(np.uint32)) & 1).astype(bool)


def pack_bits(shape, s):
    """bool[nx, ny, nz] -> uint32[nx, ny, ceil(nz / 32)], cell k of a row in bit k & 31 of word k >> 5, the bits at k >= nz zero."""
    nx, ny, nz = shape
    nzw = (nz + 31) // 32
    padded = np.zeros((nx, ny, nzw * 32), np.uint64)
    padded[:, :, :nz] = np.asarray(s, bool).reshape(shape)
    weights = np.uint64(1) << np.arange(32, dtype=np.uint64)
    return (padded.reshape(nx, ny, nzw, 32) * weights).sum(-1).astype(np.uint32)


def dense(band):
    """-> (act bool, D' float32, s bool), each [nx, ny, nz]: the mask, the grid the band stands for and the sign of the definition."""
    act = np.zeros(band.total, bool)
    act[band.cells] = True
    inside = unpack_bits(band.shape, band.bits).reshape(-1)
    d = np.where(inside, -band.bg_in, band.bg_out).astype(F)
    d[band.cells] = band.distances
    s = np.where(act, d < 0, inside)
    return act.reshape(band.shape), d.reshape(band.shape), s.reshape(band.shape)


def negate(band):
    """-X: the values' sign bits flipped, the same cells, the complement of the sign mask, the backgrounds swapped."""
    flipped = (band.distances.view(np.uint32) ^ np.uint32(0x80000000)).view(F)
    return Band(band.shape, band.cells, flipped, pack_bits(band.shape, ~unpack_bits(band.shape, band.bits)), band.bg_in, band.bg_out)


def select(op, a, b, act_a=None):
    """op of two dense grids as the definition selects it: r = pickB ? b : a, every bit.  act_a None: A counts as active everywhere
    (a tie takes a's bits)."""
    first = (b < a) if op == UNION else (b > a)
    tie = (a == b) & (~act_a if act_a is not None else False)
    return np.where(first | tie, b, a).astype(F)


def csg(a, b, op, background=None):
    """The result of m2s_band_csg(a, b, op) as a Band.  background: (outside, inside) of the result; None is the min rule."""
    if a.shape != b.shape:
        raise ValueError("the bands' grids differ")
    if op == DIFFERENCE:
        return csg(a, negate(b), INTERSECTION, background)
    if op not in (UNION, INTERSECTION):
        raise ValueError("bad op")
    act_a, da, sa = dense(a)
    act_b, db, sb = dense(b)
    if op == UNION:
        b_first, a_first = db < da, da < db
        s = sa | sb
    else:
        b_first, a_first = db > da, da > db
        s = sa & sb
    r = select(op, da, db, act_a)
    active = (act_a & ~b_first) | (act_b & ~a_first)
    cells = np.flatnonzero(active.reshape(-1))
    bg_out, bg_in = (min(a.bg_out, b.bg_out), min(a.bg_in, b.bg_in)) if background is None else background
    return Band(a.shape, cells, r.reshape(-1)[cells], pack_bits(a.shape, s), bg_out, bg_in)


def same(x, y):
    """Two Bands agree in every bit: cells, distances, sign mask (None is not a mask of zeros), backgrounds."""
    return (x.shape == y.shape and np.array_equal(x.cells, y.cells) and np.array_equal(x.distances.view(np.uint32), y.distances.view(np.uint32))
            and (x.bits is None) == (y.bits is None) and (x.bits is None or np.array_equal(x.bits, y.bits))
            and x.bg_out.view(np.uint32) == y.bg_out.view(np.uint32) and x.bg_in.view(np.uint32) == y.bg_in.view(np.uint32))
