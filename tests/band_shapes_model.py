"""m2s_band_from_capsules in numpy: include/m2s.h's definition (mesh_to_sdf_amd/csrc/shape.hip.h holds it with its error bound), brute
force over all grid points and all shapes, in float32 with the header's order of operations.

    ab = b - a;  ap = c - a;  den = (ab.x*ab.x + ab.y*ab.y) + ab.z*ab.z
    t  = den > 0 ? clamp(((ap.x*ab.x + ap.y*ab.y) + ap.z*ab.z) / den, 0, 1) : 0
    e  = ap - t*ab
    d_s = sqrt((e.x*e.x + e.y*e.y) + e.z*e.z) - r
    D = the minimum of d_s over the sound shapes; active iff -interior <= D <= exterior; sign bit D < 0 on every point.

numpy's float32 add, subtract, multiply, divide and sqrt are the correctly rounded IEEE operations and nothing here is fused.  A shape is
sound when its seven numbers are finite and r >= 0.  A d_s that is NaN (overflowing differences) takes no part: the minimum is np.fmin.
`run` takes an optional window (lo, shape) of the grid, so that a test on a grid of 2^32 points evaluates a corner of it: the cell centres
come from the absolute indices."""
from typing import NamedTuple

import numpy as np

F = np.float32
U = 2.0 ** -24
ERR_U = 96.0          # shape.hip.h's SHAPE_ERR_U: |d_s - true| <= ERR_U * U * scale


def sound(a, b, r):
    a, b, r = np.asarray(a, F).reshape(-1, 3), np.asarray(b, F).reshape(-1, 3), np.asarray(r, F).reshape(-1)
    return np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(r) & (r >= 0)


def dist(a, b, r, c):
    """d_s of one shape (a, b: 3 floats, r) at the points c = (cx, cy, cz), arrays of one shape, or of shapes a[n], b[n], r[n] at
    points of n rows: everything broadcasts.  float32 in, float32 out."""
    ax, ay, az = (F(1) * np.asarray(a, F)[..., m] for m in range(3))
    bx, by, bz = (F(1) * np.asarray(b, F)[..., m] for m in range(3))
    cx, cy, cz = (np.asarray(v, F) for v in c)
    r = np.asarray(r, F)
    with np.errstate(all="ignore"):
        abx, aby, abz = bx - ax, by - ay, bz - az
        apx, apy, apz = cx - ax, cy - ay, cz - az
        den = (abx * abx + aby * aby) + abz * abz
        num = (apx * abx + apy * aby) + apz * abz
        pos = den > 0
        t = np.where(pos, num / np.where(pos, den, F(1)), F(0)).astype(F)
        t = np.where(pos, np.where(t < 0, F(0), np.where(t > 1, F(1), t)), F(0)).astype(F)
        ex, ey, ez = apx - t * abx, apy - t * aby, apz - t * abz
        d = np.sqrt((ex * ex + ey * ey) + ez * ez) - r
    assert d.dtype == F
    return d


def centres(first, cell, lo, shape):
    """The float32 cell centres first + (float)index * size of the window's indices, per axis."""
    return [(F(first[m]) + np.arange(lo[m], lo[m] + shape[m]).astype(F) * F(cell[m])).astype(F) for m in range(3)]


class Result(NamedTuple):
    shape: tuple          # the window's (the grid's without a window)
    active: np.ndarray    # bool[shape]
    D: np.ndarray         # float32[shape], +inf where no shape is
    inside: np.ndarray    # bool[shape]: D < 0
    cells: np.ndarray     # int64, the window's own L = k + j nz + i ny nz of the active points, ascending
    values: np.ndarray    # float32, D there
    n_inside: int
    n_skipped: int
    n_off_grid: int       # sound shapes with no point of the window at d_s <= exterior
    near: np.ndarray      # bool[n]: the shape has such a point


def run(first, cell, shape, a, b, r, exterior, interior, window=None):
    a = np.asarray(a, F).reshape(-1, 3)
    b = a if b is None else np.asarray(b, F).reshape(-1, 3)
    r = np.full(a.shape[0], r, F) if np.isscalar(r) else np.asarray(r, F).reshape(-1)
    lo, wshape = ((0, 0, 0), tuple(shape)) if window is None else window
    cx, cy, cz = np.meshgrid(*centres(first, cell, lo, wshape), indexing="ij")
    ok = sound(a, b, r)
    D = np.full(wshape, np.inf, F)
    near = np.zeros(a.shape[0], bool)
    ext, neg_int = F(exterior), -F(interior)
    for s in np.flatnonzero(ok):
        d = dist(a[s], b[s], r[s], (cx, cy, cz))
        near[s] = bool((d <= ext).any())
        D = np.fmin(D, d)
    active = (D >= neg_int) & (D <= ext)
    inside = D < 0
    cells = np.flatnonzero(active.reshape(-1)).astype(np.int64)
    return Result(tuple(wshape), active, D, inside, cells, D.reshape(-1)[cells], int(inside.sum()), int((~ok).sum()), int((ok & ~near).sum()), near)


def pack_bits(inside):
    """bool[nx, ny, nz] -> uint32[nx, ny, ceil(nz / 32)], the layout of Voxels.bits."""
    nx, ny, nz = inside.shape
    pad = np.zeros((nx, ny, (nz + 31) // 32 * 32), bool)
    pad[:, :, :nz] = inside
    w = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    return (pad.reshape(nx, ny, -1, 32).astype(np.uint64) * w).sum(-1).astype(np.uint32)


def dist64(a, b, r, c):
    """The distance in float64 from the float32 inputs, for the error bound: exact up to float64 rounding."""
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    r = np.asarray(r, F).astype(np.float64)
    ab, ap = b - a, c - a
    den = (ab * ab).sum(-1)
    t = np.clip((ap * ab).sum(-1) / np.where(den > 0, den, 1.0), 0.0, 1.0) * (den > 0)
    e = ap - t[..., None] * ab
    return np.sqrt((e * e).sum(-1)) - r
