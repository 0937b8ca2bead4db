"""The definition of m2s_band_resample (include/m2s.h) in numpy: a narrow band evaluated at the cell centres of another grid under a
3 x 4 map from target space to source space, per target grid point and to the bit.  It is built from the other models: the value and the
support are band_query_model.sample's, the SNAP cell and the box test grid_query_model's, the dense act / D' / s of the source
band_csg_model's, and n_open band_redistance_model.frozen_set's.  Everything is dense over the target, so it is for the small grids of
the tests; the library does the same with no array sized by either grid.

`resample` takes a `Band` of tests/band_csg_model.py and returns (Band, Info).  All arithmetic is IEEE binary32 without FMA, every
operation in the order written here."""
from typing import NamedTuple

import numpy as np

import band_query_model as bqm
import grid_query_model as gqm
from band_csg_model import F, Band, dense, pack_bits, same  # noqa: F401  (same: re-exported for the tests)
from band_redistance_model import frozen_set

SNAP, TRILINEAR, TETRAHEDRAL = gqm.SNAP, gqm.TRILINEAR, gqm.TETRAHEDRAL
MODES = (SNAP, TRILINEAR, TETRAHEDRAL)
IDENTITY = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)


class Info(NamedTuple):
    n_cells: int
    n_partial: int
    n_nonfinite: int
    n_open: int


class GridSpec(NamedTuple):
    """A grid as m2s_grid states it: first_cell, cell_size (binary32) and cell_count."""
    first: tuple
    cell: tuple
    shape: tuple


def centres(grid):
    """p = first_cell + (float)idx * cell_size per axis (m2s_grid_cell_center) at every point, float32[total, 3] in the order of L."""
    ax = [(F(grid.first[a]) + np.arange(grid.shape[a], dtype=F) * F(grid.cell[a])).astype(F) for a in range(3)]
    return np.stack([c.reshape(-1) for c in np.meshgrid(*ax, indexing="ij")], 1)


def source_points(p, to_source):
    """q_a = ((m[4a] * p.x + m[4a+1] * p.y) + m[4a+2] * p.z) + m[4a+3], a = 0, 1, 2."""
    m = np.asarray(to_source, F).reshape(12)
    with np.errstate(all="ignore"):
        return np.stack([((m[4 * a] * p[:, 0] + m[4 * a + 1] * p[:, 1]) + m[4 * a + 2] * p[:, 2]) + m[4 * a + 3] for a in range(3)], 1).astype(F)


def snap_cell(q, pts):
    """-> (c, on): the cell the SNAP rule of m2s_sample_grid reads for each point, and whether the point is on the box (c is 0 where not)."""
    on = gqm._state(q, pts) == 0
    pp = np.where(on[:, None], pts, q.start).astype(F)
    with np.errstate(all="ignore"):
        g = q.start - q.cs * F(0.5)
        idx = np.floor((pp - g) / q.cs).astype(np.int64)
    return gqm.cell_off(q, idx[:, 0], idx[:, 1], idx[:, 2]), on


def resample(band, source, target, to_source=None, value_scale=1.0, mode=TRILINEAR, background=None):
    """The result of m2s_band_resample as (Band, Info).  band: the source handle's lists on `source`; source, target: GridSpec;
    to_source: 12 numbers, row-major 3 x 4, target space -> source space (None: the identity); background: (outside, inside) of the
    result, None is the input's times value_scale."""
    if tuple(band.shape) != tuple(source.shape):
        raise ValueError("the band is not on the source grid")
    scale = F(value_scale)
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError("bad value_scale")
    m = np.asarray(IDENTITY if to_source is None else to_source, F).reshape(12)
    if not np.isfinite(m).all():
        raise ValueError("bad to_source")
    with np.errstate(all="ignore"):
        bg_out, bg_in = (F(band.bg_out) * scale, F(band.bg_in) * scale) if background is None else (F(background[0]), F(background[1]))
    if not (np.isfinite(bg_out) and np.isfinite(bg_in) and bg_out >= 0 and bg_in >= 0):
        raise ValueError("bad backgrounds")
    q = gqm.GridQ(source.first, source.cell, source.shape)
    x = bqm.Band(source.shape, band.cells, band.distances, band.bg_out, band.bg_in, band.bits)
    K = bqm.K_OF[mode]
    pts = source_points(centres(target), m)
    v, support = bqm.sample(q, x, pts, mode, 0.0, band.bg_out)
    with np.errstate(all="ignore"):
        r = (v * scale).astype(F)
    full = support == K
    finite = np.isfinite(r)
    active = full & finite
    c, on = snap_cell(q, pts)
    s_x = dense(band)[2].reshape(-1)
    s = np.where(active, r < 0, on & s_x[c])
    shape = tuple(int(n) for n in target.shape)
    n_open = frozen_set(active.reshape(shape), s.reshape(shape))[1]
    cells = np.flatnonzero(active)
    out = Band(shape, cells, r[cells], pack_bits(shape, s.reshape(shape)), bg_out, bg_in)
    return out, Info(int(cells.size), int((on & (support > 0) & ~full).sum()), int((full & ~finite).sum()), n_open)


def similarity(matrix):
    """BandField.resample's wrapper in float64: a 3 x 4 or 4 x 4 map p = A q + t from source space to target space with A^T A = s^2 I to
    a relative 1e-5 -> (to_source float32[12] = [A^T / s^2, -A^T t / s^2], value_scale float32 s).  Reflections pass; anything else raises."""
    M = np.asarray(matrix, np.float64)
    if M.shape == (4, 4):
        if not np.array_equal(M[3], (0, 0, 0, 1)):
            raise ValueError("the last row of a 4 x 4 transform must be (0, 0, 0, 1)")
        M = M[:3]
    if M.shape != (3, 4) or not np.isfinite(M).all():
        raise ValueError("the transform must be a finite 3 x 4 or 4 x 4 array")
    A, t = M[:, :3], M[:, 3]
    G = A.T @ A
    s2 = np.trace(G) / 3
    if not s2 > 0 or np.abs(G - s2 * np.eye(3)).max() > 1e-5 * s2:
        raise ValueError("the transform is not a similarity (A^T A = s^2 I)")
    inv = A.T / s2
    return np.concatenate([inv, (-inv @ t)[:, None]], 1).astype(F).reshape(12), F(np.sqrt(s2))


def rotation(axis, angle):
    """Rodrigues' formula in float64."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def forward(scale, R, t, about=(0, 0, 0)):
    """p = scale * R (q - about) + about + t as a 3 x 4 float64 array."""
    A = scale * np.asarray(R, np.float64)
    about = np.asarray(about, np.float64)
    return np.concatenate([A, (about + np.asarray(t, np.float64) - A @ about)[:, None]], 1)


# ---- inputs the tests share ------------------------------------------------------------------------------------------------------------
def centred(shape, cell):
    """The grid of `shape` cells of `cell` centred on the origin, as band_redistance_model's is."""
    return GridSpec(tuple(-(n - 1) * c / 2 for n, c in zip(shape, cell)), tuple(cell), tuple(shape))


MOVE_SCALE, MOVE_AXIS, MOVE_ANGLE, MOVE_T = 0.75, (1, 2, 3), 0.7, (0.3, 0.05, 0.0)


def move():
    """The accuracy test's forward map: scale 0.75, a turn of 0.7 rad about (1, 2, 3) / sqrt(14), then t = (0.3, 0.05, 0)."""
    return forward(MOVE_SCALE, rotation(MOVE_AXIS, MOVE_ANGLE), MOVE_T)
