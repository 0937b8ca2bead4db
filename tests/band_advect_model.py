"""The definition of m2s_band_advect (include/m2s.h) in numpy: the values of a narrow band moved by first-order upwind steps of
phi_t + u . grad phi = 0 (a velocity per cell) or phi_t + F |grad phi| = 0 (a normal speed per cell, Godunov), per grid point and to
the bit.  Everything is built densely (the grid D' the band stands for, padded with its own edge values), so it is for the small grids
of the tests; the library does the same with no array sized by the grid.

`band_advect` takes a `Band` of tests/band_csg_model.py and a field in list order and returns (Band, Info).  All arithmetic is IEEE
binary32 without FMA, every operation in the order written here; every step is Jacobi (each new value from the previous step's values
only), which the bits depend on."""
from typing import NamedTuple

import numpy as np

from band_csg_model import F, Band, dense, pack_bits, same  # noqa: F401  (same: re-exported for the tests)
from band_filter_model import neighbours, step_of, x_crossings  # noqa: F401  (x_crossings: re-exported for the tests)
from band_redistance_model import redistance

VELOCITY, NORMAL = 0, 1
KINDS = (VELOCITY, NORMAL)


class Info(NamedTuple):
    steps: int
    max_change: float          # a binary32 value (np.float32); +inf is possible
    max_cfl: float             # a binary32 value; +inf is possible
    n_moving: int
    n_changed: int
    n_sign_flips: int
    n_nonfinite: int


def rates(cell_size):
    """The host constants r_a = 1 / h_a in binary32."""
    return tuple(F(1) / F(v) for v in cell_size)


def moving_of(field, kind):
    """Per cell: any velocity component != 0, or the speed != 0.  A NaN counts as moving (NaN != 0)."""
    return (field != 0).any(axis=1) if kind == VELOCITY else field != 0


def cfl_of(field, kind, dt, r):
    """max_cfl: the maximum of the bit patterns of the per-cell figures that are not NaN; 0 for no cell."""
    with np.errstate(all="ignore"):
        a = np.abs(field)
        if kind == VELOCITY:
            c = F(dt) * ((a[:, 0] * r[0] + a[:, 1] * r[1]) + a[:, 2] * r[2])
        else:
            c = F(dt) * (a * ((r[0] + r[1]) + r[2]))
    c = c.astype(F)
    c = c[~np.isnan(c)]
    return F(c.max()) if c.size else F(0)


def candidate(v, kind, fld, dt, r):
    """cand of one step on every grid point (the caller keeps it on the moving cells).  fld: the dense field, [nx, ny, nz, 3] or
    [nx, ny, nz], anything on the points that do not move."""
    N = neighbours(v)
    c = v
    dt = F(dt)
    zero = F(0)
    with np.errstate(all="ignore"):
        Dm = [(c - N(*step_of(a, -1))) * r[a] for a in range(3)]
        Dp = [(N(*step_of(a, 1)) - c) * r[a] for a in range(3)]
        if kind == VELOCITY:
            t = [np.where(fld[..., a] > 0, fld[..., a] * Dm[a], fld[..., a] * Dp[a]).astype(F) for a in range(3)]
            return (c - dt * ((t[0] + t[1]) + t[2])).astype(F)
        grow = fld > 0
        q = []
        for a in range(3):
            pos_m, neg_m = np.where(Dm[a] > 0, Dm[a], zero), np.where(Dm[a] < 0, Dm[a], zero)
            pos_p, neg_p = np.where(Dp[a] > 0, Dp[a], zero), np.where(Dp[a] < 0, Dp[a], zero)
            A = np.where(grow, pos_m, neg_m).astype(F)
            B = np.where(grow, neg_p, pos_p).astype(F)
            qa, qb = A * A, B * B
            q.append(np.where(qb > qa, qb, qa).astype(F))
        g = np.sqrt((q[0] + q[1]) + q[2]).astype(F)
        return (c - dt * (fld * g)).astype(F)


def band_advect(band, cell_size, kind, field, dt, steps=1, background=None):
    """The result of m2s_band_advect as (Band, Info).  field: float32[n, 3] (VELOCITY) or [n] (NORMAL) in the order of band.cells.
    background: (outside, inside) of the result; None is the input's."""
    dt = F(dt)
    if kind not in KINDS or not 1 <= steps <= 65536 or not (np.isfinite(dt) and dt > 0):
        raise ValueError("bad kind, steps or dt")
    n = band.cells.size
    field = np.zeros((0, 3) if kind == VELOCITY else 0, F) if field is None else np.asarray(field, F)
    field = field.reshape((n, 3) if kind == VELOCITY else (n,))
    r = rates(cell_size)
    act, x, s = dense(band)
    with np.errstate(invalid="ignore"):
        mv = moving_of(field, kind)
    moving = np.zeros(band.total, bool)
    moving[band.cells] = mv
    moving = moving.reshape(band.shape)
    fld = np.zeros((band.total,) + field.shape[1:], F)
    fld[band.cells] = field
    fld = fld.reshape(band.shape + field.shape[1:])
    v = x.copy()
    n_nonfinite = 0
    if n:
        for _ in range(steps):
            cand = candidate(v, kind, fld, dt, r)
            ok = np.isfinite(cand)
            n_nonfinite += int((moving & ~ok).sum())
            v = np.where(moving & ok, cand, v).astype(F)
    res = v.reshape(-1)[band.cells]
    x0 = x.reshape(-1)[band.cells]
    with np.errstate(all="ignore"):
        change = np.abs(res - x0)
    info = Info(steps, F(change.max()) if n else F(0), cfl_of(field, kind, dt, r), int(mv.sum()),
                int((res.view(np.uint32) != x0.view(np.uint32)).sum()), int(((res < 0) != (x0 < 0)).sum()), n_nonfinite)
    bg_out, bg_in = (band.bg_out, band.bg_in) if background is None else background
    return Band(band.shape, band.cells, res, pack_bits(band.shape, np.where(act, v < 0, s)), bg_out, bg_in), info


def centers(band, first, cell_size):
    """The band's cell centres float32[n, 3] in list order: first_cell + (float)idx * cell_size per axis (m2s_grid_cell_center)."""
    nx, ny, nz = band.shape
    L = band.cells
    idx = (L // (ny * nz), (L // nz) % ny, L % nz)
    return np.stack([F(first[a]) + idx[a].astype(F) * F(cell_size[a]) for a in range(3)], 1).astype(F)


# ---- the tracker and the measurements the tests and DESIGN.md 4.24 share ------------------------------------------------------------------
def flow(band, first, cell_size, time, width, kind, field_of, cfl=0.5, reach=1.0):
    """BandField.flow in the models: per round the field on the cells' centres (field_of(centers) -> float32[n, 3] or float32[n]),
    the library's schedule (mesh_to_sdf_amd.flow_round), band_advect, then the redistance model to the half-widths `width`.
    -> (Band, rounds, steps, [n_open of every round])."""
    from mesh_to_sdf_amd import flow_round

    left, rounds, steps, opens = float(time), 0, 0, []
    while left > 0 and band.cells.size:
        field = np.asarray(field_of(centers(band, first, cell_size)), F)
        n_steps, dt, took = flow_round(field, kind, cell_size, left, cfl, reach)
        if n_steps == 0:
            break
        moved, _ = band_advect(band, cell_size, kind, field, dt, n_steps)
        band, rinfo = redistance(moved, cell_size, width, width)
        opens.append(rinfo.n_open)
        rounds, steps = rounds + 1, steps + n_steps
        left = 0.0 if took >= left else left - took
    return band, rounds, steps, opens


def sphere_error(band, first, cell_size, centre, radius):
    """The largest | |p - centre| - radius | over the zero crossings p along x grid lines, in cells of h_x, and their number."""
    p = x_crossings(band, first, cell_size)
    dev = np.abs(np.linalg.norm(p - np.asarray(centre, np.float64), axis=1) - radius)
    return float(dev.max() / cell_size[0]), p.shape[0]
