"""Random chains of band calls and their reference: the chained numpy models.

Every band model maps a band_csg_model.Band to a Band, to the bit, so a chain of model calls is the definition of the same chain of
library calls.  This module draws the chains and replays them through the models; tests/test_band_chain_cpu.py checks that the chains
reach what they are meant to reach, tests/test_gpu_band_chain.py replays them through the library.  No arithmetic of its own: the
values come from band_csg_model.csg, band_filter_model.band_filter, band_redistance_model.redistance, band_resample_model.resample (with
.similarity) and band_components_model.components / .select.

A chain lives on a PAIR of grids that differ in first cell, cell size and cell count, so that `resample` changes grid; each grid has a
POOL of four start bands, which are also the partners of `csg` and the regions of `filter`.  `plan(seed, pair)` is plain data (tuples,
numbers, names), a pure function of its arguments; what a step needs of the grid it happens to run on (widths in world units, the map
between the two grids, the keep mask over however many components there are) is resolved at replay by `widths`, `forward_of` and
`keep_of`, which both sides call.

There are two families of chains.  The first (`OPS`, `SALT`, `SEEDS`, `draw`, `plan`, `chain`) is the one the suite began with and
stays exactly as it was: `draw` picks OPS[rng.integers(len(OPS))], so a sixth op in OPS would change every chain.  The second
(`OPS_B`, `SALT_B`, `SEEDS_B`, `draw_b`, `plan_b`, `chain_b`) has a generator stream of its own and `advect` as a sixth op
(band_advect_model.band_advect); its five old ops draw their arguments as in the first.  An advect step's velocities or speeds and its
time step depend on the cells it meets, so they too are resolved at replay, by `field_of` and `dt_of`."""
import functools
from typing import NamedTuple

import numpy as np

import band_advect_model as am
import band_components_model as ccm
import band_csg_model as cm
import band_filter_model as fm
import band_redistance_model as rm
import band_resample_model as rsm

F = np.float32
FMAX = np.finfo(F).max
STEPS = 8
SALT = 3            # of the generator's streams, one whose 36 chains meet every condition of tests/test_band_chain_cpu.py with a margin
SEEDS = tuple(range(12))
OPS = ("csg", "filter", "redistance", "resample", "select")
CSG_NAMES = ("union", "intersection", "difference")
# the second family: the same pairs and pools, the six ops, 16 seeds per pair (384 steps) so that each op still meets 40 non-empty inputs
OPS_B = OPS + ("advect",)
SALT_B = 4          # of the streams default_rng([salt, seed, pair, 6]) with salt 0 .. 7, the one whose 48 chains meet every condition of
#                     tests/test_band_chain_cpu.py with the widest margin: every op on 48 non-empty inputs or more, every rare branch 7 times or more
SEEDS_B = tuple(range(16))
ADVECT_NAMES = ("velocity", "normal speed")


def _around(centre, cell, shape):
    return rsm.GridSpec(tuple(float(centre[a] - (shape[a] - 1) * cell[a] / 2) for a in range(3)), tuple(cell), tuple(shape))


# The two grids of a pair cover about the same box with different cells, so that a resampled band lands on the other grid's cells.
# (2,2,2) + (3,65,1): every read clamped, nz = 1.  (9,7,70) + (13,11,37): rows that straddle mask words, totals that are no multiple
# of 64.  (24,20,28) + (5,3,70): several walk units.  All six are in the SHAPES lists of the per-call band tests.
PAIRS = ((_around((0.1, -0.2, 0.3), (0.5, 0.4, 0.45), (2, 2, 2)), _around((0.16, -0.13, 0.27), (0.3, 0.0125, 0.8), (3, 65, 1))),
         (_around((0.1, -0.2, 0.3), (0.25, 0.3, 0.05), (9, 7, 70)), _around((0.16, -0.13, 0.27), (0.17, 0.19, 0.09), (13, 11, 37))),
         (_around((0.1, -0.2, 0.3), (0.1, 0.12, 0.09), (24, 20, 28)), _around((0.16, -0.13, 0.27), (0.45, 0.7, 0.035), (5, 3, 70))))
PAIR_IDS = tuple("+".join("x".join(map(str, g.shape)) for g in pair) for pair in PAIRS)
POOL_NAMES = ("smooth", "smooth, no mask", "thin, 20 % knocked out", "noise")


def centre(spec):
    return np.array([spec.first[a] + (spec.shape[a] - 1) * spec.cell[a] / 2 for a in range(3)], np.float64)


def _trig(rng, shape):
    """A random low-order trigonometric field over the cell indices, as _smooth_band of tests/test_gpu_band_filter.py."""
    i, j, k = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    a = rng.uniform(0.2, 0.9, 3)
    d = (np.sin(a[0] * i + rng.uniform(0, 6)) + np.sin(a[1] * j + rng.uniform(0, 6)) + np.sin(a[2] * k + rng.uniform(0, 6))).astype(F) * F(0.2)
    return d.reshape(-1)


@functools.lru_cache(maxsize=None)
def pool(pair, g):
    """The four start bands of grid g (0 or 1) of PAIRS[pair], made once and never changed."""
    shape = PAIRS[pair][g].shape
    total = shape[0] * shape[1] * shape[2]
    rng = np.random.default_rng([77, pair, g])
    d = _trig(rng, shape)
    # smooth: |d| <= 0.3, one cell in ten knocked out, but none within 0.2 of the zero set: a step changes d by less than 0.18, so every
    # sign change lies between two active cells and redistance finds n_open == 0 on it
    cells = np.flatnonzero((np.abs(d) <= 0.3) & ((np.abs(d) < 0.2) | (rng.random(total) < 0.9)))
    smooth = cm.Band(shape, cells, d[cells], cm.pack_bits(shape, (d < 0).reshape(shape)), 0.75, 0.5)
    # the same without a mask, where everything beyond the band counts as outside: raised by 0.35 the field stays above -0.3, so the
    # band holds its whole negative region and is closed in the same sense
    d2 = _trig(rng, shape) + F(0.35)
    cells = np.flatnonzero((np.abs(d2) <= 0.3) & ((d2 < 0.2) | (rng.random(total) < 0.9)))
    plain = cm.Band(shape, cells, d2[cells], None, 0.75, 0.5)
    d3 = _trig(rng, shape)
    cells = np.flatnonzero((np.abs(d3) <= 0.15) & (rng.random(total) < 0.8))
    thin = cm.Band(shape, cells, d3[cells], cm.pack_bits(shape, (d3 < 0).reshape(shape)), 0.75, 0.5)
    cells = np.flatnonzero(rng.random(total) < 0.5)
    v = rng.uniform(-1, 1, cells.size).astype(F)
    pick = rng.random(cells.size) < 0.05
    v[pick] = rng.choice(np.array([0.0, -0.0, FMAX, -FMAX], F), int(pick.sum()))
    mask = rng.integers(0, 2 ** 32, (shape[0], shape[1], (shape[2] + 31) // 32), dtype=np.uint64).astype(np.uint32)
    noise = cm.Band(shape, cells, v, mask, 0.75, 0.5)
    return smooth, plain, thin, noise


def _floats(x):
    return tuple(float(v) for v in x)


def _draw_step(rng, ops):
    """One step with its op drawn from `ops`; the five ops of OPS take the same numbers from the generator in both families."""
    op = ops[int(rng.integers(len(ops)))]
    if op == "csg":
        return (op, ("partner", int(rng.integers(4))), ("swap", bool(rng.integers(2))), ("kind", int(rng.integers(3))))
    if op == "filter":
        where = int(rng.integers(5))
        bg = _floats(rng.uniform(0.1, 2.0, 2)) if rng.integers(2) else None
        return (op, ("kind", int(rng.integers(3))), ("iterations", int(rng.integers(1, 4))), ("where", None if where == 4 else where),
                ("background", bg))
    if op == "redistance":
        return (op, ("exterior", float(rng.uniform(1, 3))), ("interior", float(rng.uniform(1, 3))))
    if op == "resample":
        return (op, ("target", int(rng.integers(2))), ("scale", float(rng.uniform(0.9, 1.1))), ("axis", _floats(rng.normal(size=3))),
                ("angle", float(rng.uniform(-0.3, 0.3))), ("jitter", _floats(rng.uniform(-0.5, 0.5, 3))), ("mode", int(rng.integers(3))))
    if op == "select":
        return (op, ("connectivity", int(ccm.CONNECTIVITIES[int(rng.integers(3))])), ("keep_u", _floats(rng.random(32))))
    # advect: 9 frequencies and 3 phases of `field_of`, the share of cells at rest, the CFL fraction of `dt_of`
    coef = _floats(rng.uniform(0.2, 0.9, 9)) + _floats(rng.uniform(0, 6, 3))
    bg = _floats(rng.uniform(0.1, 2.0, 2)) if rng.integers(2) else None
    return (op, ("kind", int(rng.integers(2))), ("steps", int(rng.integers(1, 4))), ("cfl", float(rng.uniform(0.2, 0.9))), ("coef", coef),
            ("still", float(rng.uniform(0, 0.5))), ("background", bg))


def _draw(rng, ops):
    start = (int(rng.integers(2)), int(rng.integers(4)))
    return start, tuple(_draw_step(rng, ops) for _ in range(STEPS))


@functools.lru_cache(maxsize=None)
def draw(seed, pair):
    """-> ((start grid, start pool band), the 8 steps), from default_rng([SALT, seed, pair]) alone."""
    return _draw(np.random.default_rng([SALT, int(seed), int(pair)]), OPS)


@functools.lru_cache(maxsize=None)
def draw_b(seed, pair):
    """The second family's `draw`: the six ops of OPS_B, from default_rng([SALT_B, seed, pair, 6]) alone."""
    return _draw(np.random.default_rng([SALT_B, int(seed), int(pair), 6]), OPS_B)


def plan(seed, pair):
    """The 8 steps of chain `seed` on PAIRS[pair]: (op, (argument, value), ...) each, plain data."""
    return list(draw(seed, pair)[1])


def start_of(seed, pair):
    """(grid, pool band) the chain starts from."""
    return draw(seed, pair)[0]


def plan_b(seed, pair):
    return list(draw_b(seed, pair)[1])


def start_of_b(seed, pair):
    return draw_b(seed, pair)[0]


def args(step):
    return dict(step[1:])


def describe(step):
    a = args(step)
    if step[0] == "csg":
        return f"csg {CSG_NAMES[a['kind']]} with pool band {a['partner']}" + (" as the first operand" if a["swap"] else "")
    if step[0] == "select":
        return f"select connectivity {a['connectivity']}"
    if step[0] == "advect":
        return f"advect by a {ADVECT_NAMES[a['kind']]}, {a['steps']} steps, CFL fraction {a['cfl']:.3f}, {a['still']:.2f} at rest, background {a['background']}"
    return step[0] + " " + ", ".join(f"{k} {v}" for k, v in a.items())


# ---- what a step needs of the grid it runs on, for both sides -------------------------------------------------------------------------------
def widths(step, spec):
    """redistance: (exterior, interior) in world units, the drawn factors times the largest cell side."""
    a = args(step)
    h = max(spec.cell)
    return a["exterior"] * h, a["interior"] * h


def forward_of(step, src, tgt):
    """resample: the 3 x 4 float64 map from source space to target space: scale and turn about the source grid's centre, which goes to
    the target grid's centre plus the drawn fraction of a target cell."""
    a = args(step)
    t = centre(tgt) - centre(src) + np.asarray(a["jitter"]) * np.asarray(tgt.cell, np.float64)
    return rsm.forward(a["scale"], rsm.rotation(a["axis"], a["angle"]), t, about=centre(src))


def keep_of(step, n_cells):
    """select: the boolean keep mask over the components whose cell counts are n_cells: component c stays with probability 0.7 (the
    drawn numbers, taken round), the largest (the lowest-numbered of equals) always."""
    u = np.asarray(args(step)["keep_u"])
    count = len(n_cells)
    keep = u[np.arange(count) % u.size] < 0.7
    if count:
        keep[int(np.argmax(np.asarray(n_cells).astype(np.int64)))] = True
    return keep


def field_of(step, band, spec):
    """advect: the velocities float32[n, 3] (kind 0) or normal speeds float32[n] (kind 1) on the cells of `band`, in list order: one
    sine of the cell's (i, j, k) per component, so every entry lies in [-1, 1], evaluated in float64 and rounded to binary32; the
    cells a hash of L picks (the drawn share of them) are exactly 0 in every component, so that they are at rest.  `spec` is the grid
    the band is on; the field depends on the indices alone."""
    a = args(step)
    c = np.asarray(a["coef"], np.float64)
    _, ny, nz = band.shape
    L = band.cells.astype(np.int64)
    i, j, k = L // (ny * nz), (L // nz) % ny, L % nz
    width = 3 if a["kind"] == am.VELOCITY else 1
    f = np.stack([np.sin(c[3 * w] * i + c[3 * w + 1] * j + c[3 * w + 2] * k + c[9 + w]) for w in range(width)], 1).astype(F)
    h = (L.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(int(c[0] * 2 ** 40))) >> np.uint64(44)
    f[(h % np.uint64(1024)).astype(np.int64) < a["still"] * 1024] = 0
    return f if width == 3 else f.reshape(-1)


def dt_of(step, spec):
    """advect: the time step, the drawn CFL fraction of the smallest cell side, in binary32.  The entries of `field_of` reach 1 per
    component, so max_cfl goes up to that fraction times (1/h_i + 1/h_j + 1/h_k) min(h): past 1 on the cubic grids, which the call
    reports and does not forbid."""
    return F(args(step)["cfl"] * min(spec.cell))


# ---- the model chain -----------------------------------------------------------------------------------------------------------------------
class Result(NamedTuple):
    """One step of a model chain: the band and grid (0 or 1 of the pair) it ran on, its result and the grid that is on, the model's
    info, and for select the model's Components and the keep mask."""
    step: tuple
    source: cm.Band
    source_grid: int
    band: cm.Band
    grid: int
    info: tuple
    components: object
    keep: object


def model_step(pair, step, band, at):
    """One step through its model -> Result."""
    a = args(step)
    spec = PAIRS[pair][at]
    op = step[0]
    comps = keep = info = None
    to = at
    if op == "csg":
        partner = pool(pair, at)[a["partner"]]
        x, y = (partner, band) if a["swap"] else (band, partner)
        out = cm.csg(x, y, a["kind"])
    elif op == "filter":
        where = None if a["where"] is None else pool(pair, at)[a["where"]]
        out, info = fm.band_filter(band, spec.cell, a["kind"], a["iterations"], where=where, background=a["background"])
    elif op == "redistance":
        out, info = rm.redistance(band, spec.cell, *widths(step, spec))
    elif op == "resample":
        to = a["target"]
        to_source, scale = rsm.similarity(forward_of(step, spec, PAIRS[pair][to]))
        out, info = rsm.resample(band, spec, PAIRS[pair][to], to_source, scale, a["mode"])
    elif op == "select":
        comps = ccm.components(band, a["connectivity"])
        keep = keep_of(step, comps.n_cells)
        out, info = ccm.select(band, comps.labels, keep)
    elif op == "advect":
        out, info = am.band_advect(band, spec.cell, a["kind"], field_of(step, band, spec), dt_of(step, spec), a["steps"], a["background"])
    else:
        raise ValueError(op)
    return Result(step, band, at, out, to, info, comps, keep)


def run_model(pair, steps, band, at):
    """The chain `steps` from `band` on grid `at` of PAIRS[pair] through the models -> [Result], one per step."""
    out = []
    for step in steps:
        r = model_step(pair, step, band, at)
        out.append(r)
        band, at = r.band, r.grid
    return out


@functools.lru_cache(maxsize=None)
def chain(seed, pair):
    """The model's side of chain `seed` on PAIRS[pair], once: -> (start grid, start pool band, [Result])."""
    g, p = start_of(seed, pair)
    return g, p, run_model(pair, plan(seed, pair), pool(pair, g)[p], g)


@functools.lru_cache(maxsize=None)
def chain_b(seed, pair):
    """The second family's `chain`."""
    g, p = start_of_b(seed, pair)
    return g, p, run_model(pair, plan_b(seed, pair), pool(pair, g)[p], g)
