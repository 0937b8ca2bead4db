"""The random cases of m2s_band_advect that tests/test_band_advect_cpu.py (the model against itself, coverage of the generator) and
tests/test_gpu_band_advect.py (the library against the model) share: bands on the smallest grids where the kernels can go wrong, and per
band a velocity field and a speed field.

Shapes, as in tests/test_gpu_band_filter.py and for its reasons.  1x1x1, 2x2x2: every read clamped.  5x3x70: rows longer than a word,
words that straddle rows.  3x65x1: nz = 1.  7x9x11: rows shorter than a word, a total that is no multiple of 64.  24x20x28: several
units' worth of rows.  70x64x64: 4480 mask words, 18 units, more than one group of 16."""
from typing import NamedTuple

import numpy as np

import band_advect_model as am
import band_csg_model as cm

F = np.float32
FMAX = np.finfo(F).max
CELL = (0.125, 0.25, 0.1875)
FIRST = (-0.5, 0.25, 0.0)
SPECIAL = np.array([0.0, -0.0, 0.5, -0.5, 0.75, -0.75, 2.0, -2.0, FMAX, -FMAX], F)   # zeros of both signs, values beyond the backgrounds, +-f32::MAX
SHAPES = [(1, 1, 1), (2, 2, 2), (5, 3, 70), (3, 65, 1), (7, 9, 11), (24, 20, 28), (70, 64, 64)]
STEPS = (1, 2, 3, 5)                                                             # both parities of the two value buffers
RATE = sum(1.0 / h for h in CELL)                                                 # r_i + r_j + r_k


class Case(NamedTuple):
    name: str
    band: cm.Band
    kind: int
    field: np.ndarray          # float32[n, 3] or float32[n]
    dt: float
    steps: int
    background: tuple          # (outside, inside) of the result, or None


def seed_of(shape):
    return 7000 + sum(shape)


def random_band(rng, shape, density=0.5, bits=True, bg=(0.75, 0.5), special=0.3):
    total = shape[0] * shape[1] * shape[2]
    cells = np.flatnonzero(rng.random(total) < density)
    d = rng.uniform(-1, 1, cells.size).astype(F)
    pick = rng.random(cells.size) < special
    d[pick] = rng.choice(SPECIAL, int(pick.sum()))
    mask = rng.integers(0, 2 ** 32, (shape[0], shape[1], (shape[2] + 31) // 32), dtype=np.uint64).astype(np.uint32) if bits else None
    return cm.Band(shape, cells, d, mask, *bg)


def smooth_band(rng, shape, bits=True):
    """A random low-order trigonometric field's band: neighbouring values that belong together, so that many steps stay finite."""
    i, j, k = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    a = rng.uniform(0.2, 0.9, 3)
    d = (np.sin(a[0] * i + rng.uniform(0, 6)) + np.sin(a[1] * j + rng.uniform(0, 6)) + np.sin(a[2] * k + rng.uniform(0, 6))).astype(F) * F(0.2)
    d = d.reshape(-1)
    cells = np.flatnonzero((np.abs(d) <= 0.3) & (rng.random(d.size) < 0.9))
    mask = cm.pack_bits(shape, (d < 0).reshape(shape)) if bits else None
    return cm.Band(shape, cells, d[cells], mask, 0.75, 0.5)


def random_field(rng, n, kind, rest=0.25, zeros=0.15, nonfinite=False):
    """Entries of both signs in [-1, 1]; a share `zeros` of the components exactly 0 or -0.0; a share `rest` of the cells wholly at
    rest; with `nonfinite`, a few inf, -inf and NaN entries."""
    f = rng.uniform(-1, 1, (n, 3) if kind == am.VELOCITY else n).astype(F)
    z = rng.random(f.shape) < zeros
    f[z] = rng.choice(np.array([0.0, -0.0], F), int(z.sum()))
    f[rng.random(n) < rest] = 0
    if nonfinite and n:
        at = rng.random(f.shape) < max(0.02, 1.5 / f.size)
        f[at] = rng.choice(np.array([np.inf, -np.inf, np.nan], F), int(at.sum()))
    return f


def dt_for(field, kind, cfl):
    """The dt at which the fastest cell with a finite entry gives about `cfl` (a field with no such cell counts as slow)."""
    a = np.abs(field.astype(np.float64))
    rate = a @ (1.0 / np.asarray(CELL)) if kind == am.VELOCITY else a * RATE
    rate = rate[np.isfinite(rate)]
    top = rate.max() if rate.size else 0.0
    return float(F(cfl / max(top, 0.25 * RATE)))


def cases(shape):
    """The cases of one shape, the same list on every call."""
    rng = np.random.default_rng(seed_of(shape))
    big = shape[0] * shape[1] * shape[2] > 100000
    bands = [("random", random_band(rng, shape)), ("smooth", smooth_band(rng, shape)), ("smooth, no mask", smooth_band(rng, shape, bits=False))]
    if not big:
        bands += [("sparse", random_band(rng, shape, 0.05, special=1.0)), ("dense, no mask", random_band(rng, shape, 0.95, bits=False)),
                  ("full", random_band(rng, shape, 1.1, special=0.1)), ("empty", random_band(rng, shape, 0.0)),
                  ("empty, no mask", random_band(rng, shape, 0.0, bits=False))]
    out = []
    for at, (name, band) in enumerate(bands):
        n = band.cells.size
        for kind in am.KINDS:
            every = name in ("random", "smooth") or not big and name == "full"
            for steps in STEPS if every else (STEPS[(at + kind) % 4],):
                nonfinite = name == "random" and steps == 2                      # one case per shape and kind with inf / NaN entries
                fast = name == ("smooth" if big else "full") and steps == 3      # one case per shape and kind with max_cfl > 1
                field = random_field(rng, n, kind, nonfinite=nonfinite)
                dt = dt_for(field, kind, 1.6 if fast else 0.5)
                bg = (2.0, 0.125) if (at + steps + kind) % 2 else None
                out.append(Case(f"{name}, kind {kind}, {steps} steps" + (", inf / NaN" if nonfinite else "") + (", cfl > 1" if fast else ""),
                                band, kind, field, dt, steps, bg))
    return out
