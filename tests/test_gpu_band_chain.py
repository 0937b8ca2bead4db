"""Random chains of band calls on the GPU, bit for bit against the chained numpy models (tests/band_chain_cases.py).

The per-call band tests hand each call a handle made by m2s_band_create.  Here every call but the first of a chain is handed what
another call left behind: the words past `total`, the offsets of empty words, the values at the list's end, the second allocation of
a resample result, an empty result's one-float list.  None of that shows in m2s_band_export; it shows in what the next call computes.
So after every step the result is compared with the model's step (cells, distance bits, sign mask, backgrounds, count, every info
field, device_bytes), the input handle having been closed before anything is read from the result; at the end of a chain the last
handle is measured, labelled, sampled and meshed.  There are two families of chains: the first of csg, filter, redistance, resample and
select, the second with advect as a sixth op, whose result's mask and offsets are copies of its input's and whose neighbour table is
built from whatever handle it is given.  On a mismatch the same op is run once more on a handle created afresh from the model's
previous band: if that agrees, the op misread the handle it was given; if not, the op itself is wrong on that band."""
import functools

import numpy as np
import pytest
import torch

import band_advect_model as am
import band_chain_cases as cc
import band_components_model as ccm
import band_csg_model as cm
import band_filter_model as fm
import band_isosurface_model as bim
import band_measure_model as mm
import grid_query_model as gqm
import isosurface_model as im
from mesh_to_sdf_amd import BandField, CsgOp, FilterKind, Grid, Mesh, SampleMode, Topology, band_isosurface, sample_grid
from mesh_to_sdf_amd import meshes
from test_gpu_band_isosurface import _same_mesh

F = np.float32
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = [SampleMode.Snap, SampleMode.Trilinear, SampleMode.Tetrahedral]
KINDS = {fm.MEAN: FilterKind.Mean, fm.LAPLACIAN: FilterKind.Laplacian, fm.MEAN_CURVATURE: FilterKind.MeanCurvature}
CSG = {cm.UNION: CsgOp.Union, cm.INTERSECTION: CsgOp.Intersection, cm.DIFFERENCE: CsgOp.Difference}


def _np(x):
    if hasattr(x, "cpu"):
        if x.dtype == getattr(torch, "uint32", None):
            x = x.view(torch.int32)
        x = x.cpu().numpy()
    return np.asarray(x)


@functools.lru_cache(maxsize=None)
def _grid(pair, g):
    spec = cc.PAIRS[pair][g]
    return Grid(list(spec.first), list(spec.cell), list(spec.shape))


def _field(grid, band, device):
    """The BandField of a model Band, from device tensors or host arrays."""
    bg = (float(band.bg_in), float(band.bg_out))
    if device:
        bits = None if band.bits is None else torch.as_tensor(np.ascontiguousarray(band.bits).view(np.int32), device=DEV)
        return BandField(grid, torch.as_tensor(band.cells, device=DEV), torch.as_tensor(band.distances, device=DEV), background=bg, inside=bits)
    return BandField(grid, band.cells.astype(np.uint64), band.distances, background=bg, inside=band.bits)


def _band(field):
    """A handle's lists as a model Band."""
    nb = field.to_band()
    return cm.Band(tuple(int(v) for v in field.grid.get_cell_count()), _np(nb.cells).astype(np.int64), _np(nb.distances),
                   _np(nb.bits).view(np.uint32), field.background[1], field.background[0])


class Pool:
    """The pool bands of both grids of a pair as resident fields, all on one side."""

    def __init__(self, pair, device):
        self.pair, self.device = pair, device
        self.fields = [[_field(_grid(pair, g), b, device) for b in cc.pool(pair, g)] for g in range(2)]

    def close(self):
        for fs in self.fields:
            for f in fs:
                f.close()


# ---- one step through the library ------------------------------------------------------------------------------------------------------------
def _components_differences(got, want):
    out = []
    if got.count != want.count:
        return [f"{got.count} components, the model has {want.count}"]
    labels = _np(got.labels).view(np.uint32)
    differ = labels != want.labels
    if differ.any():
        out.append(f"{int(differ.sum())} labels differ, first at list place {np.flatnonzero(differ)[0]}")
    for name, g, w in (("first_cell", got.first_cell, want.first_cell), ("n_cells", got.n_cells, want.n_cells),
                       ("n_negative", got.n_negative, want.n_negative), ("box_lo", got.box_lo, want.lo), ("box_hi", got.box_hi, want.hi)):
        if g.shape != w.shape or not np.array_equal(g, w):
            out.append(f"components' {name} differs")
    return out


def _apply(pool, step, field, at, want):
    """`step` on `field`, which is on grid `at` of the pool's pair -> (the result, what already differs from the model's step `want`).
    `field` is closed as soon as the result exists."""
    a = cc.args(step)
    op = step[0]
    spec = cc.PAIRS[pool.pair][at]
    early = []
    try:
        if op == "csg":
            partner = pool.fields[at][a["partner"]]
            out = partner.csg(field, CSG[a["kind"]]) if a["swap"] else field.csg(partner, CSG[a["kind"]])
        elif op == "filter":
            bg = a["background"]
            out = field.filter(KINDS[a["kind"]], a["iterations"], where=None if a["where"] is None else pool.fields[at][a["where"]],
                               background=None if bg is None else (bg[1], bg[0]))
        elif op == "redistance":
            exterior, interior = cc.widths(step, spec)
            out = field.redistance((interior, exterior))
        elif op == "resample":
            out = field.resample(_grid(pool.pair, a["target"]), cc.forward_of(step, spec, cc.PAIRS[pool.pair][a["target"]]), mode=MODES[a["mode"]])
        elif op == "select":
            comps = field.components(a["connectivity"])
            early = _components_differences(comps, want.components)
            out = field.select(comps, cc.keep_of(step, comps.n_cells))
        elif op == "advect":
            given = cc.field_of(step, want.source, spec)                     # on the model's cells: the handle's, or an earlier step has failed
            if pool.device:
                given = torch.as_tensor(given, device=DEV)
            bg = a["background"]
            out = field.advect(float(cc.dt_of(step, spec)), a["steps"], background=None if bg is None else (bg[1], bg[0]),
                               **{"velocity" if a["kind"] == am.VELOCITY else "speed": given})
        else:
            raise ValueError(op)
    finally:
        field.close()
    return out, early


def _differences(field, want):
    """A result handle against the model's Result -> what differs, as a list of sentences (empty: nothing)."""
    out = []
    b, info, op = want.band, want.info, want.step[0]
    got = _band(field)
    if got.shape != b.shape:
        return [f"the result is on a grid of {got.shape}, the model's on {b.shape}"]
    if not got.cells.size == b.cells.size == field.count:
        out.append(f"{got.cells.size} cells exported, count {field.count}, the model has {b.cells.size}")
    if not np.array_equal(got.cells, b.cells):
        out.append("cells differ")
    else:
        differ = got.distances.view(np.uint32) != b.distances.view(np.uint32)
        if differ.any():
            out.append(f"{int(differ.sum())} distances differ, first at cell {b.cells[np.flatnonzero(differ)[0]]}")
    if not np.array_equal(got.bits, b.bits):
        wrong = cm.unpack_bits(b.shape, got.bits) != cm.unpack_bits(b.shape, b.bits)
        out.append(f"the sign mask differs on {int(wrong.sum())} grid points (first at {np.argwhere(wrong)[:1].tolist()}) and in "
                   f"{int((got.bits != b.bits).sum())} words")
    if got.bg_out.view(np.uint32) != b.bg_out.view(np.uint32) or got.bg_in.view(np.uint32) != b.bg_in.view(np.uint32):
        out.append(f"backgrounds (outside, inside) {got.bg_out, got.bg_in}, the model has {b.bg_out, b.bg_in}")
    if field.device_bytes != 24 * ((b.total + 63) // 64) + 4 * b.cells.size:
        out.append(f"device_bytes {field.device_bytes}, not 24 * {(b.total + 63) // 64} + 4 * {b.cells.size}")
    if op == "filter":
        fi = field.filter_info
        if (fi.passes, fi.n_changed, fi.n_sign_flips, fi.n_nonfinite) != (info.passes, info.n_changed, info.n_sign_flips, info.n_nonfinite) \
                or F(fi.max_change).view(np.uint32) != F(info.max_change).view(np.uint32):
            out.append(f"info {fi}, the model has {info}")
    elif op == "redistance":
        if tuple(int(v) for v in field.redistance_info) != tuple(int(v) for v in info):
            out.append(f"info {field.redistance_info}, the model has {info}")
    elif op == "resample":
        if tuple(field.resample_info) != tuple(info):
            out.append(f"info {field.resample_info}, the model has {info}")
    elif op == "select":
        if tuple(field.select_info) != tuple(info):
            out.append(f"info {field.select_info}, the model has {info}")
    elif op == "advect":
        ai = field.advect_info
        if (ai.steps, ai.n_moving, ai.n_changed, ai.n_sign_flips, ai.n_nonfinite) != (info.steps, info.n_moving, info.n_changed, info.n_sign_flips, info.n_nonfinite) \
                or F(ai.max_change).view(np.uint32) != F(info.max_change).view(np.uint32) or F(ai.max_cfl).view(np.uint32) != F(info.max_cfl).view(np.uint32):
            out.append(f"info {ai}, the model has {info}")
    return out


def _replay(pool, field, at, results, what):
    """The chain of the model's `results` from `field` (on grid `at`), every step compared -> the last handle, open."""
    for index, want in enumerate(results):
        assert at == want.source_grid
        field, wrong = _apply(pool, want.step, field, at, want)
        wrong = wrong + _differences(field, want)
        if wrong:
            field.close()
            fresh, again = _apply(pool, want.step, _field(_grid(pool.pair, at), want.source, pool.device), at, want)
            again = again + _differences(fresh, want)
            fresh.close()
            verdict = ("the same call on a handle created afresh from the model's previous band agrees with the model: the call misread the handle it was given"
                       if not again else "the same call on a handle created afresh from the model's previous band differs too: " + "; ".join(again))
            pytest.fail(f"{what}, step {index}, {cc.describe(want.step)} on grid {at} ({want.source.cells.size} cells in): " + "; ".join(wrong) + ".  " + verdict)
        at = want.grid
    return field


def _observe(pool, field, at, band, what, seed):
    """The last handle of a chain, read four ways: measure, components(26), sample in the three modes with normals, band_isosurface."""
    spec = cc.PAIRS[pool.pair][at]
    grid = _grid(pool.pair, at)
    want = mm.measure(spec.shape, spec.cell, band.cells, band.distances)
    m = field.measure()
    for f in mm.INT_FIELDS:
        w = getattr(want, f)[0]
        w = tuple(int(v) for v in w) if f == "moment_q" else int(w)
        assert getattr(m, f) == w, f"{what}, the last handle: measure's {f} = {getattr(m, f)}, the model has {w}"
    assert m.closed == mm.closed(want) and m.euler == mm.euler(want), f"{what}, the last handle: measure"
    wrong = _components_differences(field.components(26), ccm.components(band, 26))
    assert not wrong, f"{what}, the last handle: components(26): " + "; ".join(wrong)
    q = gqm.GridQ.of(grid)
    lo, hi = q.start - q.cs, q.end + q.cs
    pts = (lo + np.random.default_rng(seed).random((500, 3)) * (hi - lo)).astype(F)
    dense = cm.dense(band)[1].reshape(-1)
    if pool.device:
        pts, dense = torch.as_tensor(pts, device=DEV), torch.as_tensor(dense, device=DEV)
    for mode in MODES:
        gv, gn = field.sample(pts, mode=mode, normals=True)
        wv, wn = sample_grid(grid, dense, pts, mode=mode, normals=True)
        assert gqm.same_bits(_np(gv), _np(wv)), f"{what}, the last handle: {mode.name} samples differ from sample_grid on the model's dense grid"
        assert gqm.same_bits(_np(gn), _np(wn)), f"{what}, the last handle: {mode.name} normals differ from sample_grid on the model's dense grid"
    nb = field.to_band()
    _same_mesh(band_isosurface(grid, nb.cells, nb.distances), bim.extract(im.GridI.of(grid), band.cells.astype(np.uint64), band.distances, 0.0),
               f"{what}, the last handle: band_isosurface")


# ---- (a) random chains from the pool bands ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("pair", range(len(cc.PAIRS)), ids=cc.PAIR_IDS)
def test_random_chains(pair, device):
    pool = Pool(pair, device)
    try:
        for seed in cc.SEEDS:
            g, p, results = cc.chain(seed, pair)
            what = f"pair {cc.PAIR_IDS[pair]}, seed {seed}, {'device' if device else 'host'}, from pool band {p} ({cc.POOL_NAMES[p]}) on grid {g}"
            last = _replay(pool, _field(_grid(pair, g), cc.pool(pair, g)[p], device), g, results, what)
            with last:
                _observe(pool, last, results[-1].grid, results[-1].band, what, seed)
    finally:
        pool.close()


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("pair", range(len(cc.PAIRS)), ids=cc.PAIR_IDS)
def test_random_chains_with_advect(pair, device):
    """The second family: advect among the six ops, on what csg, resample and select left behind, and its results consumed."""
    pool = Pool(pair, device)
    try:
        for seed in cc.SEEDS_B:
            g, p, results = cc.chain_b(seed, pair)
            what = f"with advect, pair {cc.PAIR_IDS[pair]}, seed {seed}, {'device' if device else 'host'}, from pool band {p} ({cc.POOL_NAMES[p]}) on grid {g}"
            last = _replay(pool, _field(_grid(pair, g), cc.pool(pair, g)[p], device), g, results, what)
            with last:
                _observe(pool, last, results[-1].grid, results[-1].band, what, seed)
    finally:
        pool.close()


# ---- (b) chains from handles the library made ------------------------------------------------------------------------------------------------
# Whatever a producer left in the words past what export shows, every later call must behave as on the handle re-created from the
# export: the model chain starts from to_band().  All on the 13 x 11 x 37 grid, the solids filling about half of it.
B_PAIR, B_GRID = 1, 1
B_SEEDS = (0, 1, 2, 3)


def _box(spec):
    lo = np.asarray(spec.first, np.float64) - 0.5 * np.asarray(spec.cell)
    return lo, lo + np.asarray(spec.shape) * np.asarray(spec.cell)


def _mesh_source(inside):
    def make(grid, spec, rng):
        v, idx = meshes.blob(16, 17)
        lo, hi = _box(spec)
        v = (v.astype(np.float64) * (0.37 * (hi - lo)) + (lo + hi) / 2).astype(F)          # radii of 0.7 to 1.3: most of the box's half-widths
        with Mesh(torch.as_tensor(v, device=DEV), Topology.TriangleList(torch.as_tensor(idx.astype(np.int32), device=DEV))) as mesh:
            return mesh.narrow_band_field(grid, 2.0 * max(spec.cell), inside=inside)
    return make


def _capsule_source(grid, spec, rng):
    lo, hi = _box(spec)
    a = rng.uniform(lo, hi, (40, 3))
    b = a + rng.normal(0, 0.2, (40, 3)) * (hi - lo)
    r = rng.uniform(1, 2, 40) * spec.cell[0]
    a, b, r = (torch.as_tensor(x.astype(F), device=DEV) for x in (a, b, r))
    return BandField.from_capsules(grid, a, b, r, 2.0 * max(spec.cell))


def _sphere_source(grid, spec, rng):
    lo, hi = _box(spec)
    c = torch.as_tensor(rng.uniform(lo, hi, (200, 3)).astype(F), device=DEV)
    r = torch.as_tensor((rng.uniform(1, 2, 200) * spec.cell[0]).astype(F), device=DEV)
    return BandField.from_spheres(grid, c, r, 2.0 * max(spec.cell))


SOURCES = {"mesh, inside=True": _mesh_source(True), "mesh, inside=None": _mesh_source(None), "capsules": _capsule_source, "spheres": _sphere_source}


def _from_source(source, plan, family):
    spec, grid = cc.PAIRS[B_PAIR][B_GRID], _grid(B_PAIR, B_GRID)
    total = spec.shape[0] * spec.shape[1] * spec.shape[2]
    pool = Pool(B_PAIR, True)
    try:
        for seed in B_SEEDS:
            start = SOURCES[source](grid, spec, np.random.default_rng(100 + seed))
            band = _band(start)
            inside = int(cm.dense(band)[2].sum())
            assert total // 20 < band.cells.size and total // 20 < inside < total, f"{source}: {band.cells.size} cells, {inside} points inside, of {total}"
            results = cc.run_model(B_PAIR, plan(seed, B_PAIR), band, B_GRID)
            what = f"{family}pair {cc.PAIR_IDS[B_PAIR]}, seed {seed}, from {source} on grid {B_GRID}"
            last = _replay(pool, start, B_GRID, results, what)
            with last:
                _observe(pool, last, results[-1].grid, results[-1].band, what, seed)
    finally:
        pool.close()


@pytest.mark.parametrize("source", list(SOURCES), ids=[s.replace(", ", "-").replace("=", "-") for s in SOURCES])
def test_chains_from_library_made_sources(source):
    _from_source(source, cc.plan, "")


@pytest.mark.parametrize("source", list(SOURCES), ids=[s.replace(", ", "-").replace("=", "-") for s in SOURCES])
def test_chains_with_advect_from_library_made_sources(source):
    _from_source(source, cc.plan_b, "with advect, ")


# ---- (c) empty and full fields through every op ----------------------------------------------------------------------------------------------
C_PAIR, C_GRID = 1, 0                                                               # 9 x 7 x 70
C_STEPS = (("csg", ("partner", 3), ("swap", False), ("kind", cm.UNION)),
           ("csg", ("partner", 0), ("swap", True), ("kind", cm.DIFFERENCE)),
           ("filter", ("kind", fm.MEAN_CURVATURE), ("iterations", 2), ("where", 0), ("background", (1.5, 0.25))),
           ("redistance", ("exterior", 2.0), ("interior", 1.5)),
           ("resample", ("target", 1), ("scale", 1.05), ("axis", (1.0, 2.0, 3.0)), ("angle", 0.2), ("jitter", (0.3, -0.2, 0.1)), ("mode", 1)),
           ("resample", ("target", 0), ("scale", 1.0), ("axis", (0.0, 0.0, 1.0)), ("angle", 0.0), ("jitter", (0.0, 0.0, 0.0)), ("mode", 0)),
           ("select", ("connectivity", 6), ("keep_u", (0.9, 0.1))),
           ("advect", ("kind", am.VELOCITY), ("steps", 2), ("cfl", 0.6), ("coef", (0.3, 0.5, 0.7, 0.4, 0.6, 0.8, 0.25, 0.45, 0.65, 1.0, 2.0, 3.0)),
            ("still", 0.25), ("background", None)),
           ("advect", ("kind", am.NORMAL), ("steps", 3), ("cfl", 0.4), ("coef", (0.8, 0.6, 0.4, 0.7, 0.5, 0.3, 0.65, 0.45, 0.25, 4.0, 5.0, 0.5)),
            ("still", 0.4), ("background", (1.25, 0.375))))


def _extremes():
    """-> [(name, how to make the field on a side, its model Band)]: empty by create, empty by an op, full."""
    shape = cc.PAIRS[C_PAIR][C_GRID].shape
    total = shape[0] * shape[1] * shape[2]
    rng = np.random.default_rng(5)
    grid = _grid(C_PAIR, C_GRID)
    empty = cm.Band(shape, np.zeros(0, np.int64), np.zeros(0, F), None, 0.75, 0.5)
    # two bands on disjoint halves, each inside its own cells and outside the other's: the intersection has no cell; both masks are
    # set on the layer between them, so the empty result has a sign mask that is not
    i = np.arange(total) // (shape[1] * shape[2])
    between = np.zeros(shape, bool)
    between[4] = True
    halves = []
    for cells in (np.flatnonzero(i < 4), np.flatnonzero(i > 4)):
        halves.append(cm.Band(shape, cells, rng.uniform(-0.4, -0.1, cells.size).astype(F), cm.pack_bits(shape, between), 0.75, 0.5))
    disjoint = cm.csg(halves[0], halves[1], cm.INTERSECTION)
    assert disjoint.cells.size == 0 and int(cm.unpack_bits(shape, disjoint.bits).sum()) == shape[1] * shape[2]
    full = cm.Band(shape, np.arange(total), rng.uniform(-1, 1, total).astype(F), rng.integers(0, 2 ** 32, (shape[0], shape[1], (shape[2] + 31) // 32),
                                                                                              dtype=np.uint64).astype(np.uint32), 0.75, 0.5)

    def by_op(device):
        with _field(grid, halves[0], device) as fa, _field(grid, halves[1], device) as fb:
            return fa & fb
    return [("empty by create", lambda device: _field(grid, empty, device), empty), ("empty by an intersection", by_op, disjoint),
            ("full", lambda device: _field(grid, full, device), full)]


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_empty_and_full_through_every_op(device):
    spec, grid = cc.PAIRS[C_PAIR][C_GRID], _grid(C_PAIR, C_GRID)
    pool = Pool(C_PAIR, device)
    try:
        for name, make, band in _extremes():
            what = f"{name}, {'device' if device else 'host'}"
            if name == "empty by an intersection":
                with make(device) as f:
                    assert cm.same(_band(f), band) and f.count == 0, what
            for step in C_STEPS:
                want = cc.model_step(C_PAIR, step, band, C_GRID)
                last = _replay(pool, make(device), C_GRID, [want], what)
                last.close()
            # as the region of a filter: the pool's noise band smoothed where this field is inside
            target = cc.pool(C_PAIR, C_GRID)[3]
            for kind in fm.KINDS:
                w, info = fm.band_filter(target, spec.cell, kind, 2, where=band)
                want = cc.Result(("filter", ("kind", kind)), target, C_GRID, w, C_GRID, info, None, None)
                with make(device) as region, pool.fields[C_GRID][3].filter(KINDS[kind], 2, where=region) as r:
                    wrong = _differences(r, want)
                    assert not wrong, f"{what} as the region of filter kind {kind}: " + "; ".join(wrong)
    finally:
        pool.close()
