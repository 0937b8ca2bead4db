"""m2s_band_measure on the GPU against tests/band_measure_model.py (the definition in numpy): every integer field of every record is
compared for equality, the derived doubles to 1e-13.  A sphere on a grid with unequal cells at two isos and two positions; random values on
random masks where rows straddle mask words, with and without labels, from device tensors and host arrays; two spheres and a speck labelled
by m2s_band_components (more than one wave's unit, so sums are flushed where the label changes); the chains that motivate the call; empty
and degenerate bands; a grid past 2^32 points with its band at the far corner; what the call rejects of a real handle; the C and C++
consumers."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest
import torch

import band_components_model as ccm
import band_csg_model as cm
import band_measure_model as mm
import band_redistance_model as rm
import band_window as bw
from mesh_to_sdf_amd import BandField, Grid, M2SError, Measure, _lib
from test_band_measure_cpu import CONSUMERS, build_consumer

F = np.float32
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIRST = (-0.5, 0.25, 3.0)
CELL = (0.125, 0.25, 0.1875)


def _np(x):
    if hasattr(x, "cpu"):
        if x.dtype == getattr(torch, "uint32", None):
            x = x.view(torch.int32)
        x = x.cpu().numpy()
    return np.asarray(x)


def _field(grid, cells, values, device, background=1.0):
    if device:
        return BandField(grid, torch.as_tensor(np.asarray(cells).astype(np.int64), device=DEV), torch.as_tensor(np.asarray(values, F), device=DEV), background=background)
    return BandField(grid, np.asarray(cells).astype(np.uint64), np.asarray(values, F), background=background)


def _check(got, want, first, cell, what):
    """A Measure or a list of them against the model's Raw, group by group."""
    got = [got] if isinstance(got, Measure) else got
    assert len(got) == want.n_triangles.size, what
    for g, m in enumerate(got):
        for f in mm.INT_FIELDS:
            w = getattr(want, f)[g]
            w = tuple(int(v) for v in w) if f == "moment_q" else int(w)
            assert getattr(m, f) == w, f"{what}: group {g}: {f} = {getattr(m, f)}, the model has {w}"
        area, volume, centroid = mm.derived(want, first, cell, g)
        assert m.area == pytest.approx(area, rel=1e-13) and m.volume == pytest.approx(volume, rel=1e-13), (what, g)
        assert m.centroid == pytest.approx(centroid, rel=1e-13, nan_ok=True), (what, g)
        assert m.closed == mm.closed(want, g) and m.euler == mm.euler(want, g), (what, g)


# ---- 1. a sphere ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_a_sphere_on_unequal_cells_at_two_isos_and_two_positions(device):
    shape = (24, 24, 24)
    d = mm.sphere_distance(shape, (1.43, 2.9, 2.21), 1.1, CELL)
    cells, values = mm.band_of(d, 0.75)
    got = {}
    for first in (FIRST, (1000.0, -250.0, 0.0)):
        with _field(Grid(list(first), list(CELL), list(shape)), cells, values, device) as f:
            for iso in (0.0, 0.3):
                want = mm.measure(shape, CELL, cells, values, iso)
                assert int(want.n_triangles[0]) > 500 and mm.closed(want)
                m = f.measure(iso)
                _check(m, want, first, CELL, f"sphere at {first}, iso {iso}")
                assert f.measure_info == (want.area_exponent, 1, 0)
                got[first, iso] = m
            assert f.area() == got[first, 0.0].area and f.volume() == got[first, 0.0].volume and f.centroid() == got[first, 0.0].centroid
    for iso in (0.0, 0.3):   # the raw sums, the area and the volume know nothing of the grid's position
        assert got[FIRST, iso][:9] == got[(1000.0, -250.0, 0.0), iso][:9]
    m = got[FIRST, 0.0]
    assert m.volume == pytest.approx(4 / 3 * np.pi * 1.1 ** 3, rel=0.06) and m.area == pytest.approx(4 * np.pi * 1.1 ** 2, rel=0.04)   # a radius of 4.4 to 8.8 cells
    assert np.asarray(m.centroid) == pytest.approx(np.asarray(FIRST) + (1.43, 2.9, 2.21), abs=2e-3)


# ---- 2. random values on random masks --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_band():
    shape = (9, 7, 70)       # rows of 70 points straddle the mask words
    rng = np.random.default_rng(20)
    active = rng.random(shape) < 0.9
    active[2:5, 1:5, 10:60] = True                                   # a block of complete cells among the incomplete ones
    cells = np.flatnonzero(active.reshape(-1))
    values = rng.uniform(-1, 1, cells.size).astype(F)
    values[rng.random(cells.size) < 0.05] = 0.0                      # a value equal to iso is outside
    labels = rng.integers(0, 5, cells.size).astype(np.uint32)
    labels[rng.random(cells.size) < 0.1] = mm.LABEL_NONE
    labels[rng.random(cells.size) < 0.05] = 7
    return shape, cells, values, labels


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_random_values_on_random_masks(device):
    shape, cells, values, labels = _random_band()
    for iso in (0.0, -0.25):
        want = mm.measure(shape, CELL, cells, values, iso)
        cases = np.unique(_cases_of(shape, cells, values, iso))
        assert cases.size > 230 and int(want.n_open[0]) > 100 and int(want.n_border[0]) > 100, (cases.size, want)
        with _field(Grid(list(FIRST), list(CELL), list(shape)), cells, values, device) as f:
            _check(f.measure(iso), want, FIRST, CELL, f"random, iso {iso}")
            grouped = mm.measure(shape, CELL, cells, values, iso, labels=labels, n_groups=5)
            assert grouped.n_skipped == int((labels >= 5).sum()) > 50
            lab = torch.as_tensor(labels.view(np.int32), device=DEV) if device else labels
            _check(f.measure(iso, lab, n_groups=5), grouped, FIRST, CELL, f"random with labels, iso {iso}")
            assert f.measure_info == (grouped.area_exponent, 5, grouped.n_skipped)


def _cases_of(shape, cells, values, iso):
    act = np.zeros(shape, bool).reshape(-1)
    d = np.zeros(shape, F).reshape(-1)
    act[cells], d[cells] = True, values
    act, inside = act.reshape(shape), (d < F(iso)).reshape(shape)
    sub = lambda x, c: x[(c >> 2) & 1:shape[0] - 1 + ((c >> 2) & 1), (c >> 1) & 1:shape[1] - 1 + ((c >> 1) & 1), (c & 1):shape[2] - 1 + (c & 1)]   # noqa: E731
    complete = functools.reduce(np.logical_and, [sub(act, c) for c in range(8)])
    case = sum(sub(inside, c).astype(np.int64) << c for c in range(8))
    return case[complete]


# ---- 3. components -------------------------------------------------------------------------------------------------------------------------
def test_two_spheres_and_a_speck_by_component():
    shape = (48, 40, 44)     # 1320 mask words: six units of 256 words, two workgroups
    radii = (10.2, 9.1, 2.3)
    d = np.minimum(np.minimum(mm.sphere_distance(shape, (13.3, 14.1, 14.7), radii[0]), mm.sphere_distance(shape, (34.4, 26.2, 30.9), radii[1])),
                   mm.sphere_distance(shape, (40.2, 7.4, 8.1), radii[2]))
    cells, values = mm.band_of(d, 2.5)
    assert cells.size > 10000
    with _field(Grid(list(FIRST), list(CELL), list(shape)), cells, values, True) as f:
        comps = f.components(26)
        labels = _np(comps.labels).view(np.uint32)
        assert comps.count == 3 and np.array_equal(labels, ccm.components(cm.Band(shape, cells.astype(np.int64), values, None, 1.0, 1.0), 26).labels)
        want = mm.measure(shape, CELL, cells, values, labels=labels, n_groups=3)
        parts = comps.measure(f)
        _check(parts, want, FIRST, CELL, "two spheres and a speck")
        whole = f.measure()
        _check(whole, mm.measure(shape, CELL, cells, values), FIRST, CELL, "two spheres and a speck, unlabelled")
        for field in ("n_triangles", "n_vertices", "n_open", "n_border", "area_q", "volume_q"):
            assert sum(getattr(p, field) for p in parts) == getattr(whole, field), field
        assert tuple(sum(p.moment_q[c] for p in parts) for c in range(3)) == whole.moment_q
        assert all(p.closed and p.euler == 2 for p in parts) and whole.euler == 6
        assert all(0.85 < p.volume / (4 / 3 * np.pi * r ** 3 * np.prod(CELL)) < 1.0 for p, r in zip(parts, radii))   # marching cubes is low, the speck most
        # labels that change inside a wave's unit and inside a word: alternate the list places between two groups
        alt = (np.arange(cells.size) // 3 % 2).astype(np.uint32)
        _check(f.measure(0.0, alt, n_groups=2), mm.measure(shape, CELL, cells, values, labels=alt, n_groups=2), FIRST, CELL, "alternating labels")


# ---- 4. the chains ---------------------------------------------------------------------------------------------------------------------------
def _export(field):
    nb = field.to_band()
    return _np(nb.cells).astype(np.int64), _np(nb.distances)


def test_the_interference_volume_of_two_overlapping_spheres():
    grid = Grid(list(rm.FIRST), list(rm.CELLS), list(rm.SHAPE))
    half = 1.5 * 0.0625
    a, b, d = (rm.band_of(rm.sphere(c, r), half) for c, r in (((0.0, 0.0, -0.25), 0.5), ((0.1, 0.0, 0.3), 0.45), ((0.7, 0.45, -1.0), 0.15)))
    mk = lambda x: BandField(grid, torch.as_tensor(x.cells, device=DEV), torch.as_tensor(x.distances, device=DEV), background=(half, half),   # noqa: E731
                             inside=torch.as_tensor(np.ascontiguousarray(x.bits).view(np.int32), device=DEV))
    with mk(a) as fa, mk(b) as fb, mk(d) as fd, (fa & fb) as lens, (fa | fb) as fab, (fab | fd) as fall:
        m = lens.measure()
        cells, values = _export(lens)
        _check(m, mm.measure(rm.SHAPE, rm.CELLS, cells, values), rm.FIRST, rm.CELLS, "A & B")
        assert m.closed and m.euler == 2 and 0 < m.volume < min(fa.volume(), fb.volume())
        # inclusion and exclusion, to the accuracy of the creases: |A| + |B| = |A or B| + |A and B|
        assert fa.volume() + fb.volume() == pytest.approx(fab.volume() + m.volume, rel=1e-2)
        # two overlapping spheres are ONE component, so the speck goes with keep_largest(1)
        total = fall.measure()
        speck = fd.measure()
        with fall.keep_largest(1) as kept:
            after = kept.measure()
            _check(after, mm.measure(rm.SHAPE, rm.CELLS, *_export(kept)), rm.FIRST, rm.CELLS, "(A | B | D).keep_largest(1)")
            assert after.closed and total.volume_q - after.volume_q == speck.volume_q > 0 and total.area_q - after.area_q == speck.area_q
            assert after.volume_q == fab.measure().volume_q


def test_keep_largest_takes_the_specks_volume_out_of_the_total():
    """The chain of test_gpu_band_components.py: A and B apart, D a speck.  (A | B | D).keep_largest(2) measures what A | B measures, and
    the difference to the whole is D's measure, integer for integer."""
    a, b, d, ab, abd = ccm.chain_bands()
    grid = Grid(list(rm.FIRST), list(rm.CELLS), list(rm.SHAPE))
    mk = lambda x: BandField(grid, torch.as_tensor(x.cells, device=DEV), torch.as_tensor(x.distances, device=DEV),   # noqa: E731
                             background=(float(x.bg_in), float(x.bg_out)), inside=torch.as_tensor(np.ascontiguousarray(x.bits).view(np.int32), device=DEV))
    with mk(a) as fa, mk(b) as fb, mk(d) as fd, (fa | fb) as fab, (fab | fd) as fall, fall.keep_largest(2) as kept:
        total, after, speck = fall.measure(), kept.measure(), fd.measure()
        _check(total, mm.measure(rm.SHAPE, rm.CELLS, abd.cells, abd.distances), rm.FIRST, rm.CELLS, "(A | B) | D")
        _check(after, mm.measure(rm.SHAPE, rm.CELLS, ab.cells, ab.distances), rm.FIRST, rm.CELLS, "keep_largest(2)")
        assert speck.volume_q > 0 and total.volume_q - after.volume_q == speck.volume_q and total.n_triangles - after.n_triangles == speck.n_triangles
        assert tuple(t - k for t, k in zip(total.moment_q, after.moment_q)) == speck.moment_q
        assert after.closed and after.euler == 4


# ---- 5. empty and degenerate bands -----------------------------------------------------------------------------------------------------------
def test_empty_and_degenerate_bands():
    shape = (6, 5, 70)
    grid = Grid(list(FIRST), list(CELL), list(shape))
    with _field(grid, np.zeros(0, np.uint64), np.zeros(0, F), True) as f:
        m = f.measure()
        assert m[:7] == (0, 0, 0, 0, 0, 0, (0, 0, 0)) and m.area == 0.0 and m.volume == 0.0 and all(np.isnan(m.centroid)) and m.closed and m.euler == 0
        three = f.measure(0.0, np.zeros(0, np.uint32), n_groups=3)
        assert [x[:6] for x in three] == [m[:6]] * 3 and all(np.isnan(x.centroid).all() for x in three) and f.measure_info[1:] == (3, 0)
    # one layer of points: edges and vertices, but no cell has its 8 corners
    i, j, k = np.meshgrid([3], np.arange(5), np.arange(70), indexing="ij")
    cells = np.sort((k + 70 * j + 350 * i).reshape(-1))
    values = np.where((cells % 7) < 3, F(-0.5), F(0.5)).astype(F)
    with _field(grid, cells, values, True) as f:
        want = mm.measure(shape, CELL, cells, values)
        assert int(want.n_triangles[0]) == 0 and int(want.n_vertices[0]) > 50 and int(want.n_open[0]) > 50 and int(want.n_border[0]) > 0
        _check(f.measure(), want, FIRST, CELL, "one layer")
        # more groups than the labels use: the extra records are zero
        labels = (cells % 2).astype(np.uint32)
        many = f.measure(0.0, labels, n_groups=300)
        _check(many, mm.measure(shape, CELL, cells, values, labels=labels, n_groups=300), FIRST, CELL, "300 groups")
        assert all(m[:7] == (0, 0, 0, 0, 0, 0, (0, 0, 0)) for m in many[2:]) and many[0].n_vertices > 0 and many[1].n_vertices > 0


# ---- 6. past 2^32 points ---------------------------------------------------------------------------------------------------------------------
def test_a_band_at_the_far_corner_of_a_grid_past_2_to_the_32():
    big = (1700, 1600, 1600)
    assert big[0] * big[1] * big[2] > 2 ** 32 and mm.moment_limit_ok(big)
    win = bw.Window(big, tuple(n - 20 for n in big), (20, 20, 20))
    # a sphere the three far faces cut, and a whole one beside it
    d = np.minimum(mm.sphere_distance(win.shape, (15.3, 14.6, 15.9), 6.2), mm.sphere_distance(win.shape, (5.2, 5.4, 5.1), 3.1))
    cells_w, values = mm.band_of(d, 2.0)
    cells = win.to_big(cells_w)
    assert (cells > 2 ** 32).all() and int(cells[-1]) == big[0] * big[1] * big[2] - 1
    labels = (d.reshape(-1)[cells_w.astype(np.int64)] == mm.sphere_distance(win.shape, (5.2, 5.4, 5.1), 3.1).reshape(-1)[cells_w.astype(np.int64)]).astype(np.uint32)
    with _field(Grid(list(FIRST), list(CELL), list(big)), cells, values, True) as f:
        want = mm.measure(big, CELL, cells, values, box=(win.lo, win.shape))
        assert int(want.n_border[0]) > 20 and int(want.n_triangles[0]) > 500 and abs(int(want.moment_q[0, 0])) > 2 ** 32
        _check(f.measure(), want, FIRST, CELL, "past 2^32")
        parts = f.measure(0.0, labels, n_groups=2)
        _check(parts, mm.measure(big, CELL, cells, values, labels=labels, n_groups=2, box=(win.lo, win.shape)), FIRST, CELL, "past 2^32, two groups")
        assert parts[1].closed and parts[1].euler == 2 and not parts[0].closed
        assert np.asarray(parts[1].centroid) == pytest.approx(np.asarray(FIRST, np.float64) + (np.asarray(win.lo) + (5.2, 5.4, 5.1)) * np.asarray(CELL), abs=1e-3)
    torch.cuda.empty_cache()


# ---- 7. what a real handle rejects, and the consumers ----------------------------------------------------------------------------------------
def test_the_call_rejects_bad_options_and_grids_past_the_moment_limit():
    L = _lib.lib()
    BAD = _lib.ERR_BAD_ARG
    out = (_lib.M2SBandMeasureRecord * 1)()

    def opts(**kw):
        o = _lib.M2SOpts()
        o.struct_size, o.device, o.mem_kind = C.sizeof(o), -1, _lib.MEM_DEVICE
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)

    with _field(Grid(list(FIRST), list(CELL), [4, 4, 4]), np.arange(64), np.linspace(-1, 1, 64).astype(F), True) as f:
        assert L.m2s_band_measure(f._h, None, None, 0, opts(), out, None, None) == _lib.M2S_OK and out[0].n_triangles > 0
        assert L.m2s_band_measure(f._h, None, None, 0, opts(device=1), out, None, None) == BAD and "device" in _lib.last_error()
        for field, value in (("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4), ("mem_kind", 5)):
            assert L.m2s_band_measure(f._h, None, None, 0, opts(**{field: value}), out, None, None) == BAD, field
        with pytest.raises(M2SError):
            f.measure(0.0, np.zeros(3, np.uint32), n_groups=2)          # one label per cell
        with pytest.raises(M2SError):
            f.measure(float("nan"))
        tm = _lib.M2STimings()
        assert L.m2s_band_measure(f._h, None, None, 0, opts(), out, None, C.byref(tm)) == _lib.M2S_OK and tm.total_ms > 0 and tm.n_units == 64
    with _field(Grid(list(FIRST), list(CELL), [1 << 26, 1, 1]), np.array([5, 6]), np.array([-1, 1], F), True) as f:
        assert L.m2s_band_measure(f._h, None, None, 0, opts(), out, None, None) == BAD and "2^50" in _lib.last_error()
    with _field(Grid(list(FIRST), list(CELL), [1 << 24, 2, 1]), np.array([5, 7]), np.array([-1, 1], F), True) as f:
        m = f.measure()                                                  # 2^25 points times 2^24: within the limit
        assert (m.n_triangles, m.n_vertices, m.n_border) == (0, 1, 1)


@pytest.mark.parametrize("cc,std,src", CONSUMERS)
def test_c_and_cpp_consumers_run_clean(tmp_path, cc, std, src):
    r = subprocess.run([build_consumer(tmp_path, cc, std, src), "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
