"""m2s_band_redistance on the GPU, bit for bit against tests/band_redistance_model.py (the definition in numpy): random bands on the
smallest grids where the kernels can go wrong, a sphere, a box and a union of two spheres, the untouched zero set, a band grown and then
used (isosurface at an offset, sample, march), idempotence and the truncated iterates (the test that catches a sweep that is not Jacobi),
BandField.offset, and what the call rejects.  Every comparison with the model is exact equality of bits, plus the info fields."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import band_csg_model as cm
import band_redistance_model as rm
import grid_query_model as gqm
from mesh_to_sdf_amd import BandField, Grid, M2SError, M2STimings, RedistanceInfo, SampleMode, _lib, raymarch_grid, sample_grid

F = np.float32
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [SampleMode.Snap, SampleMode.Trilinear, SampleMode.Tetrahedral]
FMAX = np.finfo(F).max
CELL = (0.125, 0.25, 0.1875)                                   # the random bands' cells
SPECIAL = np.array([0.0, -0.0, 0.5, -0.5, 0.75, -0.75, FMAX, -FMAX], F)   # zeros of both signs, values beyond the widths, +-f32::MAX
HZ = rm.CELLS[2]


def _np(x):
    if hasattr(x, "cpu"):
        if x.dtype == getattr(torch, "uint32", None):
            x = x.view(torch.int32)
        x = x.cpu().numpy()
    return np.asarray(x)


def _grid(shape):
    return Grid([-0.5, 0.25, 0.0], list(CELL), list(shape))


def _random_band(rng, shape, density=0.5, bits=True, bg=(0.75, 0.5), special=0.3):
    total = shape[0] * shape[1] * shape[2]
    cells = np.flatnonzero(rng.random(total) < density)
    d = rng.uniform(-1, 1, cells.size).astype(F)
    pick = rng.random(cells.size) < special
    d[pick] = rng.choice(SPECIAL, int(pick.sum()))
    mask = rng.integers(0, 2 ** 32, (shape[0], shape[1], (shape[2] + 31) // 32), dtype=np.uint64).astype(np.uint32) if bits else None
    return cm.Band(shape, cells, d, mask, *bg)


def _smooth_band(rng, shape, bits=True):
    """A band with long same-sign runs, so that the sweeps have somewhere to go: a random low-order trigonometric field's band."""
    i, j, k = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    a = rng.uniform(0.2, 0.9, 3)
    d = (np.sin(a[0] * i + rng.uniform(0, 6)) + np.sin(a[1] * j + rng.uniform(0, 6)) + np.sin(a[2] * k + rng.uniform(0, 6))).astype(F) * F(0.2)
    d = d.reshape(-1)
    cells = np.flatnonzero((np.abs(d) <= 0.3) & (rng.random(d.size) < 0.9))
    mask = cm.pack_bits(shape, (d < 0).reshape(shape)) if bits else None
    return cm.Band(shape, cells, d[cells], mask, 0.75, 0.5)


def _field(grid, band, device):
    """The BandField of a model Band, from device tensors or host arrays."""
    bg = (float(band.bg_in), float(band.bg_out))
    if device:
        bits = None if band.bits is None else torch.as_tensor(np.ascontiguousarray(band.bits).view(np.int32), device=DEV)
        return BandField(grid, torch.as_tensor(band.cells, device=DEV), torch.as_tensor(band.distances, device=DEV), background=bg, inside=bits)
    return BandField(grid, band.cells.astype(np.uint64), band.distances, background=bg, inside=band.bits)


def _band(field):
    """A handle's lists as a model Band (a result always has a sign mask)."""
    nb = field.to_band()
    return cm.Band(tuple(int(v) for v in field.grid.get_cell_count()), _np(nb.cells).astype(np.int64), _np(nb.distances),
                   _np(nb.bits).view(np.uint32), field.background[1], field.background[0])


def _check(field, want, info, what):
    """A redistanced handle against the model's (Band, Info): the export's three arrays, the backgrounds, the info, m2s_band_info."""
    got = _band(field)
    assert got.cells.size == want.cells.size == field.count, f"{what}: {got.cells.size} cells, the model has {want.cells.size}"
    assert np.array_equal(got.cells, want.cells), f"{what}: cells differ"
    differ = got.distances.view(np.uint32) != want.distances.view(np.uint32)
    assert not differ.any(), f"{what}: {int(differ.sum())} distances differ, first at cell {want.cells[np.flatnonzero(differ)[0]]}"
    assert cm.same(got, want), f"{what}: sign mask or backgrounds differ"
    ri = field.redistance_info
    assert isinstance(ri, RedistanceInfo)
    assert (ri.sweeps, int(ri.converged), ri.n_frozen, ri.n_open, ri.n_candidates) == tuple(info), f"{what}: info {ri}, the model has {info}"
    n, nbytes = C.c_uint64(0), C.c_uint64(0)
    assert _lib.lib().m2s_band_info(field._h, None, C.byref(n), C.byref(nbytes)) == _lib.M2S_OK
    words = (want.total + 63) // 64
    assert n.value == want.cells.size and nbytes.value == 24 * words + 4 * n.value == field.device_bytes, what


# ---- 1. random bands on the shapes where the kernels can go wrong ------------------------------------------------------------------------
# 1x1x1, 2x2x2: every neighbour test at a face.  5x3x70: rows longer than a word, words that straddle rows.  3x65x1: nz = 1, a word holds
# 64 rows.  7x9x11: rows shorter than a word, the total no multiple of 64.  24x20x28: several units' worth of rows.  70x64x64: 4480 mask
# words, 18 units, more than one group of 16: the scanned sums and the v_readlane loops cross a group boundary.
SHAPES = [(1, 1, 1), (2, 2, 2), (5, 3, 70), (3, 65, 1), (7, 9, 11), (24, 20, 28), (70, 64, 64)]
WIDTHS = (0.0, 0.5, 2.5)                                          # in cells of hz


@pytest.mark.parametrize("shape", SHAPES, ids=lambda n: "x".join(map(str, n)))
def test_random_bands(shape):
    rng = np.random.default_rng(100 + sum(shape))
    grid = _grid(shape)
    big = shape[0] * shape[1] * shape[2] > 100000
    cases = [("random", _random_band(rng, shape)), ("smooth", _smooth_band(rng, shape)), ("smooth, no mask", _smooth_band(rng, shape, bits=False))]
    if not big:
        cases += [("sparse", _random_band(rng, shape, 0.05, special=1.0)), ("dense, no mask", _random_band(rng, shape, 0.95, bits=False)),
                  ("full", _random_band(rng, shape, 1.1, special=0.1)), ("empty", _random_band(rng, shape, 0.0)),
                  ("empty, no mask", _random_band(rng, shape, 0.0, bits=False))]
    seen = set()
    for at, (name, band) in enumerate(cases):
        ext, inn = (F(w * CELL[2]) for w in rng.choice(WIDTHS, 2))
        if name == "smooth":
            ext, inn = F(2.5 * CELL[2]), F(0.5 * CELL[2])
        seen.add((float(ext), float(inn)))
        want, info = rm.redistance(band, CELL, ext, inn)
        assert info.converged == 1, f"{shape} {name}: the model needs more than the default cap"
        with _field(grid, band, device=at % 2 == 0) as f, f.redistance((float(inn), float(ext))) as r:
            _check(r, want, info, f"{shape} {name} widths {ext} {inn}")
    assert len(seen) > 1 or shape == (1, 1, 1)


def test_an_explicit_background_and_a_narrower_band():
    shape = (7, 9, 11)
    rng = np.random.default_rng(7)
    band = _smooth_band(rng, shape)
    with _field(_grid(shape), band, True) as f:
        want, info = rm.redistance(band, CELL, 0.1, 0.05, background=(2.0, 0.125))
        with f.redistance((0.05, 0.1), background=(0.125, 2.0)) as r:
            _check(r, want, info, "explicit background")
            assert r.background == (0.125, 2.0) and r.count < f.count


# ---- 2. shapes ---------------------------------------------------------------------------------------------------------------------------------
GRID = Grid(list(rm.FIRST), list(rm.CELLS), list(rm.SHAPE))
W3 = F(3 * HZ)


@pytest.fixture(scope="module")
def solids():
    """The model's inputs and results, computed once: name -> (input Band(s), result Band, Info)."""
    sphere = rm.band_of(rm.sphere((0, 0, 0), 0.6), 1.8 * HZ)
    box = rm.band_of(rm.box((0.5, 0.4, 0.7)), 2 * HZ)
    a, b = rm.band_of(rm.sphere((-0.25, 0, 0), 0.5), 4 * HZ), rm.band_of(rm.sphere((0.3, 0.05, 0), 0.45), 4 * HZ)
    union = cm.csg(a, b, cm.UNION)
    return {"sphere": (sphere,) + rm.redistance(sphere, rm.CELLS, W3, W3), "box": (box,) + rm.redistance(box, rm.CELLS, W3, W3),
            "union": ((a, b),) + rm.redistance(union, rm.CELLS, W3, W3)}


@pytest.mark.parametrize("name", ["sphere", "box", "union"])
def test_shapes_equal_the_model_and_converge(solids, name):
    src, want, info = solids[name]
    assert info.converged == 1 and info.n_open == 0 and info.n_frozen > 1000
    if name == "union":
        with _field(GRID, src[0], True) as fa, _field(GRID, src[1], True) as fb, fa.union(fb) as fu, fu.redistance(float(W3)) as r:
            _check(r, want, info, name)                                   # csg and redistance of the two models chained
            assert r.redistance_info.converged
    else:
        with _field(GRID, src, True) as f, f.redistance(float(W3)) as r:
            _check(r, want, info, name)
            assert r.redistance_info.converged


# ---- 3. the zero set is untouched --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "union"])
def test_the_zero_set_is_untouched(solids, name):
    src = solids[name][0]
    with (_field(GRID, src, True) if name == "sphere" else _field(GRID, cm.csg(src[0], src[1], cm.UNION), True)) as f, f.redistance(float(W3)) as r:
        v0, i0, open0 = f.isosurface(0.0)
        v1, i1, open1 = r.isosurface(0.0)
        assert open0 == 0 and open1 == 0 and v0.shape[0] > 1000
        assert gqm.same_bits(_np(v0), _np(v1)) and np.array_equal(_np(i0), _np(i1))


# ---- 4. growth and use -----------------------------------------------------------------------------------------------------------------------
def test_a_grown_band_serves_an_offset_isosurface_a_sample_and_a_march(solids):
    sphere = solids["sphere"][0]
    w5 = F(5 * HZ)
    want, info = rm.redistance(sphere, rm.CELLS, w5, w5)
    rng = np.random.default_rng(21)
    q = gqm.GridQ.of(GRID)
    lo, hi = q.start - q.cs, q.end + q.cs
    pts = torch.as_tensor((lo + rng.random((3000, 3)) * (hi - lo)).astype(F), device=DEV)
    org = torch.as_tensor((lo + rng.random((300, 3)) * (hi - lo)).astype(F), device=DEV)
    dirs = rng.normal(size=(300, 3))
    dirs = torch.as_tensor((dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(F), device=DEV)
    iso = float(F(3 * HZ))
    with _field(GRID, sphere, True) as f, f.redistance(float(w5)) as r:
        _check(r, want, info, "sphere, 5 cells")
        assert r.count > 1.5 * f.count
        v, i, n_open = r.isosurface(iso)
        assert n_open == 0 and v.shape[0] > 1000
        radius = np.linalg.norm(_np(v).astype(np.float64), axis=1)
        # the offset surface: the definition's error at 5 cells is 0.30 cells (tests/test_band_redistance_cpu.py asserts it at 0.372),
        # and linear interpolation on a sphere of 9 cells' radius adds h^2 / 8 R, under 0.02 cells
        assert np.abs(radius - (0.6 + iso)).max() < 0.4 * HZ
        # the 1.8-cell input cannot serve that level: the call raises, reports open cells, or (every value of the band lies below
        # iso, so no active edge crosses it) returns no surface at all
        try:
            v_in, _, n_open_in = f.isosurface(iso)
        except M2SError:
            v_in, n_open_in = None, -1
        assert n_open_in != 0 or v_in.shape[0] == 0
        dense = torch.as_tensor(cm.dense(want)[1].reshape(-1), device=DEV)         # D' of the model's result
        for mode in MODES:
            gv, gn = r.sample(pts, mode=mode, normals=True)
            wv, wn = sample_grid(GRID, dense, pts, mode=mode, normals=True)
            assert gqm.same_bits(_np(gv), _np(wv)) and gqm.same_bits(_np(gn), _np(wn)), mode
            got = r.raymarch(org, dirs, mode=mode, max_steps=40, normals=True)
            ref = raymarch_grid(GRID, dense, org, dirs, mode=mode, max_steps=40, normals=True)
            for g, w in zip(got, ref):
                g, w = _np(g), _np(w)
                assert gqm.same_bits(g, w) if g.dtype == F else np.array_equal(g, w), mode


# ---- 5. idempotence, and the truncated iterates: what a sweep that is not Jacobi fails ---------------------------------------------------------
def test_idempotence_and_the_truncated_iterates(solids):
    (a, b), want, info = solids["union"]
    union = cm.csg(a, b, cm.UNION)
    with _field(GRID, union, True) as f:
        with f.redistance(float(W3)) as r, r.redistance(float(W3)) as again:
            _check(r, want, info, "union")
            want2, info2 = rm.redistance(want, rm.CELLS, W3, W3)
            _check(again, want2, info2, "union twice")
            assert cm.same(want2, want) and cm.same(_band(again), _band(r))
        for n in (1, 2, 3, 5):
            wn, infon = rm.redistance(union, rm.CELLS, W3, W3, max_sweeps=n)
            assert infon == (n, 0) + tuple(info[2:])
            with f.redistance(float(W3), max_sweeps=n) as r:
                _check(r, wn, infon, f"union, {n} sweeps")
        # a cap that is exactly the number of changing sweeps: all run, none found unchanged
        wn, infon = rm.redistance(union, rm.CELLS, W3, W3, max_sweeps=info.sweeps)
        assert infon.converged == 0 and cm.same(wn, want)
        with f.redistance(float(W3), max_sweeps=info.sweeps) as r:
            _check(r, wn, infon, "union, a cap at the last changing sweep")
        with f.redistance(float(W3), max_sweeps=info.sweeps + 1) as r:
            _check(r, want, info, "union, one sweep more")


# ---- 6. offset -------------------------------------------------------------------------------------------------------------------------------
# +-2 cells of hy = 0.04, not of hz: the grid reaches 0.70 in y, so the sphere of radius 0.6 grown by 2 hz would leave it.  The bound is
# max |r - (analytic -+ 2 hy)| / hz of the MODEL's offset results (tests/test_band_redistance_cpu.py measures and asserts them), times 1.25.
OFFSET_BOUND = {2: 1.25 * 0.1247, -2: 1.25 * 0.1769}
HY = rm.CELLS[1]


@pytest.mark.parametrize("cells", [2, -2])
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_offset_on_the_sphere(cells, device):
    analytic = rm.sphere((0, 0, 0), 0.6)
    src = rm.band_of(analytic, 4 * HZ)
    dist = float(F(cells * HY))
    want, info = rm.offset(src, rm.CELLS, dist, W3, W3)
    with _field(GRID, src, device) as f, f.offset(dist, float(W3)) as r:
        _check(r, want, info, f"offset {cells}")
        got = _band(r)
        err = np.abs(got.distances.astype(np.float64) - (analytic.reshape(-1)[got.cells] - dist)).max() / HZ
        print(f"offset by {cells} hy: max error {err:.4f} cells")
        assert err <= OFFSET_BOUND[cells] and r.redistance_info.n_open == 0
        assert torch.is_tensor(r.to_band().cells) == device
        assert (r.count > f.count * 0.8) == (cells > 0)                            # the solid grew, or shrank


def test_offset_beyond_the_band_raises():
    src = rm.band_of(rm.sphere((0, 0, 0), 0.6), 1.8 * HZ)
    with _field(GRID, src, True) as f:
        for cells in (3, -3):
            with pytest.raises(M2SError):
                f.offset(cells * HZ, float(W3))
        with f.offset(0.5 * HY, float(W3)) as r:                                   # within what the band brackets
            assert r.redistance_info.n_open == 0 and r.count > 0


# ---- 7. what the call rejects of a real handle ---------------------------------------------------------------------------------------------
def test_the_call_rejects_bad_options_and_reports_timings():
    shape = (7, 9, 11)
    rng = np.random.default_rng(15)
    band = _smooth_band(rng, shape)
    L = _lib.lib()
    BAD = _lib.ERR_BAD_ARG

    def call(f, ro=(16, 0.25, 0.25, 0), fo=None, opts=None, info=None):
        h = C.c_void_p(0x1234)
        rc = L.m2s_band_redistance(f._h, C.byref(_lib.M2SBandRedistanceOpts(*ro)) if ro else None, fo, opts, C.byref(h), info)
        assert (rc == _lib.M2S_OK) == (h.value is not None)                # *out = NULL on every failure
        if h.value is not None:
            L.m2s_band_destroy(h)
        return rc

    def opts(**kw):
        o = _lib.M2SOpts()
        o.struct_size, o.device = C.sizeof(o), -1
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)

    with _field(_grid(shape), band, True) as f:
        assert call(f) == _lib.M2S_OK
        assert call(f, ro=None) == BAD and "NULL" in _lib.last_error()
        for ro in ((12, 0.25, 0.25, 0), (16, -0.25, 0.25, 0), (16, 0.25, float("inf"), 0), (16, float("nan"), 0.25, 0)):
            assert call(f, ro=ro) == BAD, ro
        for size, out, ins in ((8, 0.5, 0.5), (12, -0.5, 0.5), (12, 0.5, float("inf")), (12, float("nan"), 0.5)):
            assert call(f, fo=C.byref(_lib.M2SBandFieldOpts(size, out, ins))) == BAD
        assert call(f, info=C.byref(_lib.M2SBandRedistanceInfo(8))) == BAD
        assert call(f, opts=opts(device=1)) == BAD and "device" in _lib.last_error()
        assert call(f, opts=opts(device=0)) == _lib.M2S_OK
        for field, value in (("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4), ("mem_kind", 5)):
            assert call(f, opts=opts(**{field: value})) == BAD, field
        assert L.m2s_band_redistance(f._h, C.byref(_lib.M2SBandRedistanceOpts(16, 0.25, 0.25, 0)), None, None, None, None) == BAD
        t = M2STimings()
        with f.redistance(0.25, timings=t) as r:
            assert t.n_units == r.count > 0 and t.seed_ms > 0 and t.distance_ms > 0 and t.total_ms >= t.seed_ms + t.distance_ms
        with pytest.raises(M2SError):
            f.redistance(-1.0)


def test_c_and_cpp_consumers_run_clean(tmp_path):
    for cc, std, src, extra in (("gcc", "-std=c99", "tests/c/band_redistance_smoke.c", ["-lm"]),
                                ("g++", "-std=c++17", "tests/cpp/band_redistance_tests.cpp", [])):
        exe = str(tmp_path / os.path.basename(src).split(".")[0])
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                               os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                               "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", *extra, "-o", exe])
        r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
