"""m2s_band_filter on the GPU, bit for bit against tests/band_filter_model.py (the definition in numpy): random bands on the smallest
grids where the kernels can go wrong, for each kind at 1, 2, 3 and 5 iterations (the test a pass that is not Jacobi fails), everywhere,
inside a random region and inside the band itself, with explicit and default backgrounds; the chain union -> fillet -> redistance ->
isosurface / sample / march; and what the call rejects.  Every comparison with the model is exact equality of bits, plus the info."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import band_csg_model as cm
import band_filter_model as fm
import band_redistance_model as rm
import grid_query_model as gqm
from mesh_to_sdf_amd import BandField, FilterInfo, FilterKind, Grid, M2SError, M2STimings, SampleMode, _lib, raymarch_grid, sample_grid

F = np.float32
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [SampleMode.Snap, SampleMode.Trilinear, SampleMode.Tetrahedral]
FMAX = np.finfo(F).max
CELL = (0.125, 0.25, 0.1875)                                   # the random bands' cells
SPECIAL = np.array([0.0, -0.0, 0.5, -0.5, 0.75, -0.75, 2.0, -2.0, FMAX, -FMAX], F)   # zeros of both signs, values beyond the backgrounds, +-f32::MAX
HZ = rm.CELLS[2]
KINDS = {fm.MEAN: FilterKind.Mean, fm.LAPLACIAN: FilterKind.Laplacian, fm.MEAN_CURVATURE: FilterKind.MeanCurvature}


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
    """A random low-order trigonometric field's band: neighbouring values that belong together, so that many passes stay finite."""
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
    """A filtered handle against the model's (Band, Info): the export's three arrays, the backgrounds, every info field, m2s_band_info."""
    got = _band(field)
    assert got.cells.size == want.cells.size == field.count, f"{what}: {got.cells.size} cells, the model has {want.cells.size}"
    assert np.array_equal(got.cells, want.cells), f"{what}: cells differ"
    differ = got.distances.view(np.uint32) != want.distances.view(np.uint32)
    assert not differ.any(), f"{what}: {int(differ.sum())} distances differ, first at cell {want.cells[np.flatnonzero(differ)[0]]}"
    assert cm.same(got, want), f"{what}: sign mask or backgrounds differ"
    fi = field.filter_info
    assert isinstance(fi, FilterInfo)
    assert (fi.passes, fi.n_changed, fi.n_sign_flips, fi.n_nonfinite) == (info.passes, info.n_changed, info.n_sign_flips, info.n_nonfinite), \
        f"{what}: info {fi}, the model has {info}"
    assert F(fi.max_change).view(np.uint32) == F(info.max_change).view(np.uint32), f"{what}: max_change {fi.max_change}, the model has {info.max_change}"
    n, nbytes = C.c_uint64(0), C.c_uint64(0)
    assert _lib.lib().m2s_band_info(field._h, None, C.byref(n), C.byref(nbytes)) == _lib.M2S_OK
    words = (want.total + 63) // 64
    assert n.value == want.cells.size and nbytes.value == 24 * words + 4 * n.value == field.device_bytes, what


# ---- 1. random bands on the shapes where the kernels can go wrong ------------------------------------------------------------------------
# 1x1x1, 2x2x2: every read clamped, diagonal neighbours that collapse onto the cell or an axis neighbour.  5x3x70: rows longer than a word,
# words that straddle rows.  3x65x1: nz = 1.  7x9x11: rows shorter than a word, a total that is no multiple of 64.  24x20x28: several
# units' worth of rows.  70x64x64: 4480 mask words, 18 units, more than one group of 16.
SHAPES = [(1, 1, 1), (2, 2, 2), (5, 3, 70), (3, 65, 1), (7, 9, 11), (24, 20, 28), (70, 64, 64)]
ITERATIONS = (1, 2, 3, 5)


@pytest.mark.parametrize("kind", list(KINDS), ids=["mean", "laplacian", "mean_curvature"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda n: "x".join(map(str, n)))
def test_random_bands(shape, kind):
    rng = np.random.default_rng(1000 * kind + sum(shape))
    grid = _grid(shape)
    big = shape[0] * shape[1] * shape[2] > 100000
    cases = [("random", _random_band(rng, shape)), ("smooth", _smooth_band(rng, shape)), ("smooth, no mask", _smooth_band(rng, shape, bits=False))]
    if not big:
        cases += [("sparse", _random_band(rng, shape, 0.05, special=1.0)), ("dense, no mask", _random_band(rng, shape, 0.95, bits=False)),
                  ("full", _random_band(rng, shape, 1.1, special=0.1)), ("empty", _random_band(rng, shape, 0.0)),
                  ("empty, no mask", _random_band(rng, shape, 0.0, bits=False))]
    region = _random_band(rng, shape, 0.4)                                        # a random band with a sign mask
    nonfinite = 0
    with _field(grid, region, True) as fw:
        for at, (name, band) in enumerate(cases):
            with _field(grid, band, device=at % 2 == 0) as f:
                for n in ITERATIONS if name in ("random", "smooth") or not big and name == "full" else (ITERATIONS[at % 4],):
                    mode = (at + n) % 3                                           # everywhere, the random region, the band itself
                    where_model, where = (None, None) if mode == 0 else (region, fw) if mode == 1 else (band, f)
                    bg = (2.0, 0.125) if (at + n) % 2 else None                   # (outside, inside) of the model
                    want, info = fm.band_filter(band, CELL, kind, n, where=where_model, background=bg)
                    nonfinite += info.n_nonfinite
                    with f.filter(KINDS[kind], n, where=where, background=None if bg is None else (bg[1], bg[0])) as r:
                        _check(r, want, info, f"{shape} {name}, kind {kind}, {n} iterations, where {mode}, background {bg}")
    assert nonfinite > 0 or shape in ((1, 1, 1), (2, 2, 2))                       # the +-f32::MAX cells made candidates overflow


# ---- 2. the chain: union -> fillet -> redistance -> isosurface, sample, march ----------------------------------------------------------------
GRID = Grid(list(rm.FIRST), list(rm.CELLS), list(rm.SHAPE))
W3 = F(3 * HZ)
CA, RA, CB, RB = (-0.25, 0.0, 0.0), 0.5, (0.3, 0.05, 0.0), 0.45


def test_a_fillet_on_the_seam_of_a_union():
    da, db = rm.sphere(CA, RA), rm.sphere(CB, RB)
    a, b = rm.band_of(da, 4 * HZ), rm.band_of(db, 4 * HZ)
    where = rm.band_of(np.abs(da - db) - 2 * HZ, HZ)                               # within two cells of the crease, a band with a sign mask
    union = cm.csg(a, b, cm.UNION)
    filtered, finfo = fm.band_filter(union, rm.CELLS, fm.MEAN_CURVATURE, 8, where=where)
    want, rinfo = rm.redistance(filtered, rm.CELLS, W3, W3)
    assert finfo.n_changed > 300 and rinfo.converged == 1 and rinfo.n_open == 0
    rng = np.random.default_rng(23)
    q = gqm.GridQ.of(GRID)
    lo, hi = q.start - q.cs, q.end + q.cs
    pts = torch.as_tensor((lo + rng.random((2000, 3)) * (hi - lo)).astype(F), device=DEV)
    org = torch.as_tensor((lo + rng.random((200, 3)) * (hi - lo)).astype(F), device=DEV)
    dirs = rng.normal(size=(200, 3))
    dirs = torch.as_tensor((dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(F), device=DEV)
    with _field(GRID, a, True) as fa, _field(GRID, b, True) as fb, _field(GRID, where, True) as fw, fa.union(fb) as fu:
        with fu.filter(FilterKind.MeanCurvature, 8, where=fw) as ff:
            _check(ff, filtered, finfo, "the filtered union")
        with fu.smooth("mean_curvature", 8, float(W3), where=fw) as r:
            got = _band(r)
            assert cm.same(got, want), "the chain's lists differ from the model chain's"
            assert r.filter_info.n_changed == finfo.n_changed and r.redistance_info.n_open == 0 and bool(r.redistance_info.converged)
            v0, i0, open0 = fu.isosurface(0.0)
            v1, i1, open1 = r.isosurface(0.0)
            assert open0 == 0 and open1 == 0 and v1.shape[0] > 1000
            # a vertex lies on an edge between two cells at most 0.0625 from it, and |D_A - D_B| changes by at most 2 per unit length:
            # above 2 hz + 2 * 0.0625 both cells are outside the region and kept every bit, through the redistancing too (frozen cells)
            v0, v1 = _np(v0), _np(v1)

            def outside(v):
                p = v.astype(np.float64)
                apart = np.abs((np.linalg.norm(p - CA, axis=1) - RA) - (np.linalg.norm(p - CB, axis=1) - RB))
                return {row.tobytes() for row in v[apart > 2 * HZ + 0.125 + 1e-6]}
            kept0, kept1 = outside(v0), outside(v1)
            assert kept0 == kept1 and len(kept0) > 1000
            assert {row.tobytes() for row in v0} != {row.tobytes() for row in v1}              # and the seam moved
            dense = torch.as_tensor(cm.dense(want)[1].reshape(-1), device=DEV)                 # D' of the model's result
            for mode in MODES:
                gv, gn = r.sample(pts, mode=mode, normals=True)
                wv, wn = sample_grid(GRID, dense, pts, mode=mode, normals=True)
                assert gqm.same_bits(_np(gv), _np(wv)) and gqm.same_bits(_np(gn), _np(wn)), mode
                res = r.raymarch(org, dirs, mode=mode, max_steps=40, normals=True)
                ref = raymarch_grid(GRID, dense, org, dirs, mode=mode, max_steps=40, normals=True)
                for g, w in zip(res, ref):
                    g, w = _np(g), _np(w)
                    assert gqm.same_bits(g, w) if g.dtype == F else np.array_equal(g, w), mode


# ---- 3. what the call rejects of a real handle -------------------------------------------------------------------------------------------------
def test_the_call_rejects_bad_options_and_reports_timings():
    shape = (7, 9, 11)
    rng = np.random.default_rng(15)
    band = _smooth_band(rng, shape)
    L = _lib.lib()
    BAD = _lib.ERR_BAD_ARG

    def call(f, fl=(16, 1, 1, 1), where=None, fo=None, opts=None, info=None):
        h = C.c_void_p(0x1234)
        rc = L.m2s_band_filter(f._h, where._h if where is not None else None, C.byref(_lib.M2SBandFilterOpts(*fl)) if fl else None, fo, opts,
                               C.byref(h), info)
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

    with _field(_grid(shape), band, True) as f, _field(_grid((7, 9, 12)), _smooth_band(rng, (7, 9, 12)), True) as other, \
            _field(Grid([-0.5, 0.25, 0.125], list(CELL), list(shape)), band, True) as moved:
        assert call(f) == _lib.M2S_OK and call(f, where=f) == _lib.M2S_OK
        assert call(f, fl=None) == BAD and "NULL" in _lib.last_error()
        for fl in ((12, 1, 1, 1), (16, 3, 1, 1), (16, -1, 1, 1), (16, 1, 0, 1), (16, 1, 65537, 1), (16, 1, 1, 0), (16, 1, 1, 2)):
            assert call(f, fl=fl) == BAD, fl
        assert call(f, fl=(16, 0, 65536, 1), where=moved) == BAD                      # checked before any pass is launched
        for size, out, ins in ((8, 0.5, 0.5), (12, -0.5, 0.5), (12, 0.5, float("inf")), (12, float("nan"), 0.5)):
            assert call(f, fo=C.byref(_lib.M2SBandFieldOpts(size, out, ins))) == BAD
        assert call(f, info=C.byref(_lib.M2SBandFilterInfo(8))) == BAD
        assert call(f, where=other) == BAD and "grids differ" in _lib.last_error()      # another cell_count
        assert call(f, where=moved) == BAD and "grids differ" in _lib.last_error()      # another first_cell
        assert call(f, opts=opts(device=1)) == BAD and "device" in _lib.last_error()
        assert call(f, opts=opts(device=0)) == _lib.M2S_OK
        for field, value in (("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4), ("mem_kind", 5)):
            assert call(f, opts=opts(**{field: value})) == BAD, field
        assert L.m2s_band_filter(f._h, None, C.byref(_lib.M2SBandFilterOpts(16, 1, 1, 1)), None, None, None, None) == BAD
        t = M2STimings()
        with f.filter(FilterKind.MeanCurvature, 4, timings=t) as r:
            assert t.n_units == r.count == f.count > 0 and t.seed_ms > 0 and t.distance_ms > 0 and t.total_ms >= t.seed_ms + t.distance_ms
            assert r.filter_info.passes == 4 and r.background == f.background
        with f.filter("mean", 2) as r:
            assert r.filter_info.passes == 6
        for bad in (dict(kind=FilterKind.Mean, iterations=0), dict(kind=7), dict(kind="median")):
            with pytest.raises(M2SError):
                f.filter(**bad)


def test_c_and_cpp_consumers_run_clean(tmp_path):
    for cc, std, src, extra in (("gcc", "-std=c99", "tests/c/band_filter_smoke.c", ["-lm"]),
                                ("g++", "-std=c++17", "tests/cpp/band_filter_tests.cpp", [])):
        exe = str(tmp_path / os.path.basename(src).split(".")[0])
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                               os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                               "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", *extra, "-o", exe])
        r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
