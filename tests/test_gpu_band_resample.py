"""m2s_band_resample on the GPU, bit for bit against tests/band_resample_model.py (the definition in numpy): random bands between the
shapes where the index walks can go wrong, under the identity, a whole-cell shift, a turn with a scale, a quarter turn with a value scale,
a translation off the box and a map that overflows, in all three modes, with and without a source sign mask, from device tensors and
host arrays, with explicit and default backgrounds; the consequences the header states, through the API; the chain that motivates the
call (two fields born on different grids -> resample -> union -> redistance -> isosurface / sample / march); and what the call rejects.
Every comparison with the model is exact equality: cells, distance bits, the sign mask on every point, both backgrounds, all four info
counts and m2s_band_info."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import band_csg_model as cm
import band_redistance_model as rm
import band_resample_model as rsm
import grid_query_model as gqm
from mesh_to_sdf_amd import BandField, Grid, M2SError, M2STimings, ResampleInfo, SampleMode, _lib, raymarch_grid, sample_grid

F = np.float32
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [SampleMode.Snap, SampleMode.Trilinear, SampleMode.Tetrahedral]
FMAX = np.finfo(F).max
FIRST = (-0.5, 0.25, 0.0)
CELL = (0.125, 0.25, 0.1875)                                   # the random bands' cells
SPECIAL = np.array([0.0, -0.0, 0.5, -0.5, 0.75, -0.75, 2.0, -2.0, FMAX, -FMAX], F)   # zeros of both signs, values beyond the backgrounds, +-f32::MAX
HZ = rm.CELLS[2]


def _np(x):
    if hasattr(x, "cpu"):
        if x.dtype == getattr(torch, "uint32", None):
            x = x.view(torch.int32)
        x = x.cpu().numpy()
    return np.asarray(x)


def _grid(spec):
    return Grid(list(spec.first), list(spec.cell), list(spec.shape))


def _random_band(rng, shape, density=0.5, bits=True, bg=(0.75, 0.5), special=0.3):
    total = shape[0] * shape[1] * shape[2]
    cells = np.flatnonzero(rng.random(total) < density)
    d = rng.uniform(-1, 1, cells.size).astype(F)
    pick = rng.random(cells.size) < special
    d[pick] = rng.choice(SPECIAL, int(pick.sum()))
    mask = rng.integers(0, 2 ** 32, (shape[0], shape[1], (shape[2] + 31) // 32), dtype=np.uint64).astype(np.uint32) if bits else None
    return cm.Band(shape, cells, d, mask, *bg)


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


def _raw(field, grid, to_source, scale, mode, background=None):
    """m2s_band_resample itself, for maps the wrapper would not make -> a BandField with .resample_info."""
    ro = _lib.M2SBandResampleOpts()
    ro.struct_size, ro.mode, ro.value_scale = C.sizeof(ro), int(mode), float(scale)
    ro.to_source[:] = [float(v) for v in to_source]
    fo = None if background is None else C.byref(_lib.M2SBandFieldOpts(12, float(F(background[0])), float(F(background[1]))))
    info = _lib.M2SBandResampleInfo(C.sizeof(_lib.M2SBandResampleInfo))
    h = C.c_void_p()
    rc = _lib.lib().m2s_band_resample(field._h, C.byref(grid._g), C.byref(ro), fo, None, C.byref(h), C.byref(info))
    assert rc == _lib.M2S_OK, _lib.last_error()
    out = BandField._adopt(h, grid, field._dev)
    out.resample_info = ResampleInfo(int(info.n_cells), int(info.n_partial), int(info.n_nonfinite), int(info.n_open))
    return out


def _check(field, want, info, what):
    """A resampled handle against the model's (Band, Info): the export's three arrays, the backgrounds, every info field, m2s_band_info."""
    got = _band(field)
    assert got.shape == want.shape, what
    assert got.cells.size == want.cells.size == field.count, f"{what}: {got.cells.size} cells, the model has {want.cells.size}"
    assert np.array_equal(got.cells, want.cells), f"{what}: cells differ"
    differ = got.distances.view(np.uint32) != want.distances.view(np.uint32)
    assert not differ.any(), f"{what}: {int(differ.sum())} distances differ, first at cell {want.cells[np.flatnonzero(differ)[0]]}"
    assert np.array_equal(got.bits, want.bits), f"{what}: the sign mask differs on {int((cm.unpack_bits(want.shape, got.bits) != cm.unpack_bits(want.shape, want.bits)).sum())} points"
    assert cm.same(got, want), f"{what}: backgrounds differ: {got.bg_out, got.bg_in}, the model has {want.bg_out, want.bg_in}"
    ri = field.resample_info
    assert isinstance(ri, ResampleInfo) and tuple(ri) == tuple(info), f"{what}: info {ri}, the model has {info}"
    n, nbytes = C.c_uint64(0), C.c_uint64(0)
    assert _lib.lib().m2s_band_info(field._h, None, C.byref(n), C.byref(nbytes)) == _lib.M2S_OK
    words = (want.total + 63) // 64
    assert n.value == want.cells.size and nbytes.value == 24 * words + 4 * n.value == field.device_bytes, what


# ---- 1. random bands between the shapes where the index walks can go wrong ----------------------------------------------------------------
# 1x1x1, 2x2x2: every read clamped.  5x3x70: rows longer than a word, words that straddle rows.  3x65x1: nz = 1.  7x9x11: rows shorter than a
# word, a total that is no multiple of 64.  24x20x28: several units' worth of rows.  70x64x64: 4480 mask words, 70 units, more than one group.
PAIRS = [((1, 1, 1), (2, 2, 2)), ((2, 2, 2), (1, 1, 1)), ((5, 3, 70), (3, 65, 1)), ((3, 65, 1), (7, 9, 11)), ((7, 9, 11), (5, 3, 70)),
         ((24, 20, 28), (24, 20, 28)), ((24, 20, 28), (70, 64, 64)), ((70, 64, 64), (7, 9, 11))]
PERM = (1, 2, 0)


def _centre(spec):
    return np.array([spec.first[a] + (spec.shape[a] - 1) * spec.cell[a] / 2 for a in range(3)])


def _around(centre, cell, shape):
    """The grid of `shape` cells of `cell` whose centre is `centre`."""
    return rsm.GridSpec(tuple(float(centre[a] - (shape[a] - 1) * cell[a] / 2) for a in range(3)), tuple(cell), tuple(shape))


def _cases(src, tshape):
    """-> [(name, target GridSpec, forward map or None, raw to_source or None)]."""
    c = _centre(src)
    quarter = np.zeros((3, 3))
    for a, p in enumerate(PERM):
        quarter[a, p] = 1.0
    far = rsm.forward(1.0, np.eye(3), (1e6, 0, 0))
    return [("identity", rsm.GridSpec(src.first, src.cell, tshape), None, None),
            ("shift", rsm.GridSpec(tuple(src.first[a] + (2, -1, 3)[a] * src.cell[a] for a in range(3)), src.cell, tshape), None, None),
            ("turn", _around(c, src.cell, tshape), rsm.forward(rsm.MOVE_SCALE, rsm.rotation(rsm.MOVE_AXIS, rsm.MOVE_ANGLE), (0, 0, 0), about=c), None),
            ("quarter", _around(c, src.cell, tshape), rsm.forward(1.6, quarter, (0, 0, 0), about=c), None),
            ("far", rsm.GridSpec(src.first, src.cell, tshape), far, None),
            ("overflow", rsm.GridSpec(src.first, src.cell, tshape), None, [3e38] * 12)]


@functools.lru_cache(maxsize=None)
def _plan(sshape, tshape):
    """Everything of a shape pair from the model, on the CPU, once: -> (source GridSpec, bands, [(name, target, forward map, raw
    to_source, mode, band index, background, the model's Band, the model's Info)])."""
    rng = np.random.default_rng(sum(sshape) + 1000 * sum(tshape))
    src = rsm.GridSpec(FIRST, CELL, sshape)
    bands = [_random_band(rng, sshape, 0.85), _random_band(rng, sshape, 0.5, bits=False), _random_band(rng, sshape, 0.97, special=0.1)]
    plan = []
    at = 0
    big = tshape[0] * tshape[1] * tshape[2] > 100000                              # the model is dense over the target: one mode per map there
    for case, (name, tgt, fwd, raw) in enumerate(_cases(src, tshape)):
        for mode in (rsm.MODES[case % 3],) if big else rsm.MODES:
            which = (mode + case) % len(bands)
            bg = (2.0, 0.125) if at % 2 else None                                   # (outside, inside) of the model
            if raw is not None:
                to_source, scale = np.asarray(raw, F), F(1.0)
            elif fwd is not None:
                to_source, scale = rsm.similarity(fwd)
            else:
                to_source, scale = None, F(1.0)
            want, info = rsm.resample(bands[which], src, tgt, to_source, scale, mode, background=bg)
            plan.append((name, tgt, fwd, raw, mode, which, bg, want, info))
            at += 1
    return src, bands, plan


@pytest.mark.parametrize("sshape,tshape", PAIRS, ids=lambda n: "x".join(map(str, n)))
def test_random_bands(sshape, tshape):
    src, bands, plan = _plan(sshape, tshape)
    if sshape[0] * sshape[1] * sshape[2] > 8 and tshape[0] * tshape[1] * tshape[2] > 8:
        assert any(p[-1].n_cells > 0 for p in plan) and any(p[-1].n_partial > 0 for p in plan)       # no vacuous case set
    for p in plan:
        if p[0] in ("far", "overflow"):
            assert p[-1] == (0, 0, 0, 0) and not p[-2].bits.any()
    fields = [_field(_grid(src), b, device=i != 1) for i, b in enumerate(bands)]   # device tensors, host arrays, device tensors
    try:
        for name, tgt, fwd, raw, mode, which, bg, want, info in plan:
            f, g = fields[which], _grid(tgt)
            what = f"{sshape} -> {tshape} {name}, mode {mode}, band {which}, background {bg}"
            if raw is not None:
                r = _raw(f, g, raw, 1.0, mode, bg)
            else:
                r = f.resample(g, fwd, mode=MODES[mode], background=None if bg is None else (bg[1], bg[0]))
            with r:
                _check(r, want, info, what)
    finally:
        for f in fields:
            f.close()


def test_the_case_sets_reach_the_non_finite_rule():
    """Over all of test_random_bands' cases (the model's side of them, shared with it): a scale of 1.6 over an f32::MAX cell makes r
    overflow, so some point has full support and a non-finite value; the GPU's count of them was compared above, case by case."""
    assert sum(p[-1].n_nonfinite for pair in PAIRS for p in _plan(*pair)[2]) > 0


# ---- 2. the consequences, through the API ---------------------------------------------------------------------------------------------------------
def test_snap_gives_the_band_back_and_pad_then_crop_keeps_every_bit():
    rng = np.random.default_rng(29)
    for first, cell in ((FIRST, CELL), ((1000.3, -77.7, 0.003), (0.1, 0.3, 0.7))):
        for shape, bits in (((7, 9, 11), True), ((5, 3, 70), False)):
            src = rsm.GridSpec(first, cell, shape)
            band = _random_band(rng, shape, bits=bits)
            s = cm.dense(band)[2]
            with _field(_grid(src), band, True) as f, f.resample(f.grid, mode=SampleMode.Snap) as same:
                got, own = _band(same), f.to_band()
                assert np.array_equal(got.cells, _np(own.cells).astype(np.int64)) and np.array_equal(got.cells, band.cells)
                assert np.array_equal(got.distances.view(np.uint32), _np(own.distances).view(np.uint32))
                assert np.array_equal(cm.unpack_bits(shape, got.bits), s) and same.background == f.background
                assert same.resample_info.n_cells == f.count and same.resample_info.n_partial == 0
                if first != FIRST:
                    continue                                                        # pad and crop need centres that agree: the dyadic grid
                pad = rsm.GridSpec(tuple(first[a] - (3, 2, 5)[a] * cell[a] for a in range(3)), cell, tuple(shape[a] + (6, 4, 10)[a] for a in range(3)))
                with f.resample(_grid(pad), mode=SampleMode.Snap) as padded, padded.resample(f, mode=SampleMode.Snap) as back:
                    assert padded.count >= f.count and padded.grid.get_cell_count() == list(pad.shape)
                    got = _band(back)
                    assert np.array_equal(got.cells, band.cells) and np.array_equal(got.distances.view(np.uint32), band.distances.view(np.uint32))
                    assert np.array_equal(cm.unpack_bits(shape, got.bits), s) and back.background == f.background


# ---- 3. the chain that motivates the call ----------------------------------------------------------------------------------------------------------
def test_two_fields_born_on_different_grids_meet_in_a_union():
    tgt = rsm.GridSpec(rm.FIRST, rm.CELLS, rm.SHAPE)
    src = rsm.centred((60, 56, 54), (0.03, 0.032, 0.034))
    a = rm.band_of(rm.sphere((-0.25, 0.0, 0.0), 0.5), 4 * HZ)
    b = rm.band_of(rm.sphere((0, 0, 0), 0.6, first=src.first, cells=src.cell, shape=src.shape), 0.2)
    fwd = rsm.move()
    to_source, scale = rsm.similarity(fwd)
    W3 = F(3 * HZ)
    moved, minfo = rsm.resample(b, src, tgt, to_source, scale, rsm.TRILINEAR)
    want, rinfo = rm.redistance(cm.csg(a, moved, cm.UNION), rm.CELLS, W3, W3)
    assert minfo.n_cells > 5000 and minfo.n_open == 0 and rinfo.converged == 1 and rinfo.n_open == 0
    rng = np.random.default_rng(31)
    GRID = _grid(tgt)
    q = gqm.GridQ.of(GRID)
    lo, hi = q.start - q.cs, q.end + q.cs
    pts = torch.as_tensor((lo + rng.random((2000, 3)) * (hi - lo)).astype(F), device=DEV)
    org = torch.as_tensor((lo + rng.random((200, 3)) * (hi - lo)).astype(F), device=DEV)
    dirs = rng.normal(size=(200, 3))
    dirs = torch.as_tensor((dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(F), device=DEV)
    with _field(GRID, a, True) as fa, _field(_grid(src), b, True) as fb:
        with pytest.raises(M2SError, match="grids differ"):
            fa.union(fb)
        with fb.resample(fa, fwd) as fm:
            _check(fm, moved, minfo, "the moved sphere")
            with fa.union(fm) as fu, fu.redistance(float(W3)) as r:
                assert cm.same(_band(r), want), "the chain's lists differ from the model chain's"
                assert bool(r.redistance_info.converged) and r.redistance_info.n_open == 0 and r.redistance_info.sweeps == rinfo.sweeps
                v, i, n_open = r.isosurface(0.0)
                assert n_open == 0 and _np(v).shape[0] > 1000
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


# ---- 4. what the call rejects of a real handle, and the timings ---------------------------------------------------------------------------------
def test_the_call_rejects_bad_options_and_reports_timings():
    shape = (7, 9, 11)
    rng = np.random.default_rng(15)
    src = rsm.GridSpec(FIRST, CELL, shape)
    band = _random_band(rng, shape, 0.9)
    L = _lib.lib()
    BAD = _lib.ERR_BAD_ARG
    grid = _grid(src)

    def ropts(size=60, mode=1, m=rsm.IDENTITY, scale=1.0):
        ro = _lib.M2SBandResampleOpts()
        ro.struct_size, ro.mode, ro.value_scale = size, mode, scale
        ro.to_source[:] = [float(v) for v in m]
        return ro

    def call(f, g=grid, ro=None, fo=None, opts=None, info=None):
        h = C.c_void_p(0x1234)
        rc = L.m2s_band_resample(f._h, C.byref(g._g) if g is not None else None, C.byref(ro) if ro is not None else None, fo, opts, C.byref(h), info)
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

    with _field(grid, band, True) as f:
        assert call(f) == _lib.M2S_OK and call(f, ro=ropts()) == _lib.M2S_OK
        assert call(f, g=None) == BAD and "target is NULL" in _lib.last_error()
        for kw in (dict(size=56), dict(size=64), dict(mode=3), dict(mode=-1), dict(scale=0.0), dict(scale=-2.0), dict(scale=float("nan")),
                   dict(scale=float("inf")), dict(m=[float("nan")] + [0.0] * 11), dict(m=list(rsm.IDENTITY[:11]) + [float("inf")])):
            assert call(f, ro=ropts(**kw)) == BAD, kw
        for size, out, ins in ((8, 0.5, 0.5), (12, -0.5, 0.5), (12, 0.5, float("inf")), (12, float("nan"), 0.5)):
            assert call(f, fo=C.byref(_lib.M2SBandFieldOpts(size, out, ins))) == BAD
        assert call(f, info=C.byref(_lib.M2SBandResampleInfo(8))) == BAD
        assert call(f, g=Grid(list(FIRST), list(CELL), [4096, 4096, 4096])) == BAD and "2^36" in _lib.last_error()
        assert call(f, g=Grid(list(FIRST), [0.125, 0.0, 0.1875], list(shape))) == BAD
        assert call(f, g=Grid(list(FIRST), list(CELL), [7, 0, 11])) == BAD
        assert call(f, opts=opts(device=1)) == BAD and "device" in _lib.last_error()
        assert call(f, opts=opts(device=0)) == _lib.M2S_OK
        for field, value in (("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4), ("mem_kind", 5)):
            assert call(f, opts=opts(**{field: value})) == BAD, field
        assert L.m2s_band_resample(f._h, C.byref(grid._g), None, None, None, None, None) == BAD
        t = M2STimings()
        with f.resample(grid, mode=SampleMode.Snap, timings=t) as r:
            assert t.n_units == r.count == f.count > 0 and t.seed_ms > 0 and t.distance_ms > 0 and t.total_ms >= t.seed_ms + t.distance_ms
        for bad in (np.diag([1.0, 1.0, 1.01, 1.0]), np.eye(3), np.concatenate([np.eye(3), [[0.0], [0.0], [np.nan]]], 1)):
            with pytest.raises(ValueError):
                f.resample(grid, bad)
        with pytest.raises(M2SError):
            f.resample("grid")
    with _field(grid, cm.Band(shape, band.cells, band.distances, None, FMAX, 0.5), True) as f:     # a default background that overflows
        assert call(f, ro=ropts(scale=1.6)) == BAD and "backgrounds" in _lib.last_error()
        assert call(f, ro=ropts(scale=1.6), fo=C.byref(_lib.M2SBandFieldOpts(12, 1.0, 0.5))) == _lib.M2S_OK


def test_c_and_cpp_consumers_run_clean(tmp_path):
    for cc, std, src, extra in (("gcc", "-std=c99", "tests/c/band_resample_smoke.c", ["-lm"]),
                                ("g++", "-std=c++17", "tests/cpp/band_resample_tests.cpp", [])):
        exe = str(tmp_path / os.path.basename(src).split(".")[0])
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                               os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                               "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", *extra, "-o", exe])
        r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
