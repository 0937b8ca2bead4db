"""m2s_band_advect on the GPU, bit for bit against tests/band_advect_model.py (the definition in numpy): the random cases of
tests/band_advect_cases.py (bands on the smallest grids where the kernels can go wrong, velocities and speeds with zeros, cells at rest,
inf and NaN, 1, 2, 3 and 5 steps: the test a step that is not Jacobi fails), from device tensors and host arrays alternately; the chain
band of a sphere -> flow -> isosurface and two rounds of morph against the chained models; and what the call rejects.  Every comparison
with the model is exact equality of bits, plus the info."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import band_advect_cases as ac
import band_advect_model as am
import band_csg_model as cm
import band_isosurface_model as bim
import band_query_model as bqm
import band_redistance_model as rm
import grid_query_model as gqm
import isosurface_model as im
from mesh_to_sdf_amd import AdvectInfo, BandField, FlowInfo, Grid, M2SError, M2STimings, _lib

F = np.float32
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {am.VELOCITY: "velocity", am.NORMAL: "speed"}
HZ = rm.CELLS[2]


def _np(x):
    if hasattr(x, "cpu"):
        if x.dtype == getattr(torch, "uint32", None):
            x = x.view(torch.int32)
        x = x.cpu().numpy()
    return np.asarray(x)


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


def _same_float(a, b):
    return F(a).view(np.uint32) == F(b).view(np.uint32)


def _check(field, want, info, what):
    """An advected handle against the model's (Band, Info): the export's three arrays, the backgrounds, every info field, m2s_band_info."""
    got = _band(field)
    assert got.cells.size == want.cells.size == field.count, f"{what}: {got.cells.size} cells, the model has {want.cells.size}"
    assert np.array_equal(got.cells, want.cells), f"{what}: cells differ"
    differ = got.distances.view(np.uint32) != want.distances.view(np.uint32)
    assert not differ.any(), f"{what}: {int(differ.sum())} distances differ, first at cell {want.cells[np.flatnonzero(differ)[0]]}"
    assert cm.same(got, want), f"{what}: sign mask or backgrounds differ"
    ai = field.advect_info
    assert isinstance(ai, AdvectInfo)
    assert (ai.steps, ai.n_moving, ai.n_changed, ai.n_sign_flips, ai.n_nonfinite) == \
        (info.steps, info.n_moving, info.n_changed, info.n_sign_flips, info.n_nonfinite), f"{what}: info {ai}, the model has {info}"
    assert _same_float(ai.max_change, info.max_change), f"{what}: max_change {ai.max_change}, the model has {info.max_change}"
    assert _same_float(ai.max_cfl, info.max_cfl), f"{what}: max_cfl {ai.max_cfl}, the model has {info.max_cfl}"
    n, nbytes = C.c_uint64(0), C.c_uint64(0)
    assert _lib.lib().m2s_band_info(field._h, None, C.byref(n), C.byref(nbytes)) == _lib.M2S_OK
    words = (want.total + 63) // 64
    assert n.value == want.cells.size and nbytes.value == 24 * words + 4 * n.value == field.device_bytes, what


# ---- 1. the random cases -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ac.SHAPES, ids=lambda n: "x".join(map(str, n)))
def test_random_cases(shape):
    grid = Grid(list(ac.FIRST), list(ac.CELL), list(shape))
    fields = {}
    try:
        for at, case in enumerate(ac.cases(shape)):
            device = at % 2 == 0
            key = (id(case.band), device)
            if key not in fields:
                fields[key] = _field(grid, case.band, device)
            f = fields[key]
            want, info = am.band_advect(case.band, ac.CELL, case.kind, case.field, case.dt, case.steps, case.background)
            given = torch.as_tensor(case.field, device=DEV) if (at // 2) % 2 == 0 else case.field        # the field's side, whatever the band's
            bg = None if case.background is None else (case.background[1], case.background[0])
            with f.advect(case.dt, case.steps, background=bg, **{KINDS[case.kind]: given}) as r:
                _check(r, want, info, f"{shape} {case.name}, background {case.background}, band on the {'device' if device else 'host'}")
    finally:
        for f in fields.values():
            f.close()


def test_a_scalar_and_a_vector_are_broadcast_and_centers_are_the_cell_centres():
    shape = (7, 9, 11)
    band = ac.smooth_band(np.random.default_rng(4), shape)
    grid = Grid(list(ac.FIRST), list(ac.CELL), list(shape))
    n = band.cells.size
    for device in (True, False):
        with _field(grid, band, device) as f:
            c = f.centers()
            assert _is_device(c) == device and gqm.same_bits(_np(c), am.centers(band, ac.FIRST, ac.CELL))
            want, info = am.band_advect(band, ac.CELL, am.VELOCITY, np.tile(F([0.5, -0.25, 0.0]), (n, 1)), 0.03, 2)
            with f.advect(0.03, 2, velocity=(0.5, -0.25, 0.0)) as r:
                _check(r, want, info, "a 3-vector")
            want, info = am.band_advect(band, ac.CELL, am.NORMAL, np.full(n, -0.75, F), 0.03, 3)
            with f.advect(0.03, 3, speed=-0.75) as r:
                _check(r, want, info, "a scalar")
            for bad in (dict(), dict(velocity=(1, 0, 0), speed=1.0), dict(speed=np.zeros(n + 1, F)), dict(velocity=np.zeros((n, 2), F))):
                with pytest.raises(M2SError):
                    f.advect(0.03, **bad)


def _is_device(x):
    return hasattr(x, "is_cuda") and x.is_cuda


# ---- 2. the chains: flow -> isosurface, and morph, against the chained models -------------------------------------------------------------------
GRID = Grid(list(rm.FIRST), list(rm.CELLS), list(rm.SHAPE))
W3 = F(3 * HZ)


def test_a_sphere_carried_by_a_flow_and_meshed():
    src = rm.band_of(rm.sphere((0.0, 0.0, 0.0), 0.5), 3 * HZ)
    u = F([0.75, -0.5, 0.25])
    time = 2 * float(F(min(rm.CELLS))) / float(np.sqrt((u.astype(np.float64) ** 2).sum()))  # two rounds of one smallest cell edge each
    want, rounds, steps, opens = am.flow(src, rm.FIRST, rm.CELLS, time, W3, am.VELOCITY, lambda c: np.tile(u, (c.shape[0], 1)))
    assert rounds == 2 and opens == [0, 0]
    g = im.GridI.of(GRID)
    wv, wt, wopen = bim.extract(g, want.cells.astype(np.uint64), want.distances, 0.0)
    for device in (True, False):
        with _field(GRID, src, device) as f, f.flow(time, float(W3), velocity=tuple(float(v) for v in u)) as r:
            assert isinstance(r.flow_info, FlowInfo) and (r.flow_info.rounds, r.flow_info.steps) == (rounds, steps)
            assert abs(r.flow_info.time - time) <= 1e-5 * time and r.redistance_info.n_open == 0 and r.advect_info.max_cfl <= 0.5
            assert cm.same(_band(r), want), "the chain's lists differ from the model chain's"
            v, t, n_open = r.isosurface(0.0)
            assert n_open == wopen == 0 and wv.shape[0] > 1000
            assert gqm.same_bits(_np(v), wv) and np.array_equal(_np(t).astype(np.int64), wt.astype(np.int64))
    # the zero set moved with the flow: the mesh's centre is the displacement to a tenth of a cell
    assert np.abs(wv.astype(np.float64).mean(0) - u.astype(np.float64) * time).max() < 0.1 * min(rm.CELLS)


def test_a_small_sphere_morphs_towards_a_larger_one():
    src = rm.band_of(rm.sphere((0.0, 0.0, 0.0), 0.4), 3 * HZ)
    target = rm.band_of(rm.sphere((0.05, 0.0, 0.0), 0.6), 5 * HZ)
    q = gqm.GridQ.of(GRID)
    tb = bqm.Band(rm.SHAPE, target.cells, target.distances, target.bg_out, target.bg_in, target.bits)

    def speed(centers):                                           # -target.sample(centers, Trilinear), as the query model samples
        return (-bqm.sample(q, tb, centers, gqm.TRILINEAR)[0]).astype(F)
    first = float(np.abs(speed(am.centers(src, rm.FIRST, rm.CELLS))).max())
    time = 1.6 * float(F(min(rm.CELLS))) / first                            # a full round, then what is left: two rounds
    want, rounds, steps, opens = am.flow(src, rm.FIRST, rm.CELLS, time, W3, am.NORMAL, speed)
    assert rounds == 2 and opens == [0, 0]
    with _field(GRID, src, True) as f, _field(GRID, target, True) as ft, f.morph(ft, time, float(W3)) as r:
        assert (r.flow_info.rounds, r.flow_info.steps) == (rounds, steps) and r.redistance_info.n_open == 0
        assert cm.same(_band(r), want), "the morph's lists differ from the model chain's"
    # the surface grew towards the target: more of the grid is inside than before
    assert cm.dense(want)[2].sum() > cm.dense(src)[2].sum()


# ---- 3. what the call rejects of a real handle -------------------------------------------------------------------------------------------------
def test_the_call_rejects_bad_options_and_reports_timings():
    shape = (7, 9, 11)
    rng = np.random.default_rng(15)
    band = ac.smooth_band(rng, shape)
    n = band.cells.size
    L = _lib.lib()
    BAD = _lib.ERR_BAD_ARG
    u = torch.as_tensor(ac.random_field(rng, n, am.VELOCITY), device=DEV)
    grid = Grid(list(ac.FIRST), list(ac.CELL), list(shape))

    def call(f, ao=(20, 0, 1, 0, 0.01), field=u, fo=None, opts=None, info=None):
        h = C.c_void_p(0x1234)
        o = opts if opts is not None else options()
        rc = L.m2s_band_advect(f._h, field.data_ptr() if field is not None else None, C.byref(_lib.M2SBandAdvectOpts(*ao)) if ao else None, fo, o,
                               C.byref(h), info)
        assert (rc == _lib.M2S_OK) == (h.value is not None)                # *out = NULL on every failure
        if h.value is not None:
            L.m2s_band_destroy(h)
        return rc

    def options(**kw):
        o = _lib.M2SOpts()
        o.struct_size, o.device, o.mem_kind = C.sizeof(o), -1, _lib.MEM_DEVICE
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)

    with _field(grid, band, True) as f, _field(grid, cm.Band(shape, [], [], None, 0.5, 0.5), True) as empty:
        assert call(f) == _lib.M2S_OK and call(f, ao=(20, 1, 3, 0, 0.01)) == _lib.M2S_OK
        assert call(f, ao=None) == BAD and "NULL" in _lib.last_error()
        assert call(f, field=None) == BAD and "field is NULL" in _lib.last_error()
        for ao in ((16, 0, 1, 0, 0.01), (24, 0, 1, 0, 0.01), (20, 2, 1, 0, 0.01), (20, -1, 1, 0, 0.01), (20, 0, 0, 0, 0.01), (20, 0, 65537, 0, 0.01),
                   (20, 0, 1, 1, 0.01), (20, 0, 1, 0, 0.0), (20, 0, 1, 0, -0.01), (20, 0, 1, 0, float("inf")), (20, 0, 1, 0, float("nan"))):
            assert call(f, ao=ao) == BAD, ao
        for size, out, ins in ((8, 0.5, 0.5), (12, -0.5, 0.5), (12, 0.5, float("inf")), (12, float("nan"), 0.5)):
            assert call(f, fo=C.byref(_lib.M2SBandFieldOpts(size, out, ins))) == BAD
        assert call(f, info=C.byref(_lib.M2SBandAdvectInfo(40))) == BAD
        assert call(f, opts=options(device=1)) == BAD and "device" in _lib.last_error()
        assert call(f, opts=options(device=0)) == _lib.M2S_OK
        for field, value in (("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4), ("mem_kind", 5)):
            assert call(f, opts=options(**{field: value})) == BAD, field
        assert L.m2s_band_advect(f._h, u.data_ptr(), C.byref(_lib.M2SBandAdvectOpts(20, 0, 1, 0, 0.01)), None, options(), None, None) == BAD
        # an empty band takes a NULL field
        info = _lib.M2SBandAdvectInfo(48)
        assert call(empty, field=None, info=C.byref(info)) == _lib.M2S_OK
        assert (info.steps, info.n_moving, info.n_changed, info.max_cfl, info.max_change) == (1, 0, 0, 0.0, 0.0)
        with empty.advect(0.01, 2, speed=1.0) as r:
            assert r.count == 0 and r.advect_info.steps == 2
        t = M2STimings()
        with f.advect(0.01, 4, velocity=u, timings=t) as r:
            assert t.n_units == r.count == f.count > 0 and t.seed_ms > 0 and t.distance_ms > 0 and t.total_ms >= t.seed_ms + t.distance_ms
            assert r.advect_info.steps == 4 and r.background == f.background
        for bad in (dict(dt=0.01, steps=0, speed=1.0), dict(dt=0.0, speed=1.0), dict(dt=float("nan"), velocity=u)):
            with pytest.raises(M2SError):
                f.advect(**bad)


def test_c_and_cpp_consumers_run_clean(tmp_path):
    for cc, std, src, extra in (("gcc", "-std=c99", "tests/c/band_advect_smoke.c", ["-lm"]),
                                ("g++", "-std=c++17", "tests/cpp/band_advect_tests.cpp", [])):
        exe = str(tmp_path / os.path.basename(src).split(".")[0])
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                               os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                               "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", *extra, "-o", exe])
        r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
