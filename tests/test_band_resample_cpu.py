"""m2s_band_resample without a GPU: the export and the header, every argument check that can be reached without a handle, the consumers,
the transform wrapper of BandField.resample, the model tests/band_resample_model.py against the consequences include/m2s.h states (SNAP
with the identity gives the band back on any grid; a whole-cell shift is crop and pad; a 90 degree turn is a transposed array), and the
accuracy of the definition itself: a sphere turned, scaled and moved onto another grid against the analytic sphere.

The accuracy figures are those of the committed model, measured once and asserted at 1.25 x: nothing is random, so the margin covers
numpy and libm differences only.  DESIGN.md 4.20 records them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import band_csg_model as cm
import band_redistance_model as rm
import band_resample_model as rsm
from mesh_to_sdf_amd import BandField, ResampleInfo, SampleMode, _lib
from mesh_to_sdf_amd.api import _similarity

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMAX = np.finfo(F).max
SPECIAL = np.array([0.0, -0.0, 0.5, -0.5, 0.75, -0.75, 2.0, -2.0, FMAX, -FMAX], F)
HZ = rm.CELLS[2]
TARGET = rsm.GridSpec(rm.FIRST, rm.CELLS, rm.SHAPE)
# the largest |r - (|p - t| - 0.45)| over the result's cells, in cells of 0.0625, measured with this model: the sphere of radius 0.6 on
# (source shape, source cell) under rsm.move(), onto band_redistance_model's grid -> (SNAP, TRILINEAR, TETRAHEDRAL)
ACCURACY = {((60, 56, 54), (0.03, 0.032, 0.034)): (0.3108, 0.0075, 0.0101),
            ((30, 28, 27), (0.06, 0.064, 0.068)): (0.6141, 0.0280, 0.0369),
            ((20, 19, 18), (0.09, 0.096, 0.102)): (0.9128, 0.0644, 0.0877)}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


# ---- 1. export, header, argument checks, consumers -------------------------------------------------------------------------------------------
def test_the_entry_point_is_exported_and_declared(lib):
    assert "m2s_band_resample" in _lib.EXPORTS and hasattr(lib, "m2s_band_resample")
    hdr = " ".join(open(os.path.join(ROOT, "include", "m2s.h")).read().split())
    for text in ("typedef struct m2s_band_resample_opts { uint32_t struct_size; int32_t mode; float to_source[12]; float value_scale; } "
                 "m2s_band_resample_opts;",
                 "typedef struct m2s_band_resample_info { uint32_t struct_size, reserved; uint64_t n_cells, n_partial, n_nonfinite, n_open; } "
                 "m2s_band_resample_info;",
                 "int m2s_band_resample(const m2s_band* band, const m2s_grid* target, const m2s_band_resample_opts* ropts "
                 "/* NULL = identity, TRILINEAR, 1 */, const m2s_band_field_opts* fopts /* NULL = the input's backgrounds times value_scale */, "
                 "const m2s_opts* opts, m2s_band** out, m2s_band_resample_info* info_out /* may be NULL */);",
                 "q_a = ((m[4a] * p.x + m[4a+1] * p.y) + m[4a+2] * p.z) + m[4a+3]", "r = v * value_scale",
                 "active[L] = (support == K) && isfinite(r)", "s[L] = active ? (r < 0) : sX[c]", "a zero background is legal and has no sign",
                 "GridTransformer / resampleToMatch", "the SNAP index has half a cell of slack", "is crop and pad",
                 "follow it with m2s_band_redistance", "A map that is not a similarity is accepted", "constant extrapolation",
                 "aliases, as OpenVDB's point samplers do", "Nothing sized 4 bytes per point of either grid is allocated"):
        assert text in hdr, text
    assert lib.m2s_version() == 5
    assert C.sizeof(_lib.M2SBandResampleOpts) == 60 and C.sizeof(_lib.M2SBandResampleInfo) == 40
    assert hasattr(BandField, "resample")
    assert ResampleInfo._fields == ("n_cells", "n_partial", "n_nonfinite", "n_open")
    hpp = open(os.path.join(ROOT, "include", "mesh_to_sdf.hpp")).read()
    for text in ("struct ResampleInfo", "BandField resample(const Grid<V>& target, const float* to_source = nullptr, float value_scale = 1.0f, "
                 "SampleMode mode = SampleMode::Trilinear, ResampleInfo* info = nullptr) const"):
        assert text in hpp, text
    for doc, text in (("README.md", "m2s_band_resample"), ("README.md", "resampleToMatch"), ("DESIGN.md", "m2s_band_resample"), ("DESIGN.md", "4.20")):
        assert text in open(os.path.join(ROOT, doc)).read(), (doc, text)


def _grid(first=(-0.5, 0.25, 0.0), cell=(0.125, 0.25, 0.1875), count=(5, 6, 7)):
    g = _lib.M2SGrid()
    for a in range(3):
        g.first_cell[a], g.cell_size[a], g.cell_count[a] = first[a], cell[a], count[a]
    return g


def _ropts(size=60, mode=1, m=rsm.IDENTITY, scale=1.0):
    ro = _lib.M2SBandResampleOpts()
    ro.struct_size, ro.mode, ro.value_scale = size, mode, scale
    ro.to_source[:] = [float(v) for v in m]
    return ro


def test_the_call_rejects_what_needs_no_handle(lib):
    BAD = _lib.ERR_BAD_ARG
    SENTINEL = 0x1234
    fake = C.c_void_p(SENTINEL)                   # never dereferenced: every call below fails before it looks at the handle
    good_grid = _grid()

    def call(band=fake, grid=good_grid, ro=None, fo=None, opts=None, info=None):
        h = C.c_void_p(SENTINEL)
        rc = lib.m2s_band_resample(band, C.byref(grid) if grid is not None else None, C.byref(ro) if ro is not None else None, fo, opts, C.byref(h), info)
        assert h.value is None                    # *out = NULL on every failure
        return rc

    assert call(band=None) == BAD and "band is NULL" in _lib.last_error()
    assert call(grid=None) == BAD and "target is NULL" in _lib.last_error()
    assert lib.m2s_band_resample(fake, C.byref(good_grid), None, None, None, None, None) == BAD and "out is NULL" in _lib.last_error()
    for size in (0, 56, 64):
        assert call(ro=_ropts(size=size)) == BAD and "struct_size" in _lib.last_error(), size
    for mode in (-1, 3, 7):
        assert call(ro=_ropts(mode=mode)) == BAD and "mode" in _lib.last_error(), mode
    for at in (0, 3, 6, 11):
        for bad in (float("nan"), float("inf"), -float("inf")):
            m = list(rsm.IDENTITY)
            m[at] = bad
            assert call(ro=_ropts(m=m)) == BAD and "to_source" in _lib.last_error(), (at, bad)
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        assert call(ro=_ropts(scale=scale)) == BAD and "value_scale" in _lib.last_error(), scale
    for fo in ((8, 0.5, 0.5), (12, -0.5, 0.5), (12, 0.5, float("inf")), (12, float("nan"), 0.5)):
        assert call(fo=C.byref(_lib.M2SBandFieldOpts(*fo))) == BAD, fo
    assert call(info=C.byref(_lib.M2SBandResampleInfo(8))) == BAD and "m2s_band_resample_info" in _lib.last_error()
    for field, value in (("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4), ("mem_kind", 5)):
        o = _lib.M2SOpts()
        o.struct_size, o.device = C.sizeof(o), -1
        setattr(o, field, value)
        assert call(opts=C.byref(o)) == BAD, field
    # what m2s_band_create rejects of a grid
    for kw in (dict(count=(0, 6, 7)), dict(count=(5, 6, 2 ** 63)), dict(cell=(0.0, 0.25, 0.1875)), dict(cell=(0.125, -0.25, 0.1875)),
               dict(cell=(0.125, 0.25, float("nan"))), dict(cell=(float("inf"), 0.25, 0.1875)), dict(first=(float("nan"), 0.25, 0.0)),
               dict(first=(0.0, float("inf"), 0.0)), dict(first=(3e38, 0.0, 0.0), cell=(3e38, 1.0, 1.0)),
               dict(count=(4096, 4096, 4096)), dict(count=(2 ** 32, 2 ** 32, 1)), dict(count=(1, 2 ** 20, 2 ** 16))):
        assert call(grid=_grid(**kw)) == BAD, kw


@pytest.mark.parametrize("cc,std,src", [("gcc", "-std=c99", "tests/c/band_resample_smoke.c"), ("g++", "-std=c++17", "tests/cpp/band_resample_tests.cpp")])
def test_consumers_compile_and_check_their_arguments(lib, tmp_path, cc, std, src):
    exe = str(tmp_path / os.path.basename(src).split(".")[0])
    subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                           os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


# ---- 2. the transform wrapper ----------------------------------------------------------------------------------------------------------------
def test_the_wrapper_takes_similarities_only():
    R = rsm.rotation((1, 2, 3), 0.7)
    fwd = rsm.forward(0.75, R, (0.3, 0.05, 0.0))
    for M in (fwd, np.concatenate([fwd, [[0, 0, 0, 1]]], 0)):
        to_source, scale = _similarity(M)
        assert to_source.dtype == F and to_source.shape == (12,) and scale == F(0.75)
        inv = np.linalg.inv(np.concatenate([fwd, [[0, 0, 0, 1]]], 0))[:3]                    # a float64 inverse
        assert np.abs(to_source.reshape(3, 4) - inv).max() <= 2.0 ** -23 * np.abs(inv).max()  # rounded to binary32, nothing else
        q = np.random.default_rng(2).uniform(-1, 1, (50, 3))
        back = (to_source.reshape(3, 4)[:, :3].astype(np.float64) @ (q @ fwd[:, :3].T + fwd[:, 3]).T).T + to_source.reshape(3, 4)[:, 3]
        assert np.abs(back - q).max() < 1e-6
        model_m, model_s = rsm.similarity(M)
        assert np.array_equal(model_m.view(np.uint32), to_source.view(np.uint32)) and model_s == scale
    mirror = rsm.forward(2.0, np.diag([1.0, -1.0, 1.0]), (0, 0, 1))                          # a reflection passes
    to_source, scale = _similarity(mirror)
    assert scale == F(2.0) and np.array_equal(to_source.reshape(3, 4)[:, :3], np.diag([0.5, -0.5, 0.5]).astype(F))
    shear = np.concatenate([np.array([[1, 0.01, 0], [0, 1, 0], [0, 0, 1.0]]), np.zeros((3, 1))], 1)
    stretch = np.concatenate([np.diag([1.0, 1.0, 1.01]), np.zeros((3, 1))], 1)
    projective = np.concatenate([fwd, [[0, 0, 0.1, 1]]], 0)
    for bad in (shear, stretch, projective, np.zeros((3, 4)), np.eye(3), np.full((3, 4), np.nan)):
        with pytest.raises(ValueError):
            _similarity(bad)
        if bad.shape in ((3, 4), (4, 4)):
            with pytest.raises(ValueError):
                rsm.similarity(bad)
    assert [int(m) for m in (SampleMode.Snap, SampleMode.Trilinear, SampleMode.Tetrahedral)] == list(rsm.MODES)


# ---- 3. the model against the consequences the header states -------------------------------------------------------------------------------
def random_band(rng, shape, density=0.5, bits=True, bg=(0.75, 0.5), special=0.3):
    total = shape[0] * shape[1] * shape[2]
    cells = np.flatnonzero(rng.random(total) < density)
    d = rng.uniform(-1, 1, cells.size).astype(F)
    pick = rng.random(cells.size) < special
    d[pick] = rng.choice(SPECIAL, int(pick.sum()))
    mask = rng.integers(0, 2 ** 32, (shape[0], shape[1], (shape[2] + 31) // 32), dtype=np.uint64).astype(np.uint32) if bits else None
    return cm.Band(shape, cells, d, mask, *bg)


GRIDS = [((-0.5, 0.25, 0.0), (0.125, 0.25, 0.1875)), (tuple(rm.FIRST), (0.05, 0.04, 0.0625)), ((1000.3, -77.7, 0.003), (0.1, 0.3, 0.7))]


@pytest.mark.parametrize("first,cell", GRIDS, ids=["dyadic", "centred", "far"])
def test_snap_with_the_identity_gives_the_band_back(first, cell):
    """Consequence 1, on grids whose centres are not exact in binary32 too: the SNAP index has half a cell of slack."""
    rng = np.random.default_rng(7)
    for shape, bits in (((7, 9, 11), True), ((5, 3, 70), True), ((3, 65, 1), False), ((1, 1, 1), True)):
        g = rsm.GridSpec(first, cell, shape)
        band = random_band(rng, shape, bits=bits)
        out, info = rsm.resample(band, g, g, None, 1.0, rsm.SNAP)
        assert np.array_equal(out.cells, band.cells) and np.array_equal(out.distances.view(np.uint32), band.distances.view(np.uint32))
        assert np.array_equal(cm.unpack_bits(shape, out.bits), cm.dense(band)[2])                   # sX on every point
        assert (out.bg_out, out.bg_in) == (band.bg_out, band.bg_in)
        assert info.n_cells == band.cells.size and info.n_partial == 0 and info.n_nonfinite == 0
        assert info.n_open == rm.frozen_set(*cm.dense(band)[::2])[1]
        if shape == (7, 9, 11):                                                                     # TRILINEAR has no such property
            tri, tinfo = rsm.resample(band, g, g, None, 1.0, rsm.TRILINEAR)
            assert tinfo.n_cells < band.cells.size and tinfo.n_partial > 0


def test_a_whole_cell_shift_is_crop_and_pad():
    """Consequence 2 against plain index arithmetic, on a dyadic grid where every centre is exact: target index t reads source index
    u = t + shift; u in [0, n) is that cell, u == n is the centre that falls on `end` and repeats cell n - 1, everything else is off the box."""
    rng = np.random.default_rng(9)
    first, cell, shape = GRIDS[0][0], GRIDS[0][1], (7, 9, 11)
    src = rsm.GridSpec(first, cell, shape)
    band = random_band(rng, shape)
    act, x, s = cm.dense(band)
    for shift, tshape in (((2, -1, 3), (7, 9, 11)), ((-3, -2, -5), (13, 13, 21)), ((1, 2, 3), (3, 4, 5)), ((-9, 0, 0), (5, 9, 11))):
        tgt = rsm.GridSpec(tuple(first[a] + shift[a] * cell[a] for a in range(3)), cell, tshape)
        out, info = rsm.resample(band, src, tgt, None, 1.0, rsm.SNAP, background=(2.0, 0.125))
        u = [np.arange(tshape[a]) + shift[a] for a in range(3)]
        on = [(u[a] >= 0) & (u[a] <= shape[a]) for a in range(3)]
        c = [np.clip(u[a], 0, shape[a] - 1) for a in range(3)]
        on3 = on[0][:, None, None] & on[1][None, :, None] & on[2][None, None, :]
        ix = np.ix_(*c)
        want_act, want_x, want_s = on3 & act[ix], x[ix], on3 & s[ix]
        assert np.array_equal(out.cells, np.flatnonzero(want_act.reshape(-1))), shift
        assert np.array_equal(out.distances.view(np.uint32), want_x[want_act].view(np.uint32)), shift
        assert np.array_equal(cm.unpack_bits(tshape, out.bits), want_s), shift
        assert (out.bg_out, out.bg_in) == (F(2.0), F(0.125)) and info.n_partial == 0 and info.n_cells == want_act.sum()
    # pad, then crop back: every bit
    pad = rsm.GridSpec(tuple(first[a] - (3, 2, 5)[a] * cell[a] for a in range(3)), cell, (13, 13, 21))
    padded, _ = rsm.resample(band, src, pad, None, 1.0, rsm.SNAP)
    back, _ = rsm.resample(padded, pad, src, None, 1.0, rsm.SNAP)
    assert np.array_equal(back.cells, band.cells) and np.array_equal(back.distances.view(np.uint32), band.distances.view(np.uint32))
    assert np.array_equal(cm.unpack_bits(shape, back.bits), s)


def test_a_quarter_turn_is_a_transposed_array():
    """The cyclic permutation (x, y, z) -> (y, z, x) is a rotation whose matrix holds zeros and ones only, so q is exact."""
    rng = np.random.default_rng(13)
    first, cell, shape = GRIDS[0][0], GRIDS[0][1], (5, 6, 7)
    src = rsm.GridSpec(first, cell, shape)
    perm = (1, 2, 0)                                                                # target axis a is source axis perm[a]
    tgt = rsm.GridSpec(tuple(first[p] for p in perm), tuple(cell[p] for p in perm), tuple(shape[p] for p in perm))
    A = np.zeros((3, 3))
    for a, p in enumerate(perm):
        A[a, p] = 1.0
    to_source, scale = rsm.similarity(rsm.forward(1.0, A, (0, 0, 0)))
    assert scale == 1 and np.array_equal(to_source.reshape(3, 4)[:, :3], A.T.astype(F))
    band = random_band(rng, shape)
    act, x, s = cm.dense(band)
    k16 = F(1.6)
    out, info = rsm.resample(band, src, tgt, to_source, k16, rsm.SNAP)
    with np.errstate(over="ignore"):
        want_r = (x * k16).astype(F).transpose(perm)
    want_act = act.transpose(perm) & np.isfinite(want_r)
    assert np.array_equal(out.cells, np.flatnonzero(want_act.reshape(-1)))
    assert np.array_equal(out.distances.view(np.uint32), want_r[want_act].view(np.uint32))
    assert np.array_equal(cm.unpack_bits(tgt.shape, out.bits), s.transpose(perm))
    assert info.n_nonfinite == (act.transpose(perm) & ~np.isfinite(want_r)).sum() > 0 and info.n_partial == 0
    assert (out.bg_out, out.bg_in) == (band.bg_out * k16, band.bg_in * k16)
    with pytest.raises(ValueError):                                                 # a default background that comes out non-finite
        rsm.resample(cm.Band(shape, [], [], None, FMAX, 0.5), src, tgt, to_source, k16, rsm.SNAP)


def test_off_the_box_and_overflowing_maps_give_an_empty_band():
    rng = np.random.default_rng(17)
    first, cell, shape = GRIDS[0][0], GRIDS[0][1], (7, 9, 11)
    g = rsm.GridSpec(first, cell, shape)
    band = random_band(rng, shape, density=0.9)
    far = list(rsm.IDENTITY)
    far[3] = 1e6
    huge = [3e38] * 12
    for m in (far, huge):
        for mode in rsm.MODES:
            out, info = rsm.resample(band, g, g, m, 1.0, mode)
            assert out.cells.size == 0 and not out.bits.any() and info == (0, 0, 0, 0)


# ---- 4. accuracy of the definition: consequence 3 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,cell", list(ACCURACY), ids=["fine", "coarse", "coarser"])
def test_a_moved_sphere_keeps_its_distances(shape, cell):
    src = rsm.centred(shape, cell)
    band = rm.band_of(rm.sphere((0, 0, 0), 0.6, first=src.first, cells=src.cell, shape=src.shape), 0.2)
    to_source, scale = rsm.similarity(rsm.move())
    assert scale == F(0.75)
    exact = rm.sphere(rsm.MOVE_T, 0.45).reshape(-1)
    for mode, bound in zip(rsm.MODES, ACCURACY[(shape, cell)]):
        out, info = rsm.resample(band, src, TARGET, to_source, scale, mode)
        err = np.abs(out.distances.astype(np.float64) - exact[out.cells]).max() / HZ
        print(f"source {shape}, mode {mode}: {info}, max error {err:.4f} cells of {HZ}")
        assert info.n_cells > 3500 and info.n_nonfinite == 0 and (out.bg_out, out.bg_in) == (F(0.2) * F(0.75), F(0.2) * F(0.75))
        assert err <= 1.25 * bound
        assert (info.n_partial > 1000) == (mode != rsm.SNAP)                         # the rim the interpolation loses; SNAP loses none
        if shape == (60, 56, 54):
            assert info.n_open == 0                                                  # the result brackets its own zero set
        if shape == (20, 19, 18) and mode == rsm.TRILINEAR:
            assert info.n_open > 0                                                   # the target cells outgrew the source band: the diagnostic fires
