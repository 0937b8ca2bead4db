"""m2s_band_filter without a GPU: the export and the header, every argument check that can be reached without a handle, the consumers,
the model tests/band_filter_model.py against its own definition (cells outside the region keep every bit, a linear field is a fixed
point, +-f32::MAX cells are counted and dropped, an empty band), and the accuracy of the definition itself: a sphere shrinking under the
mean-curvature flow and the Laplacian against R^2 = R0^2 - 4 n dt, and the seam of a union filling while the convex parts shrink.

The accuracy figures are those of the committed model, measured once and asserted at 1.25 x: nothing is random, so the margin covers
numpy and libm differences only.  DESIGN.md 4.19 records them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import band_csg_model as cm
import band_filter_model as fm
import band_redistance_model as rm
from mesh_to_sdf_amd import BandField, FilterInfo, FilterKind, _lib

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HX, HZ = rm.CELLS[0], rm.CELLS[2]
FMAX = np.finfo(F).max
# the largest | |p| - sqrt(R0^2 - 4 n dt) | / hx over the zero crossings p along x grid lines, measured with this model:
# (band width in cells of hz, kind, iterations) -> cells of hx.  The mean-curvature flow keeps 0.010 cells; the Laplacian's figure grows
# with the iterations because it also diffuses along the normal, and the crossings that carry it are those of lines that graze the sphere.
SPHERE_DEV = {(3, fm.MEAN_CURVATURE, 1): 0.0098, (3, fm.MEAN_CURVATURE, 4): 0.0099, (3, fm.MEAN_CURVATURE, 8): 0.0100,
              (3, fm.LAPLACIAN, 1): 0.0098, (3, fm.LAPLACIAN, 4): 0.0104, (3, fm.LAPLACIAN, 8): 0.0391,
              (5, fm.MEAN_CURVATURE, 1): 0.0098, (5, fm.MEAN_CURVATURE, 4): 0.0099, (5, fm.MEAN_CURVATURE, 8): 0.0100,
              (5, fm.LAPLACIAN, 1): 0.0098, (5, fm.LAPLACIAN, 4): 0.0103, (5, fm.LAPLACIAN, 8): 0.0426}
# the union of two spheres after 8 iterations of the mean-curvature flow, changes in cells of hz: the most negative one on the seam, and
# the range on the convex parts (|D_A - D_B| > 4 cells) within one cell of the surface
SEAM_FALL = -0.4051
CONVEX_RISE = (0.1750, 0.2522)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


# ---- 1. export, header, argument checks, consumers -------------------------------------------------------------------------------------------
def test_the_entry_point_is_exported_and_declared(lib):
    assert "m2s_band_filter" in _lib.EXPORTS and hasattr(lib, "m2s_band_filter")
    hdr = " ".join(open(os.path.join(ROOT, "include", "m2s.h")).read().split())
    for text in ("enum m2s_filter_kind { M2S_FILTER_MEAN = 0, M2S_FILTER_LAPLACIAN = 1, M2S_FILTER_MEAN_CURVATURE = 2 };",
                 "typedef struct m2s_band_filter_opts { uint32_t struct_size; int32_t kind; uint32_t iterations; uint32_t width; } m2s_band_filter_opts;",
                 "typedef struct m2s_band_filter_info { uint32_t struct_size, passes; float max_change; uint32_t reserved; "
                 "uint64_t n_changed, n_sign_flips, n_nonfinite; } m2s_band_filter_info;",
                 "int m2s_band_filter(const m2s_band* band, const m2s_band* where /* may be NULL = everywhere */, const m2s_band_filter_opts* fl, "
                 "const m2s_band_field_opts* fopts /* NULL = the input's backgrounds */, const m2s_opts* opts, "
                 "m2s_band** out, m2s_band_filter_info* info_out /* may be NULL */);",
                 "IT MUST BE JACOBI.  Every pass reads the previous pass's values only".replace("  ", " "),
                 "cand = ((N(-a) + c) + N(+a)) / 3", "cand = g2 > 0 ? c + dt * (num / g2) : c", "approximate OpenVDB's Gaussian",
                 "follow it with m2s_band_redistance", "Nothing sized 4 bytes per grid point is allocated"):
        assert text in hdr, text
    assert lib.m2s_version() == 5
    assert C.sizeof(_lib.M2SBandFilterOpts) == 16 and C.sizeof(_lib.M2SBandFilterInfo) == 40
    for name in ("filter", "smooth"):
        assert hasattr(BandField, name), name
    assert FilterInfo._fields == ("passes", "max_change", "n_changed", "n_sign_flips", "n_nonfinite")
    assert (int(FilterKind.Mean), int(FilterKind.Laplacian), int(FilterKind.MeanCurvature)) == (fm.MEAN, fm.LAPLACIAN, fm.MEAN_CURVATURE)
    hpp = open(os.path.join(ROOT, "include", "mesh_to_sdf.hpp")).read()
    for text in ("struct FilterInfo", "enum class FilterKind",
                 "BandField filter(FilterKind kind, uint32_t iterations = 1, const BandField* where = nullptr, FilterInfo* info = nullptr) const"):
        assert text in hpp, text
    for doc, text in (("README.md", "m2s_band_filter"), ("DESIGN.md", "4.19")):
        assert text in open(os.path.join(ROOT, doc)).read(), doc


def test_the_call_rejects_what_needs_no_handle(lib):
    BAD = _lib.ERR_BAD_ARG
    SENTINEL = 0x1234
    fake = C.c_void_p(SENTINEL)                   # never dereferenced: every call below fails before it looks at the handle
    good = _lib.M2SBandFilterOpts(16, fm.LAPLACIAN, 1, 1)

    def call(band=fake, fl=good, fo=None, opts=None, info=None):
        h = C.c_void_p(SENTINEL)
        rc = lib.m2s_band_filter(band, None, C.byref(fl) if fl is not None else None, fo, opts, C.byref(h), info)
        assert h.value is None                    # *out = NULL on every failure
        return rc

    assert call(band=None) == BAD and "band is NULL" in _lib.last_error()
    assert lib.m2s_band_filter(fake, None, C.byref(good), None, None, None, None) == BAD and "out is NULL" in _lib.last_error()
    assert call(fl=None) == BAD and "NULL" in _lib.last_error()
    for fl in ((12, 1, 1, 1), (0, 1, 1, 1), (20, 1, 1, 1),                       # struct_size
               (16, 3, 1, 1), (16, -1, 1, 1),                                    # kind
               (16, 1, 0, 1), (16, 1, 65537, 1), (16, 1, 2 ** 32 - 1, 1),        # iterations
               (16, 1, 1, 0), (16, 1, 1, 2), (16, 0, 1, 3)):                     # width
        assert call(fl=_lib.M2SBandFilterOpts(*fl)) == BAD, fl
    for fo in ((8, 0.5, 0.5), (12, -0.5, 0.5), (12, 0.5, float("inf")), (12, float("nan"), 0.5)):
        assert call(fo=C.byref(_lib.M2SBandFieldOpts(*fo))) == BAD, fo
    assert call(info=C.byref(_lib.M2SBandFilterInfo(8))) == BAD and "m2s_band_filter_info" in _lib.last_error()
    for field, value in (("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4), ("mem_kind", 5)):
        o = _lib.M2SOpts()
        o.struct_size, o.device = C.sizeof(o), -1
        setattr(o, field, value)
        assert call(opts=C.byref(o)) == BAD, field


@pytest.mark.parametrize("cc,std,src", [("gcc", "-std=c99", "tests/c/band_filter_smoke.c"), ("g++", "-std=c++17", "tests/cpp/band_filter_tests.cpp")])
def test_consumers_compile_and_check_their_arguments(lib, tmp_path, cc, std, src):
    exe = str(tmp_path / os.path.basename(src).split(".")[0])
    subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                           os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


# ---- 2. the model against itself -----------------------------------------------------------------------------------------------------------------
CELL = (0.125, 0.25, 0.1875)


def smooth_band(rng, shape, bits=True, keep=0.9):
    """The band of a random low-order trigonometric field."""
    i, j, k = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    a = rng.uniform(0.2, 0.9, 3)
    d = (np.sin(a[0] * i + rng.uniform(0, 6)) + np.sin(a[1] * j + rng.uniform(0, 6)) + np.sin(a[2] * k + rng.uniform(0, 6))).astype(F) * F(0.2)
    d = d.reshape(-1)
    cells = np.flatnonzero((np.abs(d) <= 0.3) & (rng.random(d.size) < keep))
    return cm.Band(shape, cells, d[cells], cm.pack_bits(shape, (d < 0).reshape(shape)) if bits else None, 0.75, 0.5)


@pytest.mark.parametrize("kind", fm.KINDS)
def test_cells_outside_the_region_keep_every_bit(kind):
    shape = (9, 10, 11)
    rng = np.random.default_rng(5 + kind)
    band, where = smooth_band(rng, shape), smooth_band(rng, shape)
    region = cm.dense(where)[2].reshape(-1)[band.cells]
    assert 0 < region.sum() < region.size
    everywhere, info_all = fm.band_filter(band, CELL, kind, 3)
    r, info = fm.band_filter(band, CELL, kind, 3, where=where)
    same = r.distances.view(np.uint32) == band.distances.view(np.uint32)
    assert same[~region].all() and not same[region].all()
    assert info.passes == info_all.passes == (9 if kind == fm.MEAN else 3) and 0 < info.n_changed <= region.sum() < info_all.n_changed
    assert np.array_equal(r.cells, band.cells) and (r.bg_out, r.bg_in) == (band.bg_out, band.bg_in)
    act, v, s = cm.dense(r)
    assert np.array_equal(cm.unpack_bits(shape, r.bits), np.where(act, v < 0, cm.dense(band)[2]))    # the sign mask on every point
    # the band as its own region: its negative cells alone move
    r, info = fm.band_filter(band, CELL, kind, 1, where=band, background=(2.0, 0.125))
    assert (r.distances.view(np.uint32) == band.distances.view(np.uint32))[band.distances >= 0].all() and info.n_changed > 0
    assert (r.bg_out, r.bg_in) == (F(2.0), F(0.125))


@pytest.mark.parametrize("kind", fm.KINDS)
def test_a_linear_field_is_a_fixed_point(kind):
    """a i + b j + c k with values and spacings that are exact in binary32: every difference of the stencils is exact and cancels, so
    away from the faces (clamped reads) and the rim (reads of the backgrounds) no bit changes, whatever the number of passes reaches."""
    shape = (20, 19, 21)
    cell = (0.5, 0.25, 0.125)
    i, j, k = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    d = (F(0.25) * i.astype(F) - F(0.5) * j.astype(F) + F(0.125) * k.astype(F) + F(0.0625)).astype(F)
    assert not (d == 0).any()
    keep = np.ones(shape, bool)
    keep[2:4, 2:4, 2:4] = False                                                  # a hole: a rim inside the grid
    cells = np.flatnonzero(keep.reshape(-1))
    band = cm.Band(shape, cells, d.reshape(-1)[cells], None, 0.75, 0.5)
    source = ~keep                                                               # where a stencil is not the linear field's: the hole, the faces
    for a in range(3):
        for e in (0, -1):
            edge = [slice(None)] * 3
            edge[a] = e
            source[tuple(edge)] = True
    for iterations in (1, 2):
        reach = iterations * (3 if kind == fm.MEAN else 1)                       # a changed value travels one cell per pass, diagonals included
        r, info = fm.band_filter(band, cell, kind, iterations)
        calm = ~rm.box_dilate(source, (reach, reach, reach)).reshape(-1)[cells]
        assert calm.sum() > 100
        same = r.distances.view(np.uint32) == band.distances.view(np.uint32)
        assert same[calm].all() and info.n_nonfinite == 0
        if kind != fm.MEAN_CURVATURE:                                            # a plane has no curvature at a clamped face either
            assert not same.all()


@pytest.mark.parametrize("kind", fm.KINDS)
def test_the_largest_floats_are_counted_and_dropped(kind):
    shape = (6, 5, 7)
    rng = np.random.default_rng(11)
    total = shape[0] * shape[1] * shape[2]
    d = rng.uniform(-1, 1, total).astype(F)
    d[rng.random(total) < 0.3] = FMAX
    d[rng.random(total) < 0.3] = -FMAX
    band = cm.Band(shape, np.arange(total), d, None, 0.75, 0.5)
    r, info = fm.band_filter(band, CELL, kind, 2)
    assert info.n_nonfinite > 0 and np.isfinite(r.distances).all() and info.n_changed > 0
    assert info.max_change == F(np.inf) or np.isfinite(info.max_change)


def test_an_empty_band_and_a_band_without_a_sign_mask():
    shape = (5, 6, 7)
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2 ** 32, (5, 6, 1), dtype=np.uint64).astype(np.uint32)
    for kind in fm.KINDS:
        r, info = fm.band_filter(cm.Band(shape, [], [], bits, 0.5, 0.25), CELL, kind, 2)
        assert r.cells.size == 0 and info == (6 if kind == fm.MEAN else 2, 0, 0, 0, 0) and (r.bg_out, r.bg_in) == (F(0.5), F(0.25))
        assert np.array_equal(r.bits, cm.pack_bits(shape, cm.unpack_bits(shape, bits)))                  # the sign mask, the bits at k >= nz zero
        r, info = fm.band_filter(cm.Band(shape, [], [], None, 0.5, 0.5), CELL, kind, 1)
        assert r.cells.size == 0 and r.bits is not None and not r.bits.any()                             # a result always has a mask
    # a lone cell reads the outside background on every side: the Laplacian pulls it towards it
    r, info = fm.band_filter(cm.Band(shape, [100], [-0.1], None, 0.5, 0.5), CELL, fm.LAPLACIAN, 1)
    k = fm.constants(CELL)
    t = [((F(0.5) - F(-0.1)) + (F(0.5) - F(-0.1))) * k.w[a] for a in range(3)]
    assert r.distances[0] == F(-0.1) + k.dt * ((t[0] + t[1]) + t[2]) and info.n_sign_flips == 1 and info.n_changed == 1
    assert not cm.unpack_bits(shape, r.bits).any()


def test_the_passes_are_jacobi_and_the_mean_is_three_of_them():
    """One iteration of the mean is the i, j and k passes in this order, each from the values of the pass before it."""
    shape = (7, 9, 11)
    band = smooth_band(np.random.default_rng(8), shape)
    r, info = fm.band_filter(band, CELL, fm.MEAN, 1)
    act, x, s = cm.dense(band)
    v = x
    k = fm.constants(CELL)
    for axis in range(3):
        cand = fm.candidate(v, fm.MEAN, axis, k)
        v = np.where(act, cand, v)
    assert info.passes == 3 and np.array_equal(v.reshape(-1)[band.cells].view(np.uint32), r.distances.view(np.uint32))


# ---- 3. accuracy of the definition on a sphere ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [fm.MEAN_CURVATURE, fm.LAPLACIAN])
@pytest.mark.parametrize("width", [3, 5])
def test_a_sphere_shrinks_as_the_flow_says(width, kind):
    """phi_t = kappa |grad phi| moves a sphere by dR/dt = -2 / R: R^2 = R0^2 - 4 t, and an iteration is a time step of dt."""
    src = rm.band_of(rm.sphere((0, 0, 0), 0.6), width * HZ)
    dt = float(fm.constants(rm.CELLS).dt)
    for n in (1, 4, 8):
        r, info = fm.band_filter(src, rm.CELLS, kind, n)
        p = fm.x_crossings(r, rm.FIRST, rm.CELLS)
        dev = np.abs(np.linalg.norm(p, axis=1) - np.sqrt(0.36 - 4 * n * dt)).max() / HX
        print(f"sphere, band {width} cells, kind {kind}, {n} iterations: {p.shape[0]} crossings, max deviation {dev:.4f} cells of hx")
        assert p.shape[0] > 800 and info.n_nonfinite == 0 and info.passes == n
        assert dev <= 1.25 * SPHERE_DEV[(width, kind, n)]


# ---- 4. the seam ------------------------------------------------------------------------------------------------------------------------------
def test_the_seam_of_a_union_fills_and_a_region_keeps_the_rest():
    """DESIGN.md 4.18's two spheres.  The seam of their union is a concave crease: the flow lowers the values there (the solid grows, a
    fillet), and raises them on the convex parts (the spheres shrink).  The convex parts are judged where the seam is: within one cell
    of the surface.  Further out, the cells at the band's rim read the backgrounds, a kink that include/m2s.h says the definition does
    not smooth away (the change there reaches -0.20 cells at the outer rim)."""
    ca, ra, cb, rb = (-0.25, 0.0, 0.0), 0.5, (0.3, 0.05, 0.0), 0.45
    da, db = rm.sphere(ca, ra), rm.sphere(cb, rb)
    union = cm.csg(rm.band_of(da, 4 * HZ), rm.band_of(db, 4 * HZ), cm.UNION)
    apart = np.abs(da - db).reshape(-1)[union.cells]
    d = np.minimum(da, db).reshape(-1)[union.cells]
    seam = (apart < HZ) & (np.abs(d) < HZ)
    convex = apart > 4 * HZ
    r, info = fm.band_filter(union, rm.CELLS, fm.MEAN_CURVATURE, 8)
    change = (r.distances.astype(np.float64) - union.distances.astype(np.float64)) / HZ
    near = convex & (np.abs(d) < HZ)
    print(f"seam: {seam.sum()} cells, change {change[seam].min():.4f} .. {change[seam].max():.4f} cells; convex within a cell: {near.sum()} cells, "
          f"{change[near].min():.4f} .. {change[near].max():.4f}; convex, the whole band: {change[convex].min():.4f} .. {change[convex].max():.4f}; {info}")
    assert seam.sum() > 300 and near.sum() > 2000 and info.n_nonfinite == 0
    assert change[seam].min() < 0 and (change[near] > 0).all()
    assert 1.25 * SEAM_FALL <= change[seam].min() <= SEAM_FALL / 1.25
    assert CONVEX_RISE[0] / 1.25 <= change[near].min() and change[near].max() <= 1.25 * CONVEX_RISE[1]
    # the region: within two cells of the crease |D_A - D_B| = 0, as a band of its own with a sign mask
    where = rm.band_of(np.abs(da - db) - 2 * HZ, HZ)
    fillet, info_f = fm.band_filter(union, rm.CELLS, fm.MEAN_CURVATURE, 8, where=where)
    same = fillet.distances.view(np.uint32) == union.distances.view(np.uint32)
    assert same[convex].all() and same[apart >= 2 * HZ].all() and not same[seam].all()
    assert 0 < info_f.n_changed < info.n_changed and (fillet.distances[seam] - union.distances[seam]).min() < 0
