"""m2s_band_measure without a GPU: the numpy model of the definition (tests/band_measure_model.py) against independent float64 measures
of the mesh band_isosurface_model.extract returns and against analytic spheres, its integer properties, what the call rejects before any
device work, the ABI surface and the C and C++ consumers.

Measured with the model (tests/golden/band_measure_error.json holds the figures; `python tests/test_band_measure_cpu.py --record` writes
them): the model and the float64 measure of the extracted mesh differ by at most 1.7e-7 relative in area, 7.6e-9 in volume and 1.5e-8 of
the largest coordinate in the centroid on grids within 1024 cell sizes of the origin: the float32 rounding of the mesh's vertices, which
the model does not share.  Against the analytic sphere the area is 0.30 % low and the volume 0.56 % low at R = 10.3 cells, 0.074 % and
0.14 % at R = 20.6: second order."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import band_components_model as ccm
import band_csg_model as cm
import band_isosurface_model as bim
import band_measure_model as mm
import isosurface_model as im
from mesh_to_sdf_amd import BandField, Components, Measure, _lib

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "band_measure_error.json")
CAP = 1e-5            # a condition on the model against the mesh, not a measurement: it holds whatever was recorded
ANISO = (0.5, 0.25, 0.125)


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def _union(*d):
    return functools.reduce(np.minimum, d)


@functools.lru_cache(maxsize=None)
def _mesh_cases():
    """(name, shape, first_cell, cell_size, cells, values): spheres and two-sphere unions on 32^3 unit cells and on 24 x 40 x 70 with
    cells (0.5, 0.25, 0.125); every coordinate stays below 1024 cell sizes."""
    s, s2 = (32, 32, 32), (24, 40, 70)
    out = []
    for name, shape, first, cell, d, width in (
            ("sphere 32^3", s, (-3.0, 2.0, 5.0), (1.0, 1.0, 1.0), mm.sphere_distance(s, (15.2, 16.1, 15.7), 10.3), 2.0),
            ("union 32^3", s, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), _union(mm.sphere_distance(s, (11.3, 12.2, 13.1), 7.4), mm.sphere_distance(s, (20.1, 19.4, 18.2), 6.7)), 2.0),
            ("sphere 24x40x70", s2, (-6.0, 1.0, 100.0), ANISO, mm.sphere_distance(s2, (6.1, 5.05, 4.4), 3.3, ANISO), 0.65),
            ("union 24x40x70", s2, (0.0, 0.0, 0.0), ANISO, _union(mm.sphere_distance(s2, (4.1, 4.05, 3.4), 2.3, ANISO), mm.sphere_distance(s2, (7.6, 6.0, 5.2), 2.6, ANISO)), 0.65)):
        cells, values = mm.band_of(d, width)
        out.append((name, shape, first, cell, cells, values))
    return out


def _deviation(shape, first, cell, cells, values, iso=0.0):
    """(model Raw, relative deviation of the model from the float64 measures of the extracted mesh in area, volume and centroid; the
    centroid's in units of the largest vertex coordinate)."""
    raw = mm.measure(shape, cell, cells, values, iso)
    V, T, n_open = bim.extract(im.GridI(first, cell, shape), cells, values, iso)
    assert int(raw.n_triangles[0]) == len(T) and int(raw.n_vertices[0]) == len(V) and int(raw.n_open[0]) == n_open
    area, volume, centroid = mm.derived(raw, first, cell)
    ma, mv, mc = mm.mesh_area(V, T), im.volume(V, T), mm.mesh_centroid(V, T)
    return raw, (abs(area - ma) / ma, abs(volume - mv) / abs(mv), float(np.abs(np.asarray(centroid) - mc).max() / np.abs(V).max()))


def _sphere_errors():
    """{R: (area error, volume error)} of the model against the analytic sphere, radii of about 10 and 20 cells."""
    out = {}
    for R, n in ((10.3, 32), (20.6, 56)):
        s, c = (n, n, n), (n / 2 - 0.3, n / 2 + 0.1, n / 2 - 0.2)
        raw = mm.measure(s, (1, 1, 1), *mm.band_of(mm.sphere_distance(s, c, R), 2.0))
        assert mm.closed(raw) and mm.euler(raw) == 2
        area, volume, centroid = mm.derived(raw, (0, 0, 0), (1, 1, 1))
        assert np.abs(np.asarray(centroid) - c).max() < 1e-3
        out[R] = (area / (4 * np.pi * R * R) - 1, volume / (4 / 3 * np.pi * R ** 3) - 1)
    return out


def _measured():
    dev = np.array([_deviation(*c[1:])[1] for c in _mesh_cases()])
    sph = _sphere_errors()
    return {"mesh_deviation": dict(zip(("area", "volume", "centroid"), (float(v) for v in dev.max(0)))),
            "sphere_error": {f"R{R}": {"area": float(a), "volume": float(v)} for R, (a, v) in sph.items()}}


# ---- 1. the model against float64 measures of the extracted mesh ---------------------------------------------------------------------------
def test_the_model_agrees_with_float64_measures_of_the_extracted_mesh():
    golden = json.load(open(GOLDEN))["mesh_deviation"]
    for name, *case in _mesh_cases():
        raw, dev = _deviation(*case)
        print(f"{name}: {int(raw.n_triangles[0])} triangles, deviation area {dev[0]:.3g} volume {dev[1]:.3g} centroid {dev[2]:.3g}")
        assert mm.closed(raw) and mm.euler(raw) == 2, name
        for what, got in zip(("area", "volume", "centroid"), dev):
            assert golden[what] <= CAP and got <= min(4 * golden[what], CAP), (name, what, got, golden[what])


def test_an_iso_other_than_zero_measures_the_offset_surface():
    shape, first, cell = (32, 32, 32), (-3.0, 2.0, 5.0), (1.0, 1.0, 1.0)
    cells, values = mm.band_of(mm.sphere_distance(shape, (15.2, 16.1, 15.7), 10.3), 2.6)   # the cells d = 0.7 cuts reach |d| = 0.7 + sqrt(3)
    raw, dev = _deviation(shape, first, cell, cells, values, iso=0.7)
    assert mm.closed(raw) and max(dev) <= CAP
    area, volume, _ = mm.derived(raw, first, cell)
    assert abs(area / (4 * np.pi * 11.0 ** 2) - 1) < 0.004 and abs(volume / (4 / 3 * np.pi * 11.0 ** 3) - 1) < 0.007


# ---- 2. the grid's position ----------------------------------------------------------------------------------------------------------------
def test_the_measure_does_not_degrade_far_from_the_origin():
    """48^3 cells of 0.01 at x = 0 and at x = 1000.  The raw sums know no first_cell: area and volume are the same bits and the centroid
    moves by the shift.  The extracted mesh's float32 vertices do degrade: its float64 measure moves by 8.6e-6 in area and 1.6e-6 in volume
    between the two positions (at the origin it is within 2e-8 of the model).  Against the analytic sphere the model's volume stays closer
    than the far mesh's.  The mesh's AREA at x = 1000 is nearer the analytic value than the model's, by accident: rounding noise on the
    vertices always adds area and marching cubes' area is low (0.13 % here), so the area is judged against the same surface at the origin."""
    shape, cell, R, centre = (48, 48, 48), (0.01, 0.01, 0.01), 0.153, (0.22, 0.25, 0.24)
    cells, values = mm.band_of(mm.sphere_distance(shape, centre, R, cell), 0.02)
    raw = mm.measure(shape, cell, cells, values)
    assert mm.closed(raw)
    near, far = (0.0, 0.0, 0.0), (1000.0, 0.0, 0.0)
    a0, v0, c0 = mm.derived(raw, near, cell)
    a1, v1, c1 = mm.derived(raw, far, cell)
    assert (a0, v0) == (a1, v1) and abs(c1[0] - c0[0] - 1000.0) < 1e-9 and c1[1:] == c0[1:]
    assert np.abs(np.asarray(c0) - centre).max() < 1e-5
    m = {}
    for first in (near, far):
        V, T, _ = bim.extract(im.GridI(first, cell, shape), cells, values)
        m[first] = (mm.mesh_area(V, T), im.volume(V, T))
    assert abs(m[near][0] - a0) / a0 < 1e-7 and abs(m[near][1] - v0) / v0 < 1e-7
    area_shift, volume_shift = abs(m[far][0] - m[near][0]) / a0, abs(m[far][1] - m[near][1]) / v0
    print(f"the mesh's float64 measure moves by {area_shift:.3g} in area and {volume_shift:.3g} in volume between x = 0 and x = 1000; the model by 0")
    assert area_shift > 1e-6 and volume_shift > 1e-7
    exact = 4 / 3 * np.pi * R ** 3
    assert abs(v1 - exact) < abs(m[far][1] - exact)


def test_the_raw_sums_do_not_depend_on_the_cell_sizes_except_the_area():
    name, shape, first, cell, cells, values = _mesh_cases()[2]
    a, b = mm.measure(shape, cell, cells, values), mm.measure(shape, (1.0, 1.0, 1.0), cells, values)
    for f in mm.INT_FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)) == (f != "area_q"), f
    assert a.area_exponent == -2 and b.area_exponent == 0


# ---- 3. the analytic sphere ----------------------------------------------------------------------------------------------------------------
def test_the_error_against_the_analytic_sphere_is_second_order():
    golden = json.load(open(GOLDEN))["sphere_error"]
    err = _sphere_errors()
    for R, (a, v) in err.items():
        print(f"R = {R}: area {a:+.5f}, volume {v:+.5f}")
        assert abs(a - golden[f"R{R}"]["area"]) < 1e-9 and abs(v - golden[f"R{R}"]["volume"]) < 1e-9
    (a10, v10), (a20, v20) = err[10.3], err[20.6]
    assert a10 < 0 and v10 < 0 and abs(a10) < 0.004 and abs(v10) < 0.007
    assert abs(a20) < abs(a10) / 2 and abs(v20) < abs(v10) / 2


# ---- 4. integer properties -----------------------------------------------------------------------------------------------------------------
def _fields_equal(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in mm.INT_FIELDS)


def test_the_groups_sum_to_the_unlabelled_measure():
    rng = np.random.default_rng(5)
    name, shape, first, cell, cells, values = _mesh_cases()[3]
    whole = mm.measure(shape, cell, cells, values)
    labels = rng.integers(0, 5, cells.size).astype(np.uint32)
    parts = mm.measure(shape, cell, cells, values, labels=labels, n_groups=7)
    assert parts.n_skipped == 0 and not parts.n_triangles[5:].any() and not parts.area_q[5:].any()
    for f in mm.INT_FIELDS:
        assert np.array_equal(getattr(parts, f).sum(0, keepdims=True).astype(getattr(whole, f).dtype), getattr(whole, f)), f
    # labels at or above n_groups leave their cells and vertices out, and are counted
    labels[rng.random(cells.size) < 0.2] = mm.LABEL_NONE
    some, more = (mm.measure(shape, cell, cells, values, labels=labels, n_groups=n) for n in (3, 7))
    assert some.n_skipped == int((labels >= 3).sum()) > more.n_skipped == int((labels >= 7).sum()) > 0
    for f in mm.INT_FIELDS:   # a group's sums do not depend on which other groups are counted
        assert np.array_equal(getattr(some, f), getattr(more, f)[:3]), f
    # the values of skipped places still serve as corners: dropping those places from the band instead opens cells
    kept = labels < 3
    cut = mm.measure(shape, cell, cells[kept], values[kept], labels=labels[kept], n_groups=3)
    assert cut.n_skipped == 0 and cut.n_triangles.sum() < some.n_triangles.sum() and cut.n_open.sum() > some.n_open.sum()


def test_open_cells_and_border_vertices_are_counted():
    # a sphere that the grid's box cuts: vertices on the boundary faces, and a band too thin to close every cell
    shape = (20, 20, 20)
    d = mm.sphere_distance(shape, (3.2, 9.7, 10.1), 7.3)
    cells, values = mm.band_of(d, 2.0)
    raw = mm.measure(shape, (1, 1, 1), cells, values)
    V, T, n_open = bim.extract(im.GridI((0, 0, 0), (1, 1, 1), shape), cells, values)
    assert int(raw.n_border[0]) > 0 and int(raw.n_open[0]) == n_open == 0 and not mm.closed(raw)
    assert int(raw.n_triangles[0]) == len(T) and int(raw.n_vertices[0]) == len(V)
    # the border vertices are exactly the mesh's vertices that lie in a boundary face off their own edge's axis: those with two
    # integer coordinates of which one is on a face; count them from the mesh
    idx = V.astype(np.float64)
    on_face = (idx == 0) | (idx == np.array(shape) - 1)
    whole = idx == np.round(idx)
    assert int(raw.n_border[0]) == int(((on_face & whole).sum(1) >= 1).sum())
    cells, values = mm.band_of(d, 0.6)
    raw = mm.measure(shape, (1, 1, 1), cells, values)
    V, T, n_open = bim.extract(im.GridI((0, 0, 0), (1, 1, 1), shape), cells, values)
    assert int(raw.n_open[0]) == n_open > 0 and int(raw.n_triangles[0]) == len(T) and int(raw.n_vertices[0]) == len(V)


def _labels26(shape, cells):
    band = cm.Band(shape, cells.astype(np.int64), np.zeros(cells.size, F), None, 1.0, 1.0)
    cc = ccm.components(band, 26)
    return cc.labels, cc.count


def test_euler_characteristic_of_a_torus_and_a_sphere_and_a_cavity_is_negative():
    shape = (40, 40, 24)
    torus = mm.torus_distance(shape, (19.6, 20.3, 11.8), 11.0, 4.2)
    cells, values = mm.band_of(torus, 2.0)
    raw = mm.measure(shape, (1, 1, 1), cells, values)
    assert mm.closed(raw) and mm.euler(raw) == 0
    _, volume, _ = mm.derived(raw, (0, 0, 0), (1, 1, 1))
    assert abs(volume / (2 * np.pi ** 2 * 11.0 * 4.2 ** 2) - 1) < 0.02
    # a shell: the outer skin and the cavity's skin are two components at connectivity 26; the cavity's volume is negative
    shape = (32, 32, 32)
    c = (15.4, 15.8, 16.1)
    shell = np.maximum(mm.sphere_distance(shape, c, 12.0), -mm.sphere_distance(shape, c, 5.0))
    cells, values = mm.band_of(shell, 1.8)
    labels, count = _labels26(shape, cells)
    assert count == 2
    raw = mm.measure(shape, (1, 1, 1), cells, values, labels=labels, n_groups=2)
    assert all(mm.closed(raw, g) and mm.euler(raw, g) == 2 for g in (0, 1))
    v = [mm.derived(raw, (0, 0, 0), (1, 1, 1), g)[1] for g in (0, 1)]
    assert v[0] > 0 > v[1] and abs(v[0] / (4 / 3 * np.pi * 12.0 ** 3) - 1) < 0.01 and abs(-v[1] / (4 / 3 * np.pi * 5.0 ** 3) - 1) < 0.03
    whole = mm.measure(shape, (1, 1, 1), cells, values)
    assert int(whole.volume_q[0]) == int(raw.volume_q.sum()) and mm.euler(whole) == 4


def test_an_octahedron_has_exact_sums():
    """One inside point among its 26 neighbours: the octahedron with vertices half a cell along the axes, which the C and C++ consumers
    measure on the GPU.  Every term is exact."""
    shape, cell = (8, 8, 8), (0.5, 0.5, 0.5)
    i, j, k = np.meshgrid(*(np.arange(3, 6),) * 3, indexing="ij")
    cells = np.sort((k + 8 * j + 64 * i).reshape(-1)).astype(np.uint64)
    values = np.where(cells == 4 + 8 * 4 + 64 * 4, F(-1), F(1)).astype(F)
    raw = mm.measure(shape, cell, cells, values)
    w = int(np.floor(np.ldexp(np.float64(np.sqrt(F(0.01171875))), 26)))
    assert (int(raw.n_triangles[0]), int(raw.n_vertices[0]), int(raw.n_open[0]), int(raw.n_border[0])) == (8, 6, 0, 0) and mm.euler(raw) == 2
    assert int(raw.volume_q[0]) == 1 << 20 and raw.moment_q[0].tolist() == [4096] * 3 and raw.area_exponent == -2 and int(raw.area_q[0]) == 8 * w
    area, volume, centroid = mm.derived(raw, (0.25, 0.25, 0.25), cell)
    assert volume == 0.125 / 6 and centroid == [2.25] * 3 and abs(area - 4 * np.sqrt(0.01171875)) < 1e-7


def test_the_edge_rule_of_the_kernel_is_the_tables():
    """band_measure.hip takes an edge's corner offsets from e = 4 a + r by rule: (r >> 1, r & 1) on the two other axes."""
    for e in range(12):
        a, r = e >> 2, e & 3
        other = [x for x in range(3) if x != a]
        want = [0, 0, 0]
        want[other[0]], want[other[1]] = r >> 1, r & 1
        assert im.EDGE_AXIS[e] == a and im.EDGE_OFF[e].tolist() == want, e


def test_exponent_and_limits():
    assert [mm.exponent_of(v) for v in (1.0, 0.25, 0.3, 3.9, 4.0, 1e-45, 2e-45)] == [0, -2, -2, 1, 2, -149, -149]
    assert mm.area_exponent((0.5, 0.25, 0.125)) == -2 and mm.area_exponent((0.01, 0.01, 0.01)) == -14
    assert mm.moment_limit_ok((2048, 2048, 2048)) and mm.moment_limit_ok((1 << 16, 1 << 16, 1 << 1)) and not mm.moment_limit_ok((1 << 26, 1, 1))


# ---- 5. errors without a device ------------------------------------------------------------------------------------------------------------
def _opts(**kw):
    o = _lib.M2SOpts()
    o.struct_size, o.device = C.sizeof(o), -1
    for k, v in kw.items():
        setattr(o, k, v)
    return C.byref(o)


_PEER = (C.c_void_p * 1)(0x1000)
BAD_OPTS = (("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4), ("mem_kind", 5), ("n_peer_out", 1),
            ("peer_out", C.cast(_PEER, C.POINTER(C.c_void_p))))


def test_measure_rejects_what_needs_no_handle(lib):
    BAD = _lib.ERR_BAD_ARG
    fake = C.c_void_p(0x1234)                     # never dereferenced: every call below fails before it looks at the handle
    out = (_lib.M2SBandMeasureRecord * 2)()
    labels = (C.c_uint32 * 4)()
    good = _lib.M2SBandMeasureOpts(8, 0.0)

    def call(band=fake, mo=C.byref(good), lab=None, n_groups=0, opts=None, rec=out, info=None):
        return lib.m2s_band_measure(band, mo, lab, n_groups, opts, rec, info, None)

    assert call(band=None) == BAD and "band is NULL" in _lib.last_error()
    assert call(rec=None) == BAD and "measures_out is NULL" in _lib.last_error()
    for size in (0, 4, 12):
        assert call(mo=C.byref(_lib.M2SBandMeasureOpts(size, 0.0))) == BAD and "m2s_band_measure_opts" in _lib.last_error()
    for iso in (float("nan"), float("inf"), -float("inf")):
        assert call(mo=C.byref(_lib.M2SBandMeasureOpts(8, iso))) == BAD and "iso" in _lib.last_error()
    for size in (0, 8, 16, 32):
        assert call(info=C.byref(_lib.M2SBandMeasureInfo(size))) == BAD and "m2s_band_measure_info" in _lib.last_error()
    assert call(lab=labels, n_groups=0) == BAD and "n_groups = 0" in _lib.last_error()
    assert call(lab=labels, n_groups=1 << 32) == BAD and "M2S_LABEL_NONE" in _lib.last_error()
    for field, value in BAD_OPTS:
        assert call(opts=_opts(**{field: value})) == BAD, field
    assert not any(bytes(out))                    # nothing was written


# ---- 6. the ABI surface and the consumers --------------------------------------------------------------------------------------------------
def test_the_entry_point_is_exported_and_declared(lib):
    assert "m2s_band_measure" in _lib.EXPORTS and hasattr(lib, "m2s_band_measure")
    hdr = " ".join(open(os.path.join(ROOT, "include", "m2s.h")).read().split())
    for text in ("typedef struct m2s_band_measure_opts { uint32_t struct_size; float iso; } m2s_band_measure_opts;",
                 "uint64_t n_triangles, n_vertices, n_open, n_border;", "uint64_t area_q; int64_t volume_q; int64_t moment_q[3];",
                 "double area, volume, centroid[3];", "} m2s_band_measure_record;",
                 "typedef struct m2s_band_measure_info { uint32_t struct_size; int32_t area_exponent; uint64_t n_groups, n_skipped; } m2s_band_measure_info;",
                 "int m2s_band_measure(const m2s_band* band, const m2s_band_measure_opts* mopts, const uint32_t* labels",
                 "llrint((nz * sz) * 2^20)", "llrint((n[c] * s) * 2^8)", "2^(24 - E)", "total_cells * max(cell_count) < 2^50", "n_open == 0 && n_border == 0",
                 "depend on the grid's origin", "Euler characteristic"):
        assert text in hdr, text
    assert C.sizeof(_lib.M2SBandMeasureRecord) == 112 and C.sizeof(_lib.M2SBandMeasureOpts) == 8 and C.sizeof(_lib.M2SBandMeasureInfo) == 24
    assert _lib.M2SBandMeasureRecord.area_q.offset == 32 and _lib.M2SBandMeasureRecord.moment_q.offset == 48 and _lib.M2SBandMeasureRecord.centroid.offset == 88
    assert Measure._fields == ("n_triangles", "n_vertices", "n_open", "n_border", "area_q", "volume_q", "moment_q", "area", "volume", "centroid", "closed", "euler")
    for name in ("measure", "area", "volume", "centroid"):
        assert hasattr(BandField, name), name
    assert hasattr(Components, "measure")
    hpp = open(os.path.join(ROOT, "include", "mesh_to_sdf.hpp")).read()
    for text in ("struct Measure : m2s_band_measure_record", "Measure measure(float iso = 0.0f) const",
                 "std::vector<Measure> measure(const Components& c, float iso = 0.0f) const"):
        assert text in hpp, text
    for doc, text in (("README.md", "m2s_band_measure"), ("DESIGN.md", "m2s_band_measure"), ("DESIGN.md", "4.22")):
        assert text in open(os.path.join(ROOT, doc)).read(), (doc, text)
    src = open(os.path.join(ROOT, "mesh_to_sdf_amd", "csrc", "Makefile")).read()
    assert "band_measure.o" in src and "warm_band_measure" in open(os.path.join(ROOT, "mesh_to_sdf_amd", "csrc", "capi.hip")).read()


CONSUMERS = [("gcc", "-std=c99", "tests/c/band_measure_smoke.c"), ("g++", "-std=c++17", "tests/cpp/band_measure_tests.cpp")]


def build_consumer(tmp_path, cc, std, src):
    exe = str(tmp_path / os.path.basename(src).split(".")[0])
    subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                           os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    return exe


@pytest.mark.parametrize("cc,std,src", CONSUMERS)
def test_consumers_compile_and_check_their_arguments(lib, tmp_path, cc, std, src):
    r = subprocess.run([build_consumer(tmp_path, cc, std, src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


if __name__ == "__main__" and "--record" in sys.argv:
    json.dump(_measured(), open(GOLDEN, "w"), indent=1)
    print(open(GOLDEN).read())
