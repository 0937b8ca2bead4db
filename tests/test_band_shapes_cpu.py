"""m2s_band_from_capsules without a GPU: the host build of shape.hip.h (libm2s_probe.so) against the numpy model of the definition
(tests/band_shapes_model.py) bit for bit, the model against float64 within the bound shape.hip.h derives, the index box as a superset of
what the model finds within reach, what the call rejects before any device work, the ABI surface and the C and C++ consumers.

tests/golden/shapes_error.json holds the largest |d_s - float64| the cases below reach, in units of u x scale, beside the derived bound
(`python tests/test_band_shapes_cpu.py --record` writes it)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import band_shapes_model as sm
from mesh_to_sdf_amd import BandField, ShapesInfo, _lib

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "shapes_error.json")


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def _probe():
    p = C.CDLL(os.path.join(ROOT, "mesh_to_sdf_amd", "libm2s_probe.so"))
    p.probe_shape_dist_n.restype = None
    p.probe_shape_dist_n.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    p.probe_shape_box.restype = C.c_int
    p.probe_shape_box.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    p.probe_shape_key.restype = C.c_uint32
    p.probe_shape_key.argtypes = [C.c_float]
    p.probe_shape_unkey.restype = C.c_float
    p.probe_shape_unkey.argtypes = [C.c_uint32]
    p.probe_shape_err_u.restype = C.c_float
    return p


@pytest.fixture(scope="module")
def probe():
    return _probe()


def _probe_dist(shapes, points):
    shapes, points = np.ascontiguousarray(shapes, F), np.ascontiguousarray(points, F)
    out = np.empty(shapes.shape[0], F)
    _probe().probe_shape_dist_n(shapes.shape[0], shapes.ctypes.data, points.ctypes.data, out.ctypes.data)
    return out


@functools.lru_cache(maxsize=None)
def _pairs():
    """(shapes float32[n, 7], points float32[n, 3], scale float64[n]): random capsules and points, and the special cases: a == b, a den
    that underflows to 0, t clamped at either end, t in the open interval, coordinates near 1000, r = 0."""
    rng = np.random.default_rng(7)
    n = 4000
    parts = []

    def add(a, b, r, p):
        parts.append((np.concatenate([a, b, r[:, None]], 1).astype(F), p.astype(F)))

    a, b = rng.uniform(-2, 2, (n, 3)), rng.uniform(-2, 2, (n, 3))
    add(a, b, rng.uniform(0, 0.5, n), rng.uniform(-3, 3, (n, 3)))                                   # general position
    add(a, a, rng.uniform(0, 0.5, n), rng.uniform(-3, 3, (n, 3)))                                   # spheres
    add(a * 1e-20, a * 1e-20 + rng.uniform(-1, 1, (n, 3)) * 3e-23, rng.uniform(0, 0.5, n), rng.uniform(-3, 3, (n, 3)))   # den underflows to 0 or to a denormal
    d = b - a
    add(a, b, rng.uniform(0, 0.5, n), a - d * rng.uniform(0.01, 2, (n, 1)) + rng.normal(0, 0.1, (n, 3)))   # beyond a: t clamped to 0
    add(a, b, rng.uniform(0, 0.5, n), b + d * rng.uniform(0.01, 2, (n, 1)) + rng.normal(0, 0.1, (n, 3)))   # beyond b: t clamped to 1
    add(a, b, np.zeros(n), a + d * rng.uniform(0, 1, (n, 1)) + rng.normal(0, 0.05, (n, 3)))              # beside the segment, bare
    far = np.array([1000.0, -250.0, 0.0])
    add(a + far, b + far, rng.uniform(0, 0.5, n), rng.uniform(-3, 3, (n, 3)) + far)                    # far from the origin
    add(a * 1000, b * 1000, rng.uniform(0, 500, n), rng.uniform(-3000, 3000, (n, 3)))                  # large all over
    shapes = np.concatenate([p[0] for p in parts])
    points = np.concatenate([p[1] for p in parts])
    scale = np.maximum(np.abs(shapes.astype(np.float64)).max(1), np.abs(points.astype(np.float64)).max(1))
    return shapes, points, scale


def _model_dist(shapes, points):
    return sm.dist(shapes[:, 0:3], shapes[:, 3:6], shapes[:, 6], (points[:, 0], points[:, 1], points[:, 2]))


# ---- 1. the host build of shape.hip.h is the model -----------------------------------------------------------------------------------------
def test_the_host_build_equals_the_model_bit_for_bit():
    shapes, points, _ = _pairs()
    got, want = _probe_dist(shapes, points), _model_dist(shapes, points)
    assert np.isfinite(want).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    # the cases are what they claim to be
    n = 4000
    ab = shapes[:, 3:6] - shapes[:, 0:3]
    den = (ab[:, 0] * ab[:, 0] + ab[:, 1] * ab[:, 1]) + ab[:, 2] * ab[:, 2]
    assert (den[n:2 * n] == 0).all() and (den[2 * n:3 * n] == 0).sum() > n // 10 and (den[2 * n:3 * n] < 1e-38).all() and (ab[2 * n:3 * n] != 0).any(1).all()
    ap = points - shapes[:, 0:3]
    with np.errstate(all="ignore"):
        t = ((ap * ab).sum(1) / den)
    assert (t[3 * n:4 * n] < 0).mean() > 0.9 and (t[4 * n:5 * n] > 1).mean() > 0.9 and ((t[5 * n:6 * n] > 0) & (t[5 * n:6 * n] < 1)).mean() > 0.8
    assert not (got.view(np.uint32) == 0x80000000).any()          # never -0


def test_overflowing_differences_give_nan_on_both_sides():
    shapes = np.array([[3e38, 0, 0, -3e38, 0, 0, 1.0], [0, 0, 0, 1, 0, 0, 1.0]], F)
    points = np.array([[0, 0, 0], [-3e38, 3e38, 0]], F)
    got, want = _probe_dist(shapes, points), _model_dist(shapes, points)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)].view(np.uint32), want[~np.isnan(want)].view(np.uint32))


def test_the_key_preserves_the_order(probe):
    xs = np.array([-np.inf, -3e38, -1.5, -1e-45, 0.0, 1e-45, 0.25, 7.0, 3e38, np.inf], F)
    keys = [probe.probe_shape_key(float(x)) for x in xs]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and keys[-1] == 0xff800000
    assert all(F(probe.probe_shape_unkey(k)).view(np.uint32) == x.view(np.uint32) for k, x in zip(keys, xs))


# ---- 2. the model against float64, within the derived bound --------------------------------------------------------------------------------
def _measured():
    shapes, points, scale = _pairs()
    scale = np.maximum(scale, shapes[:, 6].astype(np.float64))
    d32 = _model_dist(shapes, points).astype(np.float64)
    d64 = sm.dist64(shapes[:, 0:3], shapes[:, 3:6], shapes[:, 6], points)
    return float((np.abs(d32 - d64) / (sm.U * scale)).max())


def test_the_model_is_within_the_derived_bound_of_float64(probe):
    golden = json.load(open(GOLDEN))
    assert probe.probe_shape_err_u() == sm.ERR_U == golden["bound_u_scale"]
    got = _measured()
    print(f"max |d_s - float64| = {got:.3f} u x scale; recorded {golden['measured_u_scale']:.3f}; bound {sm.ERR_U}")
    assert got <= sm.ERR_U                                   # the bound shape.hip.h derives
    assert got <= golden["measured_u_scale"]                 # and what was recorded has not been exceeded


# ---- 3. the box holds every point within reach ----------------------------------------------------------------------------------------------
GRIDS = (((-0.5, 0.25, 3.0), (0.125, 0.25, 0.1875), (9, 7, 70)), ((1000.0, -250.0, 0.0), (0.125, 0.25, 0.1875), (24, 20, 22)),
         ((-1.0, -1.0, -1.0), (2.0 ** -5, 2.0 ** -5, 2.0 ** -5), (64, 64, 64)))


def _box(probe, shape7, first, cell, n, exterior):
    s, f, c = np.asarray(shape7, F), np.asarray(first, F), np.asarray(cell, F)
    cnt, out = np.asarray(n, np.uint32), np.zeros(6, np.uint32)
    ok = probe.probe_shape_box(s.ctypes.data, f.ctypes.data, c.ctypes.data, cnt.ctypes.data, float(F(exterior)), out.ctypes.data)
    return ok, out[:3].astype(int), out[3:].astype(int)


@pytest.mark.parametrize("gi", range(len(GRIDS)))
def test_the_index_box_contains_every_point_within_reach(probe, gi):
    first, cell, n = GRIDS[gi]
    rng = np.random.default_rng(11 + gi)
    lo_w = np.asarray(first, np.float64) - 0.5 * np.asarray(cell)
    hi_w = lo_w + np.asarray(n) * np.asarray(cell)
    span = hi_w - lo_w
    cx, cy, cz = np.meshgrid(*sm.centres(first, cell, (0, 0, 0), n), indexing="ij")
    count = 0
    for trial in range(160):
        a = rng.uniform(lo_w - 0.2 * span, hi_w + 0.2 * span)
        b = a if trial % 3 == 0 else a + rng.normal(0, 0.3, 3) * span
        r = (0.0, 0.37 * float(min(cell)), 2.6 * float(max(cell)))[trial % 3] if trial % 5 else float(rng.uniform(0, 0.4) * span.min())
        ext = (0.0, 1.5 * float(min(cell)), 3.0 * float(max(cell)))[trial % 3] if trial % 4 else float(cell[0])
        if trial % 40 == 7:      # the surface exactly through cell centres: r such that d_s == exterior is met with equality
            a = b = np.array([first[m] + 3 * cell[m] for m in range(3)])
            r, ext = 2 * cell[2], cell[2]
        shape7 = np.concatenate([a, b, [r]]).astype(F)
        ok, lo, hi = _box(probe, shape7, first, cell, n, ext)
        assert ok == 1
        near = sm.dist(shape7[0:3], shape7[3:6], shape7[6], (cx, cy, cz)) <= F(ext)
        inbox = np.zeros(n, bool)
        if (lo < hi).all():
            inbox[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
        assert (lo >= 0).all() and (hi <= np.asarray(n)).all()
        assert not (near & ~inbox).any(), (trial, shape7, ext, lo, hi)
        count += bool(near.any())
        # ... and is not wasteful: per axis no longer than the segment's extent grown by r + exterior on both sides, plus two layers
        s64 = shape7.astype(np.float64)
        for m in range(3):
            assert hi[m] - lo[m] <= (abs(s64[3 + m] - s64[m]) + 2 * (s64[6] + float(F(ext)))) / cell[m] + 2, (trial, m, lo, hi)
    assert count > 40


def test_the_box_of_an_unsound_shape_is_refused(probe):
    first, cell, n = GRIDS[0]
    for bad in ([np.nan, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, np.inf, 0, 1], [0, 0, 0, 0, 0, 0, -1e-3], [0, 0, 0, 0, 0, 0, np.inf], [0, 0, 0, 0, 0, 0, np.nan]):
        assert _box(probe, bad, first, cell, n, 0.5)[0] == 0
    assert _box(probe, [0, 0, 0, 0, 0, 0, 0], first, cell, n, 0.0)[0] == 1
    assert sm.sound([[0, 0, 0]] * 3, [[0, 0, 0]] * 3, [0.0, -0.0, -1.0]).tolist() == [True, True, False]


# ---- 4. what the call rejects before any device work ---------------------------------------------------------------------------------------
def _opts(**kw):
    o = _lib.M2SOpts()
    o.struct_size, o.device = C.sizeof(o), -1
    for k, v in kw.items():
        setattr(o, k, v)
    return C.byref(o)


_PEER = (C.c_void_p * 1)(0x1000)
BAD_OPTS = (("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4), ("mem_kind", 5), ("n_peer_out", 1),
            ("peer_out", C.cast(_PEER, C.POINTER(C.c_void_p))))


def _grid(count=(8, 8, 8), cell=(0.5, 0.5, 0.5)):
    g = _lib.M2SGrid()
    for m in range(3):
        g.first_cell[m], g.cell_size[m], g.cell_count[m] = 0.25, cell[m], count[m]
    return g


def test_the_call_rejects_bad_arguments_before_any_device_work(lib):
    BAD = _lib.ERR_BAD_ARG
    a = (C.c_float * 6)(1, 1, 1, 2, 2, 2)
    h = C.c_void_p(0x77)
    good = _lib.M2SBandShapesOpts(16, 0.5, 0.5, 0.25)
    g = _grid()

    def call(grid=g, pa=a, n=2, so=good, fo=None, opts=None, out=C.byref(h)):
        return lib.m2s_band_from_capsules(C.byref(grid) if grid is not None else None, pa, None, None, n, C.byref(so) if so is not None else None, fo,
                                          opts, out, None, None)

    assert call(out=None) == BAD and "out is NULL" in _lib.last_error()
    assert call(grid=None) == BAD and h.value is None
    assert call(so=None) == BAD and "m2s_band_shapes_opts" in _lib.last_error()
    for size in (0, 12, 20):
        assert call(so=_lib.M2SBandShapesOpts(size, 0.5, 0.5, 0.25)) == BAD and "struct_size" in _lib.last_error()
    for bad in (-1e-3, float("nan"), float("inf")):
        assert call(so=_lib.M2SBandShapesOpts(16, bad, 0.5, 0.25)) == BAD and "half-widths" in _lib.last_error()
        assert call(so=_lib.M2SBandShapesOpts(16, 0.5, bad, 0.25)) == BAD and "half-widths" in _lib.last_error()
        assert call(so=_lib.M2SBandShapesOpts(16, 0.5, 0.5, bad)) == BAD and "radius" in _lib.last_error()
    for size in (0, 8, 16):
        assert call(fo=C.byref(_lib.M2SBandFieldOpts(size, 1.0, 1.0))) == BAD and "m2s_band_field_opts" in _lib.last_error()
    assert call(fo=C.byref(_lib.M2SBandFieldOpts(12, -1.0, 1.0))) == BAD
    assert call(pa=None) == BAD and "a is NULL" in _lib.last_error()
    assert call(n=1 << 32) == BAD and "2^32" in _lib.last_error()
    for field, value in BAD_OPTS:
        assert call(opts=_opts(**{field: value})) == BAD, field
    assert call(grid=_grid(count=(1 << 12, 1 << 12, 1 << 12))) == BAD and "2^36" in _lib.last_error()
    assert call(grid=_grid(count=(1 << 33, 2, 2))) == BAD
    assert call(grid=_grid(count=(8, 0, 8))) == BAD
    assert call(grid=_grid(cell=(0.5, -0.5, 0.5))) == BAD and "cell_size" in _lib.last_error()
    assert h.value is None


# ---- 5. the ABI surface and the consumers --------------------------------------------------------------------------------------------------
def test_the_entry_point_is_exported_and_declared(lib):
    assert "m2s_band_from_capsules" in _lib.EXPORTS and hasattr(lib, "m2s_band_from_capsules")
    assert lib.m2s_version() == 5
    raw = open(os.path.join(ROOT, "include", "m2s.h")).read()
    assert "#define M2S_VERSION_MINOR 5" in raw
    hdr = " ".join(raw.split())
    for text in ("typedef struct m2s_band_shapes_opts {", "float exterior, interior;", "} m2s_band_shapes_opts;", "uint64_t n_off_grid;",
                 "} m2s_band_shapes_info;", "int m2s_band_from_capsules(const m2s_grid* grid, const float* a", "d_s = sqrtf((e.x*e.x + e.y*e.y) + e.z*e.z) - r",
                 "-interior <= D <= exterior", "m2s_band_redistance makes distances of it again"):
        assert text in hdr, text
    assert C.sizeof(_lib.M2SBandShapesOpts) == 16 and C.sizeof(_lib.M2SBandShapesInfo) == 32
    assert ShapesInfo._fields == ("n_cells", "n_inside", "n_skipped", "n_off_grid")
    for name in ("from_capsules", "from_spheres", "from_points", "from_edges"):
        assert hasattr(BandField, name), name
    hpp = open(os.path.join(ROOT, "include", "mesh_to_sdf.hpp")).read()
    for text in ("struct ShapesInfo : m2s_band_shapes_info", "static BandField from_capsules(", "static BandField from_spheres("):
        assert text in hpp, text
    for doc, text in (("README.md", "m2s_band_from_capsules"), ("DESIGN.md", "m2s_band_from_capsules"), ("DESIGN.md", "4.23")):
        assert text in open(os.path.join(ROOT, doc)).read(), (doc, text)
    src = open(os.path.join(ROOT, "mesh_to_sdf_amd", "csrc", "Makefile")).read()
    assert "band_shapes.o" in src and "shape.hip.h" in src and "warm_band_shapes" in open(os.path.join(ROOT, "mesh_to_sdf_amd", "csrc", "capi.hip")).read()
    shape_h = open(os.path.join(ROOT, "mesh_to_sdf_amd", "csrc", "shape.hip.h")).read()
    assert "correctly rounded" in shape_h and "m2s_band_redistance" in shape_h and "SHAPE_ERR_U = 96.0f" in shape_h


@pytest.mark.parametrize("cc,std,lang", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "c++")])
def test_the_header_compiles_as_c99_and_cxx17(tmp_path, cc, std, lang):
    src = tmp_path / ("only_header." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "m2s.h"\nint main(void) { return (int)sizeof(m2s_band_shapes_opts) - 16 + (int)sizeof(m2s_band_shapes_info) - 32; }\n')
    subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


CONSUMERS = [("gcc", "-std=c99", "tests/c/band_shapes_smoke.c"), ("g++", "-std=c++17", "tests/cpp/band_shapes_tests.cpp")]


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
    json.dump({"bound_u_scale": sm.ERR_U, "measured_u_scale": _measured(),
               "cases": "tests/test_band_shapes_cpu.py _pairs(): 32000 (capsule, point) pairs, scale = the largest |coordinate| and r"}, open(GOLDEN, "w"), indent=1)
    print(open(GOLDEN).read())
