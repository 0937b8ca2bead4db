"""Surface sampling without a GPU: the numpy model of the contract (tests/sample_model.py) against known answers and against the
statistics it promises, the host build of csrc/sample.hip.h against that model bit for bit, the exports, and the argument checks that
happen before any device work."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_model as sm  # noqa: E402
from mesh_to_sdf_amd import M2SPanic, Topology, _lib, meshes, sample_surface, surface_area  # noqa: E402

F = np.float32
U32 = np.uint32
U64 = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(os.path.dirname(_lib.SO_PATH), "libm2s_probe.so")

# (counter) / (key) -> (r0, r1, r2, r3): the known answers of include/m2s.h's generator
KATS = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
        ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, F)).view(U32)


# ---- the model itself --------------------------------------------------------------------------------------------------------------------
def test_model_philox_known_answers():
    for counter, key, want in KATS:
        got = sm.philox4x32_10(np.array(counter, U64), np.array(key, U64))
        assert got.tolist() == list(want)


def test_model_counter_and_key_use_both_words():
    """g >> 32 is the counter's second word and seed >> 32 the key's second: a sample beyond 2^32 is not sample g mod 2^32."""
    g = np.array([5, 5 + 2 ** 32, 2 ** 40 + 5], U64)
    r = sm.sample_random(2 ** 32 + 7, g)
    for k, gk in enumerate(g.tolist()):
        want = sm.philox4x32_10(np.array([gk & 0xFFFFFFFF, gk >> 32, 0, 0], U64), np.array([7, 1], U64))
        assert r[k].tolist() == want.tolist()
    assert len({tuple(x) for x in r.tolist()}) == 3
    assert sm.sample_random(7, g[:1]).tolist() != r[:1].tolist()


def _standardised_chi2(counts, expected):
    """(chi^2 - k) / sqrt(2 k) over bins pooled, in order, until each expects >= 20; k = bins - 1."""
    c, e, cc, ee = [], [], 0.0, 0.0
    for ci, ei in zip(counts, expected):
        cc, ee = cc + ci, ee + ei
        if ee >= 20:
            c.append(cc)
            e.append(ee)
            cc = ee = 0.0
    if ee > 0:
        c[-1] += cc
        e[-1] += ee
    c, e = np.array(c), np.array(e)
    k = c.size - 1
    assert k >= 1
    return float((((c - e) ** 2 / e).sum() - k) / np.sqrt(2.0 * k)), k


@pytest.fixture(scope="module")
def million():
    """10^6 samples of a mesh whose triangle areas span 1 : 4000, two seeds, computed once."""
    tris = sm.triangles_of(sm.graded_fan(64, 4000.0))
    A, _ = sm.tri_area2(tris)
    assert A.max() / A.min() >= 1000
    return tris, [sm.sample(tris, 1_000_000, seed=s) for s in (0, 2 ** 32 + 7)]


def test_model_triangle_counts_follow_the_weights(million):
    tris, runs = million
    A, _ = sm.tri_area2(tris)
    w, e = sm.weights(A)
    n = 1_000_000
    for s in runs:
        counts = np.bincount(s["triangle"], minlength=tris.shape[0]).astype(np.float64)
        z, k = _standardised_chi2(counts, n * w.astype(np.float64) / float(w.sum()))
        assert k >= 40 and z < 5, (z, k)
        z_wrong, _ = _standardised_chi2(counts, np.full(tris.shape[0], n / tris.shape[0]))
        assert z_wrong > 5, z_wrong      # equal probability per triangle is rejected: the statistic can tell


def test_model_points_are_uniform_within_triangles(million):
    tris, runs = million
    for s in runs:
        u, v = s["uv"][:, 0].astype(np.float64), s["uv"][:, 1].astype(np.float64)
        assert (u > 0).all() and (v > 0).all() and (u + v <= 1 + 2.0 ** -23).all()
        # the four midpoint sub-triangles: at a (u + v < 1/2), at b (u > 1/2), at c (v > 1/2), the middle one
        which = np.where(u > 0.5, 1, np.where(v > 0.5, 2, np.where(u + v < 0.5, 0, 3)))
        counts = np.bincount(which, minlength=4).astype(np.float64)
        z, k = _standardised_chi2(counts, np.full(4, u.size / 4))
        assert k == 3 and z < 5, (z, counts)
        # the points lie in their triangles' plane z = 0 and inside their bounding boxes
        t = s["triangle"]
        assert (s["point"][:, 2] == 0).all()
        assert (s["point"][:, :2] >= tris[t].min(1)[:, :2]).all() and (s["point"][:, :2] <= tris[t].max(1)[:, :2]).all()


def test_model_area_and_degenerates():
    v, idx = meshes.cube()
    assert sm.table(sm.triangles_of(v, idx))[3] == 24.0
    dv, didx = sm.with_degenerates(v, idx)
    tris = sm.triangles_of(dv, didx)
    A, n = sm.tri_area2(tris)
    raw = np.sqrt((n.astype(np.float64) ** 2).sum(1))
    assert (A == 0).sum() == 4 and np.isnan(raw).sum() >= 1 and np.isinf(n).any()   # two of area 0, a NaN, an overflow
    C, W, e, area = sm.table(tris)
    assert area == 24.0
    s = sm.sample(tris, 20000, seed=3)
    assert (A[s["triangle"]] > 0).all()
    assert sm.table(np.zeros((5, 3, 3), F))[1:] == (0, None, 0.0)


# ---- the host build of sample.hip.h against the model ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        _lib.build()
    L = C.CDLL(PROBE)
    L.probe_philox.argtypes = [C.c_void_p] * 3
    L.probe_sample_random.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    L.probe_tri_weight_area.restype = C.c_float
    L.probe_tri_weight_area.argtypes = [C.c_void_p] * 4
    L.probe_sample_exponent.restype = C.c_int
    L.probe_sample_exponent.argtypes = [C.c_float]
    L.probe_sample_weight.restype = C.c_uint64
    L.probe_sample_weight.argtypes = [C.c_float, C.c_int]
    L.probe_sample_target.restype = C.c_uint64
    L.probe_sample_target.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
    L.probe_sample_pick.restype = C.c_uint64
    L.probe_sample_pick.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    L.probe_sample_fold.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
    L.probe_sample_point.argtypes = [C.c_void_p] * 3 + [C.c_float, C.c_float, C.c_void_p]
    L.probe_sample_normal.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
    return L


def test_host_generator_matches(probe):
    out = np.zeros(4, U32)
    for counter, key, want in KATS:
        probe.probe_philox(np.array(counter, U32).ctypes.data, np.array(key, U32).ctypes.data, out.ctypes.data)
        assert out.tolist() == list(want)
    rng = np.random.default_rng(1)
    g = np.concatenate([rng.integers(0, 2 ** 63, 200).astype(U64), np.array([0, 2 ** 32 - 1, 2 ** 32, 2 ** 40, 2 ** 64 - 1], U64)])
    for seed in (0, 2 ** 32 + 7, 2 ** 64 - 1):
        want = sm.sample_random(seed, g)
        for k, gk in enumerate(g.tolist()):
            probe.probe_sample_random(seed, gk, out.ctypes.data)
            assert out.tolist() == want[k].tolist(), (seed, gk)


def _area_cases():
    """Triangles [n, 3, 3] over the range in which |n|^2 is an f32 (A_t from 4e-23 to 1.8e19) and beyond both of its ends: random, huge (the
    squares overflow: not finite, counted as 0), tiny (the squares are subnormal, or underflow to 0), degenerate, NaN."""
    rng = np.random.default_rng(2)
    t = rng.uniform(-3, 3, (400, 3, 3)).astype(F)
    scale = np.ones(400, F)
    scale[50:100] = F(5.0e8)         # areas near 1e18
    scale[100:130] = F(3.0e19)       # the squares of n overflow: not finite
    scale[130:180] = F(1.0e-11)      # areas near 1e-22: their squares are subnormal
    scale[180:250] = F(2.0e-22)      # underflow to 0
    t = (t * scale[:, None, None]).astype(F)
    t[250:260, 1] = t[250:260, 0]
    t[260:270, 2] = ((t[260:270, 0] + t[260:270, 1]) * F(0.5)).astype(F)
    t[270:275, 0, 0] = np.nan
    t[275:280, 1, 2] = np.inf
    return np.ascontiguousarray(t)


def test_host_areas_and_weights_match(probe):
    t = _area_cases()
    A, n = sm.tri_area2(t)
    assert (A == 0).sum() >= 100 and (A > 1e17).any() and ((A > 0) & (A < 1e-20)).sum() >= 20
    got_n = np.zeros(3, F)
    for i in range(t.shape[0]):
        got = probe.probe_tri_weight_area(t[i, 0].ctypes.data, t[i, 1].ctypes.data, t[i, 2].ctypes.data, got_n.ctypes.data)
        assert _bits(got) == _bits(A[i]), i
        assert _bits(got_n).tolist() == _bits(n[i]).tolist(), i
    # the exponent and the weights: Amax at both ends of the f32 range, and a subnormal one
    tiny = np.array([1, 2, 3, 2 ** 22, 2 ** 23 - 1], U32).view(F)               # subnormals: 2^-149 ..
    for amax in [F(3.4028235e38), F(2.0 ** 127), F(1.0), F(1.5), F(2.0 ** -126), F(1.17549435e-38)] + tiny.tolist() + A[A > 0][:60].tolist():
        amax = F(amax)
        e = sm.exponent_of(amax)
        assert probe.probe_sample_exponent(amax) == e, amax
        assert 2.0 ** e <= float(amax) < 2.0 ** (e + 1)
        group = np.concatenate([[amax, F(0)], (amax * np.random.default_rng(3).random(20, dtype=F)).astype(F), A[(A > 0) & (A <= amax)][:40]]).astype(F)
        w, e2 = sm.weights(group)
        assert e2 == e and w[0] >= 2 ** 37 and w[0] < 2 ** 38
        for a, wi in zip(group.tolist(), w.tolist()):
            assert probe.probe_sample_weight(a, e) == wi, (amax, a)


def test_host_pick_matches(probe):
    C_ = np.array([5, 5, 5, 9, 9, 20, 20, 20, 21], U64)      # repeated entries = triangles of weight 0
    W = int(C_[-1])
    for T in range(W):
        want = int(sm.pick(C_, np.array([T], U64))[0])
        assert int(probe.probe_sample_pick(C_.ctypes.data, C_.size, T)) == want
        assert C_[want] > T and (want == 0 or C_[want - 1] <= T)
    assert int(probe.probe_sample_pick(C_.ctypes.data, C_.size, 0)) == 0            # the table's first entry
    assert int(probe.probe_sample_pick(C_.ctypes.data, C_.size, 4)) == 0
    assert int(probe.probe_sample_pick(C_.ctypes.data, C_.size, 5)) == 3            # past the repeated entries
    assert int(probe.probe_sample_pick(C_.ctypes.data, C_.size, W - 1)) == 8        # the last
    lead = np.array([0, 0, 7], U64)                                                  # weight 0 in front
    assert int(probe.probe_sample_pick(lead.ctypes.data, 3, 0)) == 2
    rng = np.random.default_rng(4)
    r = rng.integers(0, 2 ** 32, (300, 2)).astype(U64)
    r[:4] = [[0, 0], [0xFFFFFFFF, 0xFFFFFFFF], [0, 0xFFFFFFFF], [0xFFFFFFFF, 0]]
    for W in (1, 21, 2 ** 38 - 1, 2 ** 62 + 12345, 2 ** 63 - 1):
        want = sm.target(r[:, 0], r[:, 1], W)
        assert (want < W).all()
        for k in range(r.shape[0]):
            assert int(probe.probe_sample_target(int(r[k, 0]), int(r[k, 1]), W)) == int(want[k])


def test_host_fold_point_and_normal_match(probe):
    rng = np.random.default_rng(5)
    r = rng.integers(0, 2 ** 32, (500, 2)).astype(U32)
    r[:6] = [[0, 0], [0xFFFFFFFF, 0xFFFFFFFF], [0xFFFFFFFF, 0], [0, 0xFFFFFFFF],
             [(2 ** 22) << 9, ((2 ** 22) - 1) << 9],       # u' + v' = 1 exactly (2^-1 + 2^-24 and 2^-1 - 2^-24): not folded
             [(2 ** 22) << 9, (2 ** 22) << 9]]             # u' + v' = 1 + 2^-23, the smallest sum above 1 (sums are multiples of 2^-23: exact): folded
    u, v = sm.fold(r[:, 0], r[:, 1])
    up, vp = sm.unit(r[:, 0]), sm.unit(r[:, 1])
    assert (up[4] + vp[4]) == F(1) and float(up[4]) + float(vp[4]) == 1.0 and u[4] == up[4]
    assert F(up[5] + vp[5]) == F(1 + 2.0 ** -23) and u[5] == F(1) - up[5] and v[5] == F(1) - vp[5]
    folded = u != up
    assert folded.sum() > 150 and (~folded).sum() > 150
    assert (u > 0).all() and (v > 0).all() and (u.astype(np.float64) + v.astype(np.float64) <= 1 + 2.0 ** -23).all()
    uv = np.zeros(2, F)
    t = _area_cases()[:500 // 5 * 5]
    t = np.concatenate([t[:50], t[50:60], t[130:140], np.random.default_rng(6).uniform(-1e4, 1e4, (430, 3, 3)).astype(F)])
    A, n = sm.tri_area2(t)
    p = sm.point(t[:, 0], t[:, 1], t[:, 2], u, v)
    nu = sm.unit_normal(n, A)
    got = np.zeros(3, F)
    for i in range(500):
        probe.probe_sample_fold(int(r[i, 0]), int(r[i, 1]), uv.ctypes.data)
        assert _bits(uv).tolist() == _bits([u[i], v[i]]).tolist(), i
        probe.probe_sample_point(t[i, 0].ctypes.data, t[i, 1].ctypes.data, t[i, 2].ctypes.data, u[i], v[i], got.ctypes.data)
        assert _bits(got).tolist() == _bits(p[i]).tolist(), i
        if A[i] > 0:
            probe.probe_sample_normal(np.ascontiguousarray(n[i]).ctypes.data, A[i], got.ctypes.data)
            assert _bits(got).tolist() == _bits(nu[i]).tolist(), i


# ---- the library: exports and argument checks that need no device ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


def test_new_entry_points_are_exported(lib):
    for name in ("m2s_sample_surface", "m2s_mesh_sample_surface"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    hdr = open(os.path.join(ROOT, "include", "m2s.h")).read()
    assert "typedef struct m2s_surface_sample_opts" in hdr
    assert "#define M2S_VERSION_MINOR 5" in hdr
    assert C.sizeof(_lib.M2SSurfaceSampleOpts) == 24
    assert lib.m2s_version() == 5


def _opts(**kw):
    o = _lib.M2SOpts()
    o.struct_size = C.sizeof(_lib.M2SOpts)
    o.device = -1
    o.synchronous = 1
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _sopts(struct_size=None, reserved=0, seed=0, first=0):
    return _lib.M2SSurfaceSampleOpts(C.sizeof(_lib.M2SSurfaceSampleOpts) if struct_size is None else struct_size, reserved, seed, first)


def test_bad_arguments_fail_before_the_device(lib):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    idx = np.array([0, 1, 2, 0, 2, 3], np.uint32)
    pt, tri, uv, nrm = np.zeros((4, 3), F), np.zeros(4, np.uint32), np.zeros((4, 2), F), np.zeros((4, 3), F)
    area = C.c_double(-1.0)
    V, I = v.ctypes.data, idx.ctypes.data
    outs = [x.ctypes.data for x in (pt, tri, uv, nrm)] + [C.byref(area)]
    BAD, EMPTY, OK = _lib.ERR_BAD_ARG, _lib.ERR_EMPTY_MESH, _lib.M2S_OK
    ss, ms = lib.m2s_sample_surface, lib.m2s_mesh_sample_surface
    assert ss(V, 4, I, 6, 4, 0, 4, None, None, None, None, None, None, None) == BAD                  # every output NULL, area_out included
    assert "NULL" in _lib.last_error()
    assert ss(V, 4, I, 6, 4, 0, 0, None, None, None, None, None, None, None) == BAD                  # ... also without samples
    assert ss(V, 4, I, 6, 3, 0, 4, None, *outs, None) == BAD                                         # index_bytes
    assert ss(V, 4, I, 6, 4, 7, 4, None, *outs, None) == BAD                                         # topology
    assert ss(None, 4, I, 6, 4, 0, 4, None, *outs, None) == BAD                                      # NULL vertices
    bad_idx = np.array([0, 1, 2, 0, 2, 4], np.uint32)
    assert ss(V, 4, bad_idx.ctypes.data, 6, 4, 0, 4, None, *outs, None) == BAD                       # vertex index out of range
    assert "out of range" in _lib.last_error()
    assert ss(V, 4, bad_idx.ctypes.data, 6, 4, 1, 0, None, *outs, None) == BAD                       # ... as a strip, without samples
    for so in (_sopts(struct_size=8), _sopts(struct_size=32), _sopts(struct_size=0), _sopts(reserved=1),
               _sopts(first=2 ** 64 - 4), _sopts(first=2 ** 64 - 1)):   # first + 4 = 2^64 is the smallest overflow
        assert ss(V, 4, I, 6, 4, 0, 4, C.byref(so), *outs, None) == BAD, (so.struct_size, so.reserved, so.first_sample)
        assert ms(None, 4, C.byref(so), *outs, None) == BAD
    for field, value in (("x_begin", 1), ("x_end", 2), ("x_period", 4), ("n_peer_out", 1), ("mem_kind", 5), ("algorithm", 2)):
        assert ss(V, 4, I, 6, 4, 0, 4, None, *outs, C.byref(_opts(**{field: value}))) == BAD, field
    assert ms(None, 4, None, *outs, None) == BAD                                                      # NULL mesh
    # a mesh without triangles: the area is 0; no samples is fine, samples are M2S_ERR_EMPTY_MESH — no device needed
    for args in ((V, 2, None, 0, 4, 0), (V, 4, I, 2, 4, 0), (V, 4, I, 2, 4, 1), (None, 0, None, 0, 4, 0)):
        area.value = -1.0
        assert ss(*args, 0, None, None, None, None, None, C.byref(area), None) == OK and area.value == 0.0
        area.value = -1.0
        assert ss(*args, 4, C.byref(_sopts(first=2 ** 64 - 5)), *outs, None) == EMPTY and area.value == 0.0     # (first + n = 2^64 - 1: the largest sum that fits)
    assert surface_area(np.zeros((0, 3), F), Topology.TriangleList()) == 0.0
    with pytest.raises(M2SPanic):
        sample_surface(np.zeros((0, 3), F), Topology.TriangleList(), 3)
    with pytest.raises(M2SPanic):
        sample_surface(v, Topology.TriangleList(idx), 3, first_sample=2 ** 64 - 2)


def _compile(tmp_path, cc, std, src, extra=()):
    exe = str(tmp_path / os.path.basename(src).split(".")[0])
    subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                           os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", *extra, "-o", exe])
    return exe


@pytest.mark.parametrize("cc,std,src", [("gcc", "-std=c99", "tests/c/sample_smoke.c"), ("g++", "-std=c++17", "tests/cpp/sample_tests.cpp")])
def test_headers_compile_and_the_early_answers_hold(lib, tmp_path, cc, std, src):
    """The C and C++ headers with the new declarations, from consumers of their own; run without arguments the programs ask only what is
    decided before any device work."""
    if not shutil.which(cc):
        pytest.skip("no " + cc)
    exe = _compile(tmp_path, cc, std, src, ["-lm"] if cc == "gcc" else [])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
