"""m2s_band_csg / m2s_band_export / m2s_band_field_info without a GPU: the exports and the header, every argument check that can be reached
without a handle, the consumers, and the model tests/band_csg_model.py against its own definition: idempotence, A \\ B = A & -B, De Morgan
through the negation, the equal-background consequence against a select on dense grids, and the tie rules."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import band_csg_model as cm
from mesh_to_sdf_amd import BandField, CsgOp, M2SPanic, Mesh, _lib, boolean

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = (cm.UNION, cm.INTERSECTION, cm.DIFFERENCE)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


# ---- 1. exports, header ------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_exported(lib):
    for name in ("m2s_band_csg", "m2s_band_export", "m2s_band_field_info"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    hdr = " ".join(open(os.path.join(ROOT, "include", "m2s.h")).read().split())
    for text in ("enum m2s_csg_op { M2S_CSG_UNION = 0, M2S_CSG_INTERSECTION = 1, M2S_CSG_DIFFERENCE = 2 };",
                 "int m2s_band_csg(const m2s_band* a, const m2s_band* b, int op, const m2s_band_field_opts* fopts /* NULL = the min rule */, "
                 "const m2s_opts* opts, m2s_band** out);",
                 "int m2s_band_export(const m2s_band* band, uint64_t* cells_out, float* distances_out, uint64_t capacity, "
                 "uint32_t* inside_bits_out, const m2s_opts* opts);",
                 "int m2s_band_field_info(const m2s_band* band, m2s_band_field_opts* fopts_out, int* has_inside);",
                 "pickB = (b < a) || (a == b && !actA[L])", "pickB = (b > a) || (a == b && !actA[L])",
                 "A \\ B = INTERSECTION(A, -B)", "NOT the exact distance"):
        assert text in hdr, text
    assert lib.m2s_version() == 5
    assert (int(CsgOp.Union), int(CsgOp.Intersection), int(CsgOp.Difference)) == (0, 1, 2) == (_lib.CSG_UNION, _lib.CSG_INTERSECTION, _lib.CSG_DIFFERENCE)
    for cls, names in ((BandField, ("csg", "union", "intersection", "difference", "__or__", "__and__", "__sub__", "to_band", "isosurface")),
                       (Mesh, ("boolean",))):
        for name in names:
            assert hasattr(cls, name), (cls, name)
    assert callable(boolean)
    hpp = open(os.path.join(ROOT, "include", "mesh_to_sdf.hpp")).read()
    for text in ("enum class CsgOp", "BandField csg(", "export_band("):
        assert text in hpp, text


# ---- 2. argument checks that need no handle ------------------------------------------------------------------------------------------------
def test_the_calls_reject_what_needs_no_handle(lib):
    BAD = _lib.ERR_BAD_ARG
    SENTINEL = 0x1234
    fake = C.c_void_p(SENTINEL)                   # never dereferenced: every call below fails before it looks at a handle
    for a, b in ((None, None), (None, fake), (fake, None)):
        for op in (0, 1, 2):
            h = C.c_void_p(SENTINEL)
            assert lib.m2s_band_csg(a, b, op, None, None, C.byref(h)) == BAD
            assert "band is NULL" in _lib.last_error() and h.value is None     # *out = NULL on every failure
    assert lib.m2s_band_csg(None, None, 0, None, None, None) == BAD
    assert "out is NULL" in _lib.last_error()
    for op in (-1, 3, 7):
        h = C.c_void_p(SENTINEL)
        assert lib.m2s_band_csg(None, None, op, None, None, C.byref(h)) == BAD
        assert "m2s_csg_op" in _lib.last_error() and h.value is None
    cells, d, bits = np.zeros(4, np.uint64), np.zeros(4, F), np.zeros(4, np.uint32)
    assert lib.m2s_band_export(None, None, None, 4, None, None) == BAD
    assert "no output" in _lib.last_error()
    assert lib.m2s_band_export(None, cells.ctypes.data, d.ctypes.data, 4, bits.ctypes.data, None) == BAD
    assert "band is NULL" in _lib.last_error()
    fo, has = _lib.M2SBandFieldOpts(), C.c_int(7)
    assert lib.m2s_band_field_info(None, C.byref(fo), C.byref(has)) == BAD and has.value == 7
    assert lib.m2s_band_field_info(None, None, None) == BAD


def test_python_checks_its_own_arguments():
    from mesh_to_sdf_amd.api import _csg_op

    assert _csg_op("union") is CsgOp.Union and _csg_op("Difference") is CsgOp.Difference and _csg_op(1) is CsgOp.Intersection
    assert _csg_op(CsgOp.Difference) is CsgOp.Difference
    for bad in ("xor", 3, -1, None, 0.5j):
        with pytest.raises(M2SPanic):
            _csg_op(bad)


# ---- 3. the consumers compile -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cc,std,src", [("gcc", "-std=c99", "tests/c/band_csg_smoke.c"), ("g++", "-std=c++17", "tests/cpp/band_csg_tests.cpp")])
def test_consumers_compile_and_check_their_arguments(lib, tmp_path, cc, std, src):
    exe = str(tmp_path / os.path.basename(src).split(".")[0])
    subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                           os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


# ---- 4. the model -----------------------------------------------------------------------------------------------------------------------------------
SPECIAL = np.array([0.0, -0.0, 0.5, -0.5, 0.75, -0.75, np.finfo(F).max, -np.finfo(F).max], F)


def random_band(rng, shape, density=0.5, bits=True, bg=(0.75, 0.5), special=0.3):
    """A random active set with random finite values, a share of them from SPECIAL (zeros of both signs, the backgrounds, +-f32::MAX)."""
    total = shape[0] * shape[1] * shape[2]
    cells = np.flatnonzero(rng.random(total) < density)
    d = rng.uniform(-1, 1, cells.size).astype(F)
    pick = rng.random(cells.size) < special
    d[pick] = rng.choice(SPECIAL, int(pick.sum()))
    mask = rng.integers(0, 2 ** 32, (shape[0], shape[1], (shape[2] + 31) // 32), dtype=np.uint64).astype(np.uint32) if bits else None
    return cm.Band(shape, cells, d, mask, *bg)


def same_dense(x, y):
    (ax, dx, sx), (ay, dy, sy) = cm.dense(x), cm.dense(y)
    return np.array_equal(ax, ay) and np.array_equal(dx.view(np.uint32), dy.view(np.uint32)) and np.array_equal(sx, sy)


@pytest.mark.parametrize("shape", [(5, 6, 7), (2, 3, 33), (1, 1, 65)], ids=lambda n: "x".join(map(str, n)))
def test_a_band_with_itself_is_itself(shape):
    rng = np.random.default_rng(31)
    for bits in (True, False):
        a = random_band(rng, shape, bits=bits)
        for op in (cm.UNION, cm.INTERSECTION):
            r = cm.csg(a, a, op)
            assert same_dense(r, a)
            assert np.array_equal(r.cells, a.cells) and np.array_equal(r.distances.view(np.uint32), a.distances.view(np.uint32))
            # the result's mask is s on every point: the band's own bit where it is inactive, the value's sign where it is active
            assert np.array_equal(cm.unpack_bits(shape, r.bits), cm.dense(a)[2])


@pytest.mark.parametrize("shape", [(5, 6, 7), (3, 2, 67)], ids=lambda n: "x".join(map(str, n)))
def test_difference_is_intersection_with_the_negation_and_de_morgan_holds(shape):
    rng = np.random.default_rng(32)
    for bits_a, bits_b in ((True, True), (True, False), (False, True)):
        a, b = random_band(rng, shape, bits=bits_a), random_band(rng, shape, 0.4, bits=bits_b, bg=(0.5, 0.25))
        assert cm.same(cm.csg(a, b, cm.DIFFERENCE), cm.csg(a, cm.negate(b), cm.INTERSECTION))
        nb = cm.negate(b)
        assert np.array_equal(cm.dense(nb)[1].view(np.uint32), (-cm.dense(b)[1]).view(np.uint32))          # D'_{-B} = -D'_B, zeros included
        assert (nb.bg_out, nb.bg_in) == (b.bg_in, b.bg_out)
        assert same_dense(cm.negate(nb), b)
        # -(A | B) = -A & -B and -(A & B) = -A | -B, as grids: act, D' to the bit, s
        assert same_dense(cm.negate(cm.csg(a, b, cm.UNION)), cm.csg(cm.negate(a), nb, cm.INTERSECTION))
        assert same_dense(cm.negate(cm.csg(a, b, cm.INTERSECTION)), cm.csg(cm.negate(a), nb, cm.UNION))


@pytest.mark.parametrize("shape", [(5, 6, 7), (2, 3, 33), (1, 1, 64)], ids=lambda n: "x".join(map(str, n)))
def test_with_equal_backgrounds_the_result_stands_for_op_of_the_dense_grids(shape):
    rng = np.random.default_rng(33)
    for bits_a, bits_b in ((True, True), (True, False), (False, False)):
        a, b = random_band(rng, shape, bits=bits_a, bg=(0.75, 0.75)), random_band(rng, shape, 0.3, bits=bits_b, bg=(0.75, 0.75))
        (act_a, da, _), (_, db, _) = cm.dense(a), cm.dense(b)
        for op in OPS:
            r = cm.csg(a, b, op)
            assert (r.bg_out, r.bg_in) == (F(0.75), F(0.75))
            bb = -db if op == cm.DIFFERENCE else db
            want = np.where(bb < da, bb, da) if op == cm.UNION else np.where(bb > da, bb, da)
            got = cm.dense(r)[1]
            assert np.array_equal(got, want)                                           # as numbers everywhere (-0 == +0)
            # ... and to the bit, with the tie rule: an inactive A hands a tie to B
            want = cm.select(cm.UNION if op == cm.UNION else cm.INTERSECTION, da, bb, act_a)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_the_tie_rules():
    shape = (1, 1, 8)
    z, nz_ = F(0.0), F(-0.0)
    # point: 0 both active +0 / -0; 1 the reverse; 2 only B active, a tie with A's background; 3 only A active, a tie with B's background;
    # 4 both inactive (equal backgrounds); 5 both active, equal values; 6 only B active at A's inside background; 7 both inactive, A inside
    a = cm.Band(shape, [0, 1, 3, 5], [z, nz_, 0.5, 0.25], np.array([0b11000000], np.uint32), 0.5, 0.5)
    b = cm.Band(shape, [0, 1, 2, 5, 6], [nz_, z, 0.5, 0.25, -0.5], None, 0.5, 0.5)
    for op in (cm.UNION, cm.INTERSECTION):
        r = cm.csg(a, b, op)
        act, d, s = cm.dense(r)
        act, d, s = act.reshape(-1), d.reshape(-1), s.reshape(-1)
        assert np.signbit(d[0]) == np.signbit(z) and np.signbit(d[1]) == np.signbit(nz_)           # a tie between two active operands: A's bits
        assert act[0] and act[1] and act[2] and act[3] and not act[4] and act[5]
        assert d[2] == F(0.5) and d[3] == F(0.5) and d[4] == F(0.5)
        assert list(np.searchsorted(r.cells, [2, 3])) == [2, 3]
        if op == cm.UNION:
            assert act[6] and d[6] == F(-0.5) and s[6]                  # a tie at -0.5: the active B supplies it; inside either way
            assert not act[7] and d[7] == F(-0.5) and s[7]              # min(-0.5, 0.5): A's background, inactive
        else:
            assert act[6] and d[6] == F(-0.5) and s[6]                  # the same tie: B supplies it, and both are inside there
            assert not act[7] and d[7] == F(0.5) and not s[7]           # max(-0.5, 0.5): B's background, outside
    # zero backgrounds: +0 outside, -0 inside, and their tie with an active zero goes to the active operand
    a = cm.Band(shape, [0], [nz_], None, 0.0, 0.0)
    b = cm.Band(shape, [1], [z], np.array([0b1], np.uint32), 0.0, 0.0)
    r = cm.csg(a, b, cm.UNION)
    assert list(r.cells) == [0, 1] and np.signbit(r.distances[0]) and not np.signbit(r.distances[1])
    assert np.signbit(cm.dense(b)[1].reshape(-1)[0]) and not np.signbit(cm.dense(b)[1].reshape(-1)[2])
    d = cm.csg(a, b, cm.DIFFERENCE)
    # -B: its values and backgrounds with the sign bit flipped, so point 0 is a tie of -0 (A, active) with +0 (-B's outside): A's bits
    assert 0 in d.cells and np.signbit(d.distances[list(d.cells).index(0)])


def test_the_min_rule_and_an_explicit_background():
    rng = np.random.default_rng(34)
    a, b = random_band(rng, (3, 4, 5), bg=(0.75, 0.25)), random_band(rng, (3, 4, 5), bg=(0.5, 0.375))
    u, d = cm.csg(a, b, cm.UNION), cm.csg(a, b, cm.DIFFERENCE)
    assert (u.bg_out, u.bg_in) == (F(0.5), F(0.25))
    assert (d.bg_out, d.bg_in) == (F(0.375), F(0.25))                   # -B: outside 0.375, inside 0.5
    e = cm.csg(a, b, cm.UNION, (0.125, 2.0))
    assert (e.bg_out, e.bg_in) == (F(0.125), F(2.0)) and np.array_equal(e.cells, u.cells)
    # with the min rule the result is no farther from zero than op of the grids on the inactive cells
    for op, r in ((cm.UNION, u), (cm.DIFFERENCE, d)):
        act, dr, _ = cm.dense(r)
        da, db = cm.dense(a)[1], cm.dense(b)[1]
        want = np.minimum(da, db) if op == cm.UNION else np.maximum(da, -db)
        assert (np.abs(dr[~act]) <= np.abs(want[~act])).all() and (np.sign(dr[~act]) == np.sign(want[~act])).all()
