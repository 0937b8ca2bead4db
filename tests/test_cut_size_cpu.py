"""k_cut's size test (csrc/cut_size.hip.h cut_small_enough, built for the host into the CPU probe library): the maximum of the node's two
wave-uniform extents is formed from their bit patterns where both are non-negative numbers, by fmaxf otherwise.  Its decision must equal
fmaxf(R, half) <= e — fmaxf drops a NaN operand, NaN compares false — for every bit pattern of the three arguments."""
import ctypes as C
import os

import numpy as np
import pytest

from mesh_to_sdf_amd import _lib

PROBE = os.path.join(os.path.dirname(_lib.SO_PATH), "libm2s_probe.so")
F = np.float32


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        pytest.fail(f"{PROBE} missing: run __graft_entry__.build()")
    L = C.CDLL(PROBE)
    L.probe_cut_small_enough.restype = C.c_int
    L.probe_cut_small_enough.argtypes = [C.c_float, C.c_float, C.c_float]
    L.probe_cut_small_enough_n.restype = None
    L.probe_cut_small_enough_n.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def bits(*patterns):
    return np.array(patterns, np.uint32).view(F)


# +-0, the smallest and largest denormals, the smallest normal, 1, values around it, large values, the largest finite, +-inf, quiet and
# signalling NaNs of both signs, negative values
SPECIAL = np.concatenate([
    bits(0x00000000, 0x80000000, 0x00000001, 0x007fffff, 0x80000001, 0x807fffff, 0x00800000, 0x80800000),
    np.array([1.0, -1.0, 0.99999994, 1.0000001, 0.5, 2.0, 3.0e-3, 1.0e10, 3.0e37, 3.4028235e38, -3.4028235e38, -2.5, -1.0e-30, -1.0e10], F),
    bits(0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7fc00001, 0xffffffff, 0x7f800001, 0xff800001, 0x7fbfffff),
])


def want(R, half, e):
    with np.errstate(invalid="ignore"):
        return np.fmax(R, half) <= e          # np.fmax: the other operand where one is NaN, NaN for two


def got(probe, R, half, e):
    R, half, e = (np.ascontiguousarray(a, F) for a in (R, half, e))
    out = np.empty(R.size, np.uint8)
    probe.probe_cut_small_enough_n(R.size, R.ctypes.data, half.ctypes.data, e.ctypes.data, out.ctypes.data)
    return out.astype(bool)


def assert_equal_decisions(probe, R, half, e):
    g, w = got(probe, R, half, e), want(R, half, e)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (f"{bad.size} of {w.size} decisions differ; first: R {R[bad[0]]!r} ({R[bad[:1]].view(np.uint32)[0]:#010x}), "
                           f"half {half[bad[0]]!r} ({half[bad[:1]].view(np.uint32)[0]:#010x}), e {e[bad[0]]!r} ({e[bad[:1]].view(np.uint32)[0]:#010x}): "
                           f"helper {bool(g[bad[0]])}, fmaxf {bool(w[bad[0]])}")


def test_cross_product_of_the_special_values(probe):
    R, half, e = (a.ravel() for a in np.meshgrid(SPECIAL, SPECIAL, SPECIAL, indexing="ij"))
    assert R.size == SPECIAL.size ** 3 and SPECIAL.size >= 30
    assert_equal_decisions(probe, R, half, e)
    w = want(R, half, e)
    assert w.any() and not w.all()


def test_random_bit_patterns(probe):
    rng = np.random.default_rng(20261019)
    R, half, e = (rng.integers(0, 1 << 32, 100000, dtype=np.uint64).astype(np.uint32).view(F) for _ in range(3))
    assert_equal_decisions(probe, R, half, e)
    # random patterns against every special value in each position, and the decision at equality
    for k in range(3):
        args = [R.copy(), half.copy(), e.copy()]
        args[k] = np.resize(SPECIAL, R.size)
        assert_equal_decisions(probe, *args)
    assert_equal_decisions(probe, R, half, np.fmax(R, half))
    assert_equal_decisions(probe, np.abs(R), np.abs(half), np.abs(e))     # the kernel's own regime: nothing negative


def test_scalar_entry_point_agrees(probe):
    for R, half, e in [(1.0, 2.0, 2.0), (1.0, 2.0, 1.5), (float("nan"), 2.0, 2.0), (float("nan"), float("nan"), float("inf")), (-0.0, 0.0, 0.0),
                       (float("inf"), 1.0, float("inf")), (-1.0, float("nan"), -1.0)]:
        assert bool(probe.probe_cut_small_enough(R, half, e)) == bool(want(F(R), F(half), F(e))), (R, half, e)


@pytest.mark.parametrize("knob", ["M2S_CUT_WAVE_CAP", "M2S_CUT_COARSE_CAP"])
def test_visit_caps_stay_below_the_removed_budget(knob):
    """k_cut no longer counts the nodes a brick has opened against a budget of 100 000: a wave's visit cap of at most 99 999 always came first.
    The knobs that set the caps are clamped so that this holds for every setting a caller can make."""
    for asked, want in [(40, 40), (99999, 99999), (100000, 99999), (4000000000, 99999), (0, 0)]:
        with _lib.knobs(**{knob: asked}):
            assert int(_lib.describe_knobs()[knob]) == want, (knob, asked)
    assert int(_lib.describe_knobs()[knob]) == 0
