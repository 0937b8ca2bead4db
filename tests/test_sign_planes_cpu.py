"""The index arithmetic of the ray-cast sign planes (csrc/sign.hip.h, built for the host into the CPU probe library), with no device.

axis_range turns one axis of a triangle's padded box into a range of grid lines; the marking kernels then run the exact test on every line
of the range, so a range that drops a line whose centre lies in the box flips the sign of a stripe of cells, while a range that is too wide
only costs time.  Hence two checks against the f32 centres the kernels themselves form (probe_sign_centre, compared in float64):

* conservative, no tolerance: every i < n whose centre lies in the closed [bmn, bmx] is in [lo, hi];
* tight: where max(|bmn|, |bmx|, |first|) / |cs| <= 2^16 the widening of axis_range is below one index — |i0|, |i1| <= 2^17, so
  tol <= 1e-3 + 4e-6 * 2^17 + 1e-6 * 3 * 2^16 = 0.72, the quotients' own rounding (a few ulps of 2^17: under 0.1) and the centres' rounding
  (an ulp of 2^17 cells: 0.008) stay under the rest — so [lo, hi] exceeds the hull of those i by at most one index at either end, and where
  there is no such i it holds at most two indices.  The observed maximum is printed.

Then the windows (free axes, emptiness, slab clipping), x_in_slab against a list comprehension, the bucket of a hit against a numpy-f32
model of the reference's `floor(t / cs) as usize .min(n - 1)`, and the path a call takes at every threshold."""
import ctypes as C
import os

import numpy as np
import pytest

from mesh_to_sdf_amd import _lib

PROBE = os.path.join(os.path.dirname(_lib.SO_PATH), "libm2s_probe.so")
F = np.float32
U32 = np.uint32
ENUMERATE_BELOW = 1 << 18          # lines of an axis whose centres are all looked at; longer axes are sampled around every place of interest


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        pytest.fail(f"{PROBE} missing: run __graft_entry__.build()")
    L = C.CDLL(PROBE)
    L.probe_sign_centre.restype = C.c_float
    L.probe_sign_centre.argtypes = [C.c_float, C.c_float, C.c_uint32]
    L.probe_sign_centres_n.restype = None
    L.probe_sign_centres_n.argtypes = [C.c_float, C.c_float, C.c_size_t, C.c_void_p, C.c_void_p]
    L.probe_sign_axis_range.restype = None
    L.probe_sign_axis_range.argtypes = [C.c_float] * 4 + [C.c_uint32, C.c_void_p]
    L.probe_sign_window.restype = C.c_uint32
    L.probe_sign_window.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
    L.probe_sign_x_in_slab.restype = None
    L.probe_sign_x_in_slab.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.probe_sign_bucket.restype = C.c_uint32
    L.probe_sign_bucket.argtypes = [C.c_float, C.c_float, C.c_uint32]
    L.probe_sign_path.restype = None
    L.probe_sign_path.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.probe_tri_box.restype = None
    L.probe_tri_box.argtypes = [C.c_void_p] * 5
    return L


# ---- axis_range ---------------------------------------------------------------------------------------------------------------------------
def centres(probe, first, cs, idx):
    idx = np.ascontiguousarray(idx, U32)
    out = np.empty(idx.size, F)
    probe.probe_sign_centres_n(F(first), F(cs), idx.size, idx.ctypes.data, out.ctypes.data)
    return out.astype(np.float64)


def axis_range(probe, bmn, bmx, first, cs, n):
    out = np.zeros(2, U32)
    probe.probe_sign_axis_range(F(bmn), F(bmx), F(first), F(cs), int(n), out.ctypes.data)
    return int(out[0]), int(out[1])


def indices_to_look_at(bmn, bmx, first, cs, n):
    """All of them, or (long axes) both ends and +-64 around where either bound falls, in float64."""
    if n <= ENUMERATE_BELOW:
        return np.arange(n, dtype=np.int64), True
    spots = [0, n - 1]
    with np.errstate(all="ignore"):
        for b in (bmn, bmx):
            q = (np.float64(b) - np.float64(first)) / np.float64(cs)
            if np.isfinite(q):
                spots.append(int(min(max(q, 0), n - 1)))
    idx = np.unique(np.clip(np.concatenate([np.arange(s - 64, s + 65, dtype=np.int64) for s in spots]), 0, n - 1))
    return idx, False


def check_box(probe, bmn, bmx, first, cs, n):
    """Conservative always; returns the excess of [lo, hi] over the hull of the truth where the tight bound applies (else None)."""
    bmn, bmx, first, cs = F(bmn), F(bmx), F(first), F(cs)
    what = f"bmn={bmn!r} bmx={bmx!r} first={first!r} cs={cs!r} n={n}"
    lo, hi = axis_range(probe, bmn, bmx, first, cs, n)
    assert (lo <= hi < n) or (lo, hi) == (1, 0), f"{what}: [{lo}, {hi}] is neither a range of the axis nor the empty one"
    idx, complete = indices_to_look_at(bmn, bmx, first, cs, n)
    c = centres(probe, first, cs, idx)
    truth = idx[(c >= np.float64(bmn)) & (c <= np.float64(bmx))]
    missed = truth[(truth < lo) | (truth > hi)]
    assert missed.size == 0, f"{what}: [{lo}, {hi}] drops the lines {missed[:5].tolist()} whose centres lie in the box"
    with np.errstate(all="ignore"):
        ratio = np.abs(np.array([bmn, bmx, first], np.float64)).max() / np.float64(abs(cs))          # NaN where any of them is
        small = bool(ratio <= 2.0 ** 16)
    if not (complete and small):
        return None
    if lo > hi:
        return 0
    if truth.size == 0:
        assert hi - lo + 1 <= 2, f"{what}: no centre lies in the box, [{lo}, {hi}] holds more than two lines"
        return hi - lo + 1
    excess = max(int(truth.min()) - lo, hi - int(truth.max()))
    assert excess <= 1, f"{what}: [{lo}, {hi}] against the hull [{truth.min()}, {truth.max()}]"
    return excess


def test_random_boxes_conservative_and_tight(probe, capsys):
    rng = np.random.default_rng(20261)
    worst, tight = 0, 0
    for _ in range(4000):
        n = int(rng.choice([1, 2, 7, 64, 100, 513, 4099]))
        cs = F(rng.choice([-1, 1]) * 10.0 ** rng.uniform(-3, 3))
        first = F(rng.normal() * abs(cs) * 10.0 ** rng.uniform(0, 4))
        span = abs(np.float64(cs)) * n
        a = np.float64(first) + (np.float64(cs) * n / 2) + rng.normal() * span
        w = span * 10.0 ** rng.uniform(-4, 0.5) * rng.choice([0, 1, 1, 1])
        e = check_box(probe, a - w / 2, a + w / 2, first, cs, n)
        if e is not None:
            worst, tight = max(worst, e), tight + 1
    assert tight > 2000, tight
    with capsys.disabled():
        print(f"\n[sign axis_range] random boxes: largest excess over the hull {worst} index (bound 1), {tight} tight cases")


def on_a_centre_cases(probe):
    """Bounds exactly on a centre (or an ulp beside it), 1e3, 1e4 and 1e5 cells from the origin of the axis, for cell sizes no f32 holds
    exactly, negative ones and very small and large ones: where the rounding of (b - first) / cs decides whether a line is dropped."""
    rng = np.random.default_rng(20262)
    for cs in (0.01, 0.1, 0.3, -0.01, -0.7, 1.0 / 3.0, 1.0e-6, 1.0e6, -1.0e-6, 3.1e6):
        for first in (0.0, 0.1 * cs, -0.37 * cs, 12.3 * cs, -977.1 * cs):
            for off in (1000, 10000, 100000):
                for j in np.concatenate([[off], off + rng.integers(-900, 900, 5)]):
                    j = int(j)
                    n = j + int(rng.integers(1, 40))
                    c = F(centres(probe, first, cs, [j])[0])
                    for d_lo, d_hi in ((0, 0), (0, 3), (-2, 0), (-5, 4)):          # bmn == bmx on the centre; then the centre as either bound
                        a = F(centres(probe, first, cs, [max(j + d_lo, 0)])[0]) if d_lo else c
                        b = F(centres(probe, first, cs, [min(j + d_hi, n - 1)])[0]) if d_hi else c
                        yield min(a, b), max(a, b), first, cs, n
                    yield np.nextafter(c, F(-np.inf)), np.nextafter(c, F(np.inf)), first, cs, n
    # the grid's origin itself far from zero: the centres are coarse there, in the last case so coarse that neighbouring lines share one
    for first, cs in ((1000.0, 0.01), (-2.0e4, 0.013), (1.0e5, 0.3), (-1.0e5, -0.3), (1.0e5, 0.01)):
        for j in (0, 1, 17, 511):
            c = F(centres(probe, first, cs, [j])[0])
            yield c, c, first, cs, 512
            yield c, F(centres(probe, first, cs, [min(j + 9, 511)])[0]), first, cs, 512


def test_bounds_on_a_centre_far_from_the_origin(probe, capsys):
    worst, cases, tight = 0, 0, 0
    for bmn, bmx, first, cs, n in on_a_centre_cases(probe):
        if bmn > bmx:
            bmn, bmx = bmx, bmn
        e = check_box(probe, bmn, bmx, first, cs, n)
        cases += 1
        if e is not None:
            worst, tight = max(worst, e), tight + 1
    assert cases > 4000 and tight > 1000, (cases, tight)
    with capsys.disabled():
        print(f"\n[sign axis_range] bounds on a centre: largest excess over the hull {worst} index (bound 1), {tight} tight of {cases} cases")


@pytest.mark.parametrize("cs", [0.25, -0.25, 1.0e-6, 1.0e6, 3.0, -1.0e-6])
def test_boxes_before_after_around_the_grid_and_single_lines(probe, cs):
    for n in (1, 2, 33):
        first = F(-0.4 * cs)
        c = centres(probe, first, cs, np.arange(n))
        lo_c, hi_c, step = c.min(), c.max(), abs(np.float64(F(cs)))
        boxes = [(lo_c - 9 * step, lo_c - 2 * step), (hi_c + 2 * step, hi_c + 7 * step), (lo_c - 5 * step, hi_c + 5 * step),
                 (lo_c - 3 * step, lo_c), (hi_c, hi_c + 3 * step), (lo_c, hi_c), (lo_c, lo_c), (hi_c, hi_c),
                 (lo_c - 0.4 * step, lo_c - 0.3 * step), (hi_c + 0.3 * step, hi_c + 0.4 * step), (lo_c + 0.3 * step, lo_c + 0.4 * step)]
        for a, b in boxes:
            check_box(probe, a, b, first, cs, n)
        # wholly before and wholly after: empty, not a clamped line
        assert axis_range(probe, lo_c - 9 * step, lo_c - 2 * step, first, cs, n) == (1, 0)
        assert axis_range(probe, hi_c + 2 * step, hi_c + 7 * step, first, cs, n) == (1, 0)
        assert axis_range(probe, lo_c - 5 * step, hi_c + 5 * step, first, cs, n) == (0, n - 1)


def test_anisotropic_axes_are_independent(probe):
    """One box over three axes of very different cell sizes: each axis' range depends on its own first / cs / n alone."""
    first, cs, n = (F(-1.0), F(20.0), F(1.0e-3)), (F(0.002), F(-7.0), F(1.0e-6)), (1000, 9, 4000)
    for m in range(3):
        a, b = sorted((np.float64(first[m]) + 0.31 * np.float64(cs[m]) * n[m], np.float64(first[m]) + 0.62 * np.float64(cs[m]) * n[m]))
        e = check_box(probe, a, b, first[m], cs[m], n[m])
        assert e is not None and e <= 1
        lo, hi = axis_range(probe, a, b, first[m], cs[m], n[m])
        assert abs(lo - 0.31 * n[m]) <= 2 and abs(hi - 0.62 * n[m]) <= 2, (m, lo, hi)


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("n", [1, 5, 4097, 2 ** 31 + 3, 2 ** 32 - 1])
def test_non_finite_bounds_and_overflowing_indices_give_the_whole_range(probe, n):
    whole = (0, n - 1)
    for bmn, bmx in ((NAN, 1.0), (0.0, NAN), (NAN, NAN), (-INF, INF), (-INF, 0.5), (0.5, INF), (INF, INF), (-INF, -INF)):
        for first, cs in ((0.0, 1.0), (-3.5, -0.01), (1.0e30, 1.0e-3)):
            assert axis_range(probe, bmn, bmx, first, cs, n) == whole, (bmn, bmx, first, cs)
    # finite bounds whose index is not: the difference overflows, the quotient overflows, the cell size is zero or not a number
    for bmn, bmx, first, cs in ((-3.0e38, 0.0, 3.0e38, 1.0), (0.0, 3.0e38, -3.0e38, -1.0), (-1.0, 1.0e10, 0.0, 1.0e-30), (-1.0e10, 1.0, 0.0, -1.0e-30),
                                (-1.0, 1.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0), (-1.0, 1.0, 0.0, NAN), (-1.0, 1.0, NAN, 1.0), (-1.0, 1.0, INF, 1.0),
                                (-1.0, 1.0, 0.0, 1.0e-45), (1.0, 2.0, 0.0, -1.0e-45)):
        assert axis_range(probe, bmn, bmx, first, cs, n) == whole, (bmn, bmx, first, cs)
        check_box(probe, bmn, bmx, first, cs, n)


def test_indices_beyond_2_31_do_not_wrap(probe):
    """(uint32_t) of a float at or above 2^32, or below 0, is not defined and wraps on the hardware: the range must be empty or clamped."""
    two31, two32 = 2.0 ** 31, 2.0 ** 32
    for n in (1, 100, 4097):
        assert axis_range(probe, 3.0e9, 3.5e9, 0.0, 1.0, n) == (1, 0)            # both indices past the axis, above 2^31
        assert axis_range(probe, 5.0e9, 6.0e9, 0.0, 1.0, n) == (1, 0)            # above 2^32
        assert axis_range(probe, 1.0e30, 2.0e30, 0.0, 1.0, n) == (1, 0)
        assert axis_range(probe, -3.5e9, -3.0e9, 0.0, 1.0, n) == (1, 0)          # below -2^31
        assert axis_range(probe, -3.0e9, 3.0e9, 0.0, 1.0, n) == (0, n - 1)
        assert axis_range(probe, -1.0e30, 5.0e9, 0.0, 1.0, n) == (0, n - 1)
        assert axis_range(probe, 3.0e9, 3.5e9, 0.0, -1.0, n) == (1, 0)           # negative cell size: the indices are -3.5e9 .. -3e9
        assert axis_range(probe, -3.5e3, -3.0e3, 0.0, -1.0e-6, n) == (1, 0)      # +3e9 .. 3.5e9 through a tiny negative cell size
        assert axis_range(probe, -1.0, 3.0e3, 0.0, 1.0e-6, n) == (0, n - 1)
        for args in ((3.0e9, 3.5e9, 0.0, 1.0), (-3.0e9, 3.0e9, 0.0, 1.0), (-1.0, 3.0e3, 0.0, 1.0e-6), (2.0, 3.0e9, 0.0, 1.0)):
            check_box(probe, *args, n)
    for n in (2 ** 31 + 3, 2 ** 32 - 1):                                         # axes that long: the indices themselves pass 2^31
        assert axis_range(probe, -5.0, 5.0e9, 0.0, 1.0, n) == (0, n - 1)
        assert axis_range(probe, 5.0e9, 6.0e9, 0.0, 1.0, n) == (1, 0)
        assert axis_range(probe, -7.0, -3.0, 0.0, 1.0, n) == (1, 0)
        lo, hi = axis_range(probe, two31 - 1000.0, two31 + 1024.0, 0.0, 1.0, n)
        assert two31 - 20000 <= lo <= two31 - 1000 and min(two31 + 1024, n - 1) <= hi <= min(two31 + 20000, n - 1), (lo, hi)
        check_box(probe, two31 - 1000.0, two31 + 1024.0, 0.0, 1.0, n)
        check_box(probe, two31 - 1000.0, 1.0e10, 0.0, 1.0, n)
        check_box(probe, -1.0, 17.0, 0.0, 1.0, n)
    lo, hi = axis_range(probe, 4.0e9, 4.2e9, 0.0, 1.0, 2 ** 32 - 1)
    assert 3.99e9 <= lo <= 4.0e9 and 4.2e9 <= hi <= 4.21e9 and hi < two32, (lo, hi)
    check_box(probe, 4.0e9, 4.2e9, 0.0, 1.0, 2 ** 32 - 1)
    check_box(probe, 4.29e9, 4.2949673e9, 0.0, 1.0, 2 ** 32 - 1)                  # up to the last index: h >= (float)(n - 1) clamps


# ---- windows --------------------------------------------------------------------------------------------------------------------------------
WHOLE = (0, 0, 31, 0, 1)            # lo, hi, chunk_log, period, all
FREE = {0: (1, 2), 1: (0, 2), 2: (0, 1)}          # line axis -> its two free axes (U, W)


def window(probe, tri, first, size, n, slab, axis):
    tri, first, size = (np.ascontiguousarray(a, F).reshape(-1) for a in (tri, first, size))
    n, slab = np.ascontiguousarray(n, U32), np.ascontiguousarray(slab, U32)
    out = np.zeros(4, U32)
    cnt = probe.probe_sign_window(tri.ctypes.data, first.ctypes.data, size.ctypes.data, n.ctypes.data, slab.ctypes.data, axis, out.ctypes.data)
    return tuple(int(x) for x in out), int(cnt)


def tri_box(probe, tri):
    tri = np.ascontiguousarray(tri, F).reshape(3, 3)
    mn, mx = np.zeros(3, F), np.zeros(3, F)
    probe.probe_tri_box(tri[0].ctypes.data, tri[1].ctypes.data, tri[2].ctypes.data, mn.ctypes.data, mx.ctypes.data)
    return mn, mx


GRID = (np.array([-1.0, -2.0, 0.5], F), np.array([0.05, 0.11, -0.02], F), np.array([61, 37, 83], U32))     # every axis its own first / size / n


def test_window_uses_the_two_free_axes(probe):
    first, size, n = GRID
    rng = np.random.default_rng(7)
    seen_non_empty = 0
    for _ in range(300):
        centre = first + size * n * rng.uniform(0.1, 0.9, 3).astype(F)
        tri = (centre + rng.normal(0, 1, (3, 3)).astype(F) * np.abs(size) * rng.uniform(0.5, 12)).astype(F)
        mn, mx = tri_box(probe, tri)
        per_axis = [axis_range(probe, mn[m], mx[m], first[m], size[m], n[m]) for m in range(3)]
        for axis in range(3):
            u, w = FREE[axis]
            (ulo, uhi, wlo, whi), cnt = window(probe, tri, first, size, n, WHOLE, axis)
            if per_axis[u][0] > per_axis[u][1] or per_axis[w][0] > per_axis[w][1]:
                assert cnt == 0 and ulo > uhi
            else:
                assert (ulo, uhi) == per_axis[u] and (wlo, whi) == per_axis[w], (axis, per_axis)
                assert cnt == (uhi - ulo + 1) * (whi - wlo + 1) > 0
                seen_non_empty += 1
    assert seen_non_empty > 600


def test_an_empty_range_on_either_free_axis_empties_the_window(probe):
    first, size, n = GRID
    inside = first + size * n * F(0.5)
    for out_axis in range(3):
        for sign in (-1, 1):
            centre = inside.copy()
            centre[out_axis] = first[out_axis] + size[out_axis] * n[out_axis] * (0.5 + sign * 0.8)       # well past that face of the grid
            tri = (centre + np.array([[0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1]], F)).astype(F)
            mn, mx = tri_box(probe, tri)
            assert axis_range(probe, mn[out_axis], mx[out_axis], first[out_axis], size[out_axis], n[out_axis]) == (1, 0)
            for axis in range(3):
                _, cnt = window(probe, tri, first, size, n, WHOLE, axis)
                assert (cnt == 0) == (out_axis in FREE[axis]), (out_axis, axis, cnt)


def test_slab_clips_the_y_and_z_lines_only(probe):
    first, size, n = GRID
    tri = (first + size * n * np.array([[0.1, 0.2, 0.3], [0.9, 0.25, 0.5], [0.5, 0.8, 0.7]], F)).astype(F)       # x range about 6 .. 54
    whole = [window(probe, tri, first, size, n, WHOLE, axis) for axis in range(3)]
    assert whole[1][0][0] < 10 and whole[1][0][1] > 50
    for slab in ((20, 33, 31, 0, 0), (20, 33, 31, 1, 0), (0, 9, 31, 1, 0), (50, 61, 31, 1, 0), (3, 60, 2, 8, 0), (58, 61, 31, 1, 0), (0, 3, 31, 1, 0)):
        lo, hi = slab[0], slab[1]
        assert window(probe, tri, first, size, n, slab, 0) == whole[0], "X-lines cross every layer: never clipped"
        for axis in (1, 2):
            (ulo, uhi, wlo, whi), cnt = window(probe, tri, first, size, n, slab, axis)
            (a, b, c, d), _ = whole[axis]
            want_lo, want_hi = max(a, lo), min(b, hi - 1)
            if want_lo > want_hi:
                assert cnt == 0 and ulo > uhi, (slab, axis)
            else:
                assert (ulo, uhi, wlo, whi) == (want_lo, want_hi, c, d) and cnt == (want_hi - want_lo + 1) * (d - c + 1), (slab, axis)
    # all == true wins over whatever the other fields hold
    assert [window(probe, tri, first, size, n, (20, 33, 2, 8, 1), axis) for axis in range(3)] == whole


@pytest.mark.parametrize("chunk_log", [0, 2, 31])
def test_x_in_slab_against_a_list_comprehension(probe, chunk_log):
    nx = 97
    chunk = 1 << min(chunk_log, 30)
    slabs = [(0, nx, chunk_log, max(chunk, 1), 0), (5, 60, chunk_log, 2 * chunk if chunk_log < 31 else 1, 0), (5, 61, chunk_log, 3 * chunk + 1 if chunk_log < 31 else 7, 0),
             (40, 41, chunk_log, 5 * chunk if chunk_log < 31 else 1, 0), (96, 97, chunk_log, chunk if chunk_log < 31 else 1, 0), (13, 13, chunk_log, 4 * chunk if chunk_log < 31 else 1, 0),
             (7, 90, chunk_log, 16 if chunk_log < 31 else 1, 0), (7, 90, chunk_log, 16 if chunk_log < 31 else 1, 1)]
    for lo, hi, cl, period, all_ in slabs:
        want = [1 if all_ or (lo <= x < hi and (cl >= 31 or (x - lo) % period < (1 << cl))) else 0 for x in range(nx)]
        got = np.zeros(nx, np.uint8)
        slab = np.array([lo, hi, cl, period, all_], U32)
        probe.probe_sign_x_in_slab(slab.ctypes.data, nx, got.ctypes.data)
        assert got.tolist() == want, (lo, hi, cl, period, all_)
    if chunk_log < 31:                                     # an interleaved slab really leaves layers out, a contiguous one none
        got = np.zeros(nx, np.uint8)
        slab = np.array([7, 90, chunk_log, 4 * chunk, 0], U32)
        probe.probe_sign_x_in_slab(slab.ctypes.data, nx, got.ctypes.data)
        assert 0 < got[7:90].sum() < 83


# ---- the bucket of a hit --------------------------------------------------------------------------------------------------------------------
def bucket_model(t, cs, n):
    """floor(t / cs) in f32, `as usize` as Rust casts (NaN -> 0, saturating at 0 and at usize::MAX), .min(n - 1)."""
    with np.errstate(all="ignore"):
        f = np.floor(F(t) / F(cs))
    if np.isnan(f) or f <= 0:
        k = 0
    elif f >= 2.0 ** 64:
        k = 2 ** 64 - 1
    else:
        k = int(f)
    return min(k, n - 1)


@pytest.mark.parametrize("cs", [1.0, 0.01, 0.3, 1.0 / 3.0, 1.0e-6, 1.0e6, -0.25, -1.0e-6])
def test_bucket_against_the_numpy_f32_model(probe, cs):
    """Found a bug when it was written: the kernel clamped with `f >= (float)n ? n - 1 : min((uint32_t)f, n - 1)`.  For n = 2^31 + 5 cells
    (float)n is 2^31, so a hit at t = 2^31 * cs (f = 2^31 <= n - 1) went into cell n - 1 = 2^31 + 4 where the reference's
    `(f as usize).min(n - 1)` gives 2^31; any n above 2^24 that f32 rounds down has such an f.  ray_bucket now guards the cast by 2^32."""
    cs = F(cs)
    ts = [0.0, -0.0, 1.0e-45, 1.0e-38, 1.0e-30, -1.0e-30, -1.0, -3.0e38, 1.0, 3.0e9, 5.0e9, 1.0e19, 2.0e19, 1.0e30, 3.4e38, INF, -INF, NAN]
    for j in (1, 2, 3, 6, 7, 31, 32, 99, 100, 101, 4095, 65535, 1 << 24, (1 << 31) - 64, 1 << 31, (1 << 32) - 256, 1 << 32):
        with np.errstate(all="ignore"):
            c = F(cs) * F(j)
        ts += [c, np.nextafter(c, F(INF)), np.nextafter(c, F(-INF)), -c]
    hit_last, hit_inner = 0, 0
    for n in (1, 2, 7, 100, 101, 2 ** 24 + 1, 2 ** 31 + 5, 2 ** 32 - 1):
        for t in ts:
            want, got = bucket_model(t, cs, n), probe.probe_sign_bucket(F(t), cs, n)
            assert got == want, f"t={F(t)!r} cs={cs!r} n={n}: bucket {got}, model {want}"
            hit_last += want == n - 1
            hit_inner += 0 < want < n - 1
    assert hit_last > 20 and (hit_inner > 20 or cs < 0)
    if cs < 0:                                             # t > 0 over a negative cell size: every hit lands in cell 0
        assert all(probe.probe_sign_bucket(F(t), cs, 100) == 0 for t in (0.1, 1.0, 77.0, INF))


# ---- the path of a call -----------------------------------------------------------------------------------------------------------------------
def path(probe, n_tris, count):
    out, consts = np.zeros(3, U32), np.zeros(4, np.uint64)
    cnt = np.array(count, U32)
    probe.probe_sign_path(n_tris, cnt.ctypes.data, out.ctypes.data, consts.ctypes.data)
    return tuple(int(x) for x in out), tuple(int(x) for x in consts)


def test_path_at_every_threshold(probe):
    (_, consts) = path(probe, 1, (1, 1, 1))
    assert consts == (64, 16384, 4096, 2048), "SMALL_WINDOW, RAY_MARK_SHARED_BELOW, LIST_ABOVE_LINES, BIG_CHUNK"
    small = (8, 8, 8)
    assert [path(probe, t, small)[0][0] for t in (1, 16383, 16384, 16385, 20000, 2 ** 32 - 1)] == [16, 16, 16, 1, 1, 1]
    # faces of 4 096 and 4 097 lines, on each pair of axes; the triangle count does not matter
    for t in (2, 20000):
        for perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
            for face, want in (((64, 64), 0), ((4096, 1), 0), ((1, 4096), 0), ((4097, 1), 1), ((17, 241), 1), ((241, 17), 1), ((63, 65), 0), ((64, 65), 1)):
                count = [0, 0, 0]
                count[perm[0]], count[perm[1]], count[perm[2]] = face[0], face[1], 1
                assert path(probe, t, count)[0][1] == want, (t, count)
    assert path(probe, 2, (40, 36, 8))[0][1] == 0 and path(probe, 2, (72, 68, 8))[0][1] == 1
    assert path(probe, 2, (70000, 70000, 1))[0][1] == 1                           # a face past 2^32 lines: 64-bit products
    # nz -> words per row -> the rows form (a power of two of at most 64 words) or the serial carry
    want_rows = {1: 1, 32: 1, 33: 1, 64: 1, 65: 0, 96: 0, 97: 1, 2048: 1, 2049: 0, 128: 1, 129: 0, 160: 0, 161: 0, 1024: 1, 1025: 0, 4096: 0}
    for nz, rows in want_rows.items():
        nzw = (nz + 31) // 32
        assert rows == int(nzw <= 64 and nzw & (nzw - 1) == 0), "the table itself"
        for t in (2, 20000):
            assert path(probe, t, (5, 6, nz))[0][2] == rows, nz
