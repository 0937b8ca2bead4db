"""The f64 model behind tests/test_gpu_bounds.py (tests/bounds_model.py) and the two test hooks it uses, as far as they can be checked
without a GPU: the model's distance against the CPU oracle, its tree decoding and point sets on a hand-made tree, the record sizes, the
exports, and the argument checks that happen before any device work."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bounds_model as bm  # noqa: E402
import oracle as orc  # noqa: E402
from mesh_to_sdf_amd import _lib  # noqa: E402
from test_device_math_host import _cases  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


def test_model_distance_agrees_with_the_oracle():
    """The cases of test_device_math_host.py (regular, point and segment triangles, points on an edge line), to 1e-5 relative.  Relative to
    the larger of the distance and the largest |coordinate| of the case: the oracle works in f32 on coordinates up to 10, so its own result
    is uncertain by a few ulps of those (measured: at most 4.9e-6 absolute over these cases), which for a point on an edge line
    (true distance 4e-10 .. 1e-6) is many times the distance itself; the model, in f64, carries none of that."""
    cases = list(_cases(4000, 1))
    p, a, b, c = (np.array([x[k] for x in cases]) for k in range(4))
    got = bm.point_triangle_distance(p, a, b, c)
    want = np.array([orc.point_triangle_distance(*x) for x in cases], np.float64)
    size = np.maximum(got, np.abs(np.concatenate([p, a, b, c], 1)).max(1))
    err = np.abs(got - want) / size
    print(f"model against oracle: largest |difference| / size {err.max():.3g}, largest |difference| {np.abs(got - want).max():.3g}")
    assert (err <= 1e-5).all(), (int(np.argmax(err)), err.max())


def test_model_distance_on_known_configurations():
    """Closed forms, exactly representable: every region of a 3-4-5 style triangle, a segment and a point."""
    a, b, c = [0, 0, 0], [4, 0, 0], [0, 4, 0]
    cases = [([1, 1, 3], a, b, c, 3.0),          # face
             ([2, -3, 0], a, b, c, 3.0),         # edge ab
             ([-3, -4, 0], a, b, c, 5.0),        # vertex a
             ([7, -4, 0], a, b, c, 5.0),         # vertex b
             ([4, 4, 0], a, b, c, np.sqrt(8.0)),  # edge bc
             ([-3, 8, 0], a, b, c, 5.0),         # vertex c
             ([2, 3, 4], a, b, b, 5.0),          # segment ab (b == c)
             ([2, 3, 4], a, a, b, 5.0),          # segment (a == b)
             ([3, 4, 12], a, a, a, 13.0),        # point
             ([2, 0, 5], [0, 0, 0], [1, 0, 0], [4, 0, 0], 5.0)]   # collinear, distinct
    p, ta, tb, tc, want = (np.array([x[k] for x in cases], np.float64) for k in range(5))
    assert np.allclose(bm.point_triangle_distance(p, ta, tb, tc), want, rtol=1e-15, atol=0)


def test_record_sizes_match_common_h():
    assert {k: d.itemsize for k, d in bm.DTYPES.items()} == bm.ITEMSIZE == {"tris": 96, "planes": 64, "nodes": 32, "ext": 48}
    src = open(os.path.join(ROOT, "mesh_to_sdf_amd", "csrc", "common.h")).read()
    for name, size in (("TriRec", 96), ("TriPlanes", 64), ("NodeRec", 32), ("NodeExt", 48)):
        assert f"static_assert(sizeof({name}) == {size}" in src
    assert _lib.EVAL_RECORD_BYTES == {_lib.EVAL_EXT: 48, _lib.EVAL_PLANES: 64, _lib.EVAL_DIST2: 96}
    # field offsets as common.h lays the records out
    assert [bm.TRI.fields[k][1] for k in ("a", "cls", "b", "index", "c", "ab", "nrx", "ac", "bc", "nrz")] == [0, 12, 16, 28, 32, 48, 60, 64, 80, 92]
    assert [bm.EXT.fields[k][1] for k in ("c", "R", "n", "mid", "half", "skip", "tri")] == [0, 12, 16, 28, 32, 36, 40]
    assert [bm.NODE.fields[k][1] for k in ("mn", "skip", "mx", "tri")] == [0, 12, 16, 28]
    assert [bm.PLANES.fields[k][1] for k in ("n", "dn", "m0", "o0", "m1", "o1", "m2", "o2")] == [0, 12, 16, 28, 32, 44, 48, 60]


def test_tree_decoding_on_a_hand_made_tree():
    """Five triangles: root(0..4) -> [A(0..2) -> [leaf 0, B(1..2) -> [leaf 1, leaf 2]], C(3..4) -> [leaf 3, leaf 4]], in pre-order."""
    skip = np.array([9, 6, 3, 6, 5, 6, 9, 8, 9])
    first = np.array([0, 0, 0, 1, 1, 2, 3, 3, 4])
    assert bm.tree_errors(skip, first, 5) == []
    assert list(bm.subtree_counts(skip)) == [5, 3, 1, 2, 1, 1, 2, 1, 1]
    k, node = bm.ancestors(skip, first, np.arange(5))
    paths = {t: sorted(node[k == t]) for t in range(5)}
    assert paths == {0: [0, 1, 2], 1: [0, 1, 3, 4], 2: [0, 1, 3, 5], 3: [0, 6, 7], 4: [0, 6, 8]}
    for broken in (np.array([9, 6, 3, 6, 5, 6, 9, 8, 8]), np.array([9, 6, 3, 5, 5, 6, 9, 8, 9]), np.array([8, 6, 3, 6, 5, 6, 9, 8, 9])):
        assert bm.tree_errors(broken, first, 5)
    assert bm.tree_errors(skip, np.array([0, 0, 0, 1, 1, 2, 3, 4, 4]), 5)
    assert bm.tree_errors(skip[:7], first[:7], 5)


def test_point_sets_and_containment_checks():
    rng = np.random.default_rng(0)
    a, b, c = (rng.uniform(-1, 1, (7, 3)).astype(F) for _ in range(3))
    b[1] = a[1]                       # a segment triangle
    b[2] = a[2]
    c[2] = a[2]                       # a point triangle
    pts = bm.triangle_points(a, b, c, 2.0, np.random.default_rng(1))
    assert pts.shape == (7, 58, 3) and np.isfinite(pts).all()
    d = bm.point_triangle_distance(bm.round_points(pts[:, :9]).reshape(-1, 3), *(np.repeat(x, 9, 0) for x in (a, b, c)))
    assert d.max() < 4 * 2.0 ** -24 * 2                              # the first nine lie on the triangle, up to their own rounding
    ext = np.zeros(2, bm.EXT)
    ext["c"], ext["n"], ext["R"], ext["mid"], ext["half"] = [[1, 2, 3], [0, 0, 0]], [[0, 0, 1], [0.6, 0.8, 0]], [2, 1], [0.5, 0], [0.25, 0]
    dp = bm.disc_points(ext)
    assert dp.shape == (2, 60, 3)
    w = dp - ext["c"].astype(np.float64)[:, None, :]
    t = (w * ext["n"].astype(np.float64)[:, None, :]).sum(2)
    lat = np.sqrt(np.maximum((w * w).sum(2) - t * t, 0))
    assert np.allclose(np.unique(np.round(t[0], 9)), [0.2475, 0.25, 0.5, 0.75, 0.7525])
    assert np.allclose(np.unique(np.round(lat[0], 9)), [0, 1.98, 2, 2.02, 12.8, 200])
    # containment: a triangle inside its record passes, one that sticks out of the slab or the disc does not
    tris = np.zeros(3, bm.TRI)
    tris["a"], tris["b"], tris["c"] = [[1, 2, 3.5]] * 3, [[2, 2, 3.25], [2, 2, 3.2], [3.5, 2, 3.5]], [[1, 3, 3.75]] * 3
    slab, rad, _ = bm.ext_reserves(ext, tris, np.arange(3), np.zeros(3, np.int64))
    assert not bm.outside(slab[0]).any() and not bm.outside(rad[0]).any()
    assert bm.outside(slab[1]).any() and not bm.outside(rad[1]).any()
    assert bm.outside(rad[2]).any() and not bm.outside(slab[2]).any()
    assert not bm.outside(np.array([np.nan, np.inf, 0.0])).any()
    low = bm.lowered_d2(np.array([0.0, 1.0, 4.0e-12, np.inf], F))
    assert low.dtype == F and low[0] == 0 and low[3] == np.inf
    assert float(low[1]) <= (1 - 2.0 ** -22 - 1e-6) ** 2 < float(np.nextafter(low[1], F(2)))
    assert float(low[2]) <= (2.0e-6 * (1 - 2.0 ** -22) - 1e-6) ** 2 < float(np.nextafter(low[2], F(2)))


def test_hooks_are_exported_and_stay_out_of_the_header(lib):
    hdr = open(os.path.join(ROOT, "include", "m2s.h")).read()
    for name in ("m2s_debug_mesh_arrays", "m2s_debug_eval"):
        assert hasattr(lib, name), name
        assert name not in hdr and name not in _lib.EXPORTS


def test_bad_arguments_fail_before_the_device(lib):
    BAD = _lib.ERR_BAD_ARG
    arrays = lib.m2s_debug_mesh_arrays
    arrays.restype = C.c_int
    arrays.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    buf, nbytes = np.zeros(64, np.uint32), C.c_size_t(77)
    for which in (0, 3, 7, -1, 8):
        assert arrays(None, which, buf.ctypes.data, buf.nbytes, C.byref(nbytes)) == BAD        # NULL mesh, whatever else
        assert arrays(None, which, None, 0, C.byref(nbytes)) == BAD
    assert "NULL mesh" in _lib.last_error()
    assert nbytes.value == 77                                                                    # no failed check writes *bytes
    ev = lib.m2s_debug_eval
    ev.restype = C.c_int
    ev.argtypes = [C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    pts, rec, aux, out = np.zeros((4, 3), F), np.zeros(4 * 96, np.uint8), np.zeros((4, 2), F), np.full(4, 7, F)
    P, R, A, O = pts.ctypes.data, rec.ctypes.data, aux.ctypes.data, out.ctypes.data
    for kind in (-1, 5, 99):
        assert ev(kind, 4, P, R, A, O) == BAD
    assert "kind" in _lib.last_error()
    for kind, args in ((0, (None, R, A, O)), (0, (P, None, A, O)), (1, (P, None, None, O)), (2, (P, R, A, None)), (3, (None, None, A, O)),
                       (3, (P, None, None, O)), (4, (None, None, None, O)), (4, (None, None, A, None))):
        assert ev(kind, 4, *args) == BAD, (kind, args)
    assert "NULL" in _lib.last_error()
    assert ev(0, 2 ** 26 + 1, P, R, A, O) == BAD
    for kind in range(5):
        assert ev(kind, 0, None, None, None, None) == _lib.M2S_OK                                # nothing to do: no device needed
    assert (out == 7).all()
    with pytest.raises(ValueError):
        _lib.debug_eval(_lib.EVAL_EXT, pts, rec)                                                 # 4 points, 8 records of 48 bytes
    with pytest.raises(ValueError):
        _lib.debug_eval(_lib.EVAL_SLACK, pts, rec, aux)                                          # a kind without records
