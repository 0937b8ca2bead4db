"""m2s_band_csg / m2s_band_export / m2s_band_field_info on the GPU, bit for bit against tests/band_csg_model.py (the definition in numpy):
random bands on the smallest grids where the kernels can go wrong, the value and operand cases the definition singles out, chaining, the
result as a field against the dense calls, the export round trip, and mesh booleans of two spheres end to end.  Every comparison is exact
equality of bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import band_csg_model as cm
import grid_query_model as gqm
import isosurface_model as im
from mesh_to_sdf_amd import (BandField, CsgOp, Grid, M2SError, M2STimings, Mesh, SampleMode, Topology, _lib, boolean, grid_isosurface,
                             isosurface_band, raymarch_grid, sample_grid)

F = np.float32
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = (CsgOp.Union, CsgOp.Intersection, CsgOp.Difference)
MODES = [SampleMode.Snap, SampleMode.Trilinear, SampleMode.Tetrahedral]
FMAX = np.finfo(F).max
SPECIAL = np.array([0.0, -0.0, 0.5, -0.5, 0.75, -0.75, FMAX, -FMAX], F)   # zeros of both signs, the backgrounds, +-f32::MAX


def _np(x):
    if hasattr(x, "cpu"):
        if x.dtype == getattr(torch, "uint32", None):
            x = x.view(torch.int32)
        x = x.cpu().numpy()
    return np.asarray(x)


def _grid(shape):
    return Grid([-0.5, 0.25, 0.0], [0.125, 0.25, 0.1875], list(shape))


def _random_band(rng, shape, density=0.5, bits=True, bg=(0.75, 0.5), special=0.3, force=()):
    total = shape[0] * shape[1] * shape[2]
    act = rng.random(total) < density
    for L in force:
        if L < total:
            act[L] = True
    cells = np.flatnonzero(act)
    d = rng.uniform(-1, 1, cells.size).astype(F)
    pick = rng.random(cells.size) < special
    d[pick] = rng.choice(SPECIAL, int(pick.sum()))
    mask = rng.integers(0, 2 ** 32, (shape[0], shape[1], (shape[2] + 31) // 32), dtype=np.uint64).astype(np.uint32) if bits else None
    return cm.Band(shape, cells, d, mask, *bg)


def _field(grid, band, device):
    """The BandField of a model Band, from device tensors or host arrays."""
    bg = (float(band.bg_in), float(band.bg_out))
    if device:
        bits = None if band.bits is None else torch.as_tensor(np.ascontiguousarray(band.bits).view(np.int32), device=DEV)
        return BandField(grid, torch.as_tensor(band.cells, device=DEV), torch.as_tensor(band.distances, device=DEV), background=bg, inside=bits)
    return BandField(grid, band.cells.astype(np.uint64), band.distances, background=bg, inside=band.bits)


def _check(field, want, what):
    """The handle against a model Band: the export's three arrays, m2s_band_info's count and bytes, m2s_band_field_info."""
    nb = field.to_band()
    cells, dist, bits = _np(nb.cells).astype(np.int64), _np(nb.distances), _np(nb.bits).view(np.uint32)
    assert nb.count == want.cells.size == field.count, f"{what}: {nb.count} cells, the model has {want.cells.size}"
    assert np.array_equal(cells, want.cells), f"{what}: cells differ"
    assert dist.dtype == F and np.array_equal(dist.view(np.uint32), want.distances.view(np.uint32)), \
        f"{what}: {int((dist.view(np.uint32) != want.distances.view(np.uint32)).sum())} distances differ"
    want_bits = cm.pack_bits(want.shape, cm.unpack_bits(want.shape, want.bits))    # the caller's layout with the bits at k >= nz zero; None: zeros
    assert bits.shape == want_bits.shape and np.array_equal(bits, want_bits), f"{what}: {int((bits != want_bits).sum())} sign words differ"
    n, nbytes, fo, has = C.c_uint64(0), C.c_uint64(0), _lib.M2SBandFieldOpts(), C.c_int(-1)
    L = _lib.lib()
    assert L.m2s_band_info(field._h, None, C.byref(n), C.byref(nbytes)) == _lib.M2S_OK
    words = (want.total + 63) // 64
    assert n.value == want.cells.size and nbytes.value == 16 * words + 4 * n.value + (8 * words if want.bits is not None else 0), what
    assert L.m2s_band_field_info(field._h, C.byref(fo), C.byref(has)) == _lib.M2S_OK
    assert fo.struct_size == C.sizeof(fo) and has.value == (want.bits is not None), what
    assert F(fo.background_outside).view(np.uint32) == want.bg_out.view(np.uint32), what
    assert F(fo.background_inside).view(np.uint32) == want.bg_in.view(np.uint32), what
    assert field.background == (float(want.bg_in), float(want.bg_out)) and field.device_bytes == nbytes.value, what


def _all_ops(grid, a, b, what, device, same_handle=False):
    """csg(a, b) for the three ops against the model; with same_handle the one handle is both operands."""
    with _field(grid, a, device) as fa, (fa if same_handle else _field(grid, b, device)) as fb:
        for op in OPS:
            with fa.csg(fb, op) as fr:
                _check(fr, cm.csg(a, a if same_handle else b, int(op)), f"{what} {op.name}")


# ---- 1. random bands on the shapes where the kernels can go wrong ------------------------------------------------------------------------
# 5x6x7: 210 points, the last mask word partial, rows start mid-word, nz < 32.  3x2x67, 2x3x33: nz crosses a 64- and a 32-bit boundary.
# 1x1x64, 1x1x65: exactly one word, and one word plus one bit, with bit 63 and bit 0 of the next word active.
SMALL = [(5, 6, 7), (3, 2, 67), (2, 3, 33), (1, 1, 64), (1, 1, 65)]


@pytest.mark.parametrize("shape", SMALL, ids=lambda n: "x".join(map(str, n)))
def test_random_bands_and_the_cases_of_the_definition(shape):
    rng = np.random.default_rng(sum(shape))
    grid = _grid(shape)
    total = shape[0] * shape[1] * shape[2]
    edge = (63, 64)
    empty = lambda bits=True: _random_band(rng, shape, 0.0, bits=bits)
    full = lambda bg: _random_band(rng, shape, 1.1, bg=bg)
    rb = lambda **kw: _random_band(rng, shape, force=edge, **kw)
    # a == b ties with one side inactive: B repeats A's values where both are active and A's backgrounds where only B is
    a = rb()
    da = cm.dense(a)[1].reshape(-1)
    b = rb(density=0.6, bg=(0.5, 0.75))
    b = cm.Band(shape, b.cells, da[b.cells], b.bits, 0.5, 0.75)
    cases = [("random", rb(), rb(density=0.4, bg=(0.5, 0.25))),
             ("equal backgrounds", rb(bg=(0.75, 0.75)), rb(bg=(0.75, 0.75))),
             ("ties", a, b),
             ("zero backgrounds", rb(bg=(0.0, 0.0)), rb(density=0.3, bg=(0.0, 0.5))),
             ("A empty", empty(), rb()), ("B empty", rb(), empty()), ("both empty", empty(), empty(False)),
             ("A masked, B not", rb(), rb(bits=False)), ("B masked, A not", rb(bits=False), rb()), ("neither masked", rb(bits=False), rb(bits=False)),
             ("both full", full((0.75, 0.5)), full((0.25, 1.0))),
             ("dense and sparse", rb(density=0.95), rb(density=0.05, special=1.0))]
    ties = cm.dense(a)[1].reshape(-1) == cm.dense(b)[1].reshape(-1)
    assert (ties & (cm.dense(a)[0].reshape(-1) != cm.dense(b)[0].reshape(-1))).any() or total < 70, "no tie with one side inactive"
    assert all(L in cases[0][1].cells for L in edge if L < total)
    for at, (name, x, y) in enumerate(cases):
        _all_ops(grid, x, y, f"{shape} {name}", device=at % 2 == 0)
    x = rb()
    _all_ops(grid, x, x, f"{shape} a is b", device=True, same_handle=True)
    _all_ops(grid, rb(bits=False), None, f"{shape} a is b, no mask", device=False, same_handle=True)
    # an explicit background replaces the min rule and changes nothing else
    x, y = rb(), rb()
    with _field(grid, x, True) as fx, _field(grid, y, False) as fy, fx.csg(fy, "difference", background=(2.0, 0.125)) as fr:
        _check(fr, cm.csg(x, y, cm.DIFFERENCE, (0.125, 2.0)), f"{shape} explicit background")


def test_a_sparse_band_over_many_scan_tiles():
    """100 x 100 x 101: 15 782 mask words, four tiles of the scan, about 1 % of the points active: a quarter of the words have no
    active point in either operand and are settled at word level, the sign mask included; the others hold one or two."""
    shape = (100, 100, 101)
    rng = np.random.default_rng(5)
    grid = _grid(shape)
    a, b = _random_band(rng, shape, 0.01), _random_band(rng, shape, 0.012, bg=(0.5, 0.25))
    assert (a.total + 63) // 64 > 3 * 4096
    _all_ops(grid, a, b, "sparse", device=True)
    _all_ops(grid, a, _random_band(rng, shape, 0.01, bits=False), "sparse, B without a mask", device=False)
    _all_ops(grid, a, None, "sparse a is b", device=True, same_handle=True)
    _all_ops(grid, _random_band(rng, shape, 0.0), b, "sparse A empty", device=True)


# ---- 2. chaining ---------------------------------------------------------------------------------------------------------------------------
def test_chaining_stays_on_the_device_and_equals_the_model_applied_twice():
    shape = (5, 7, 67)
    rng = np.random.default_rng(11)
    grid = _grid(shape)
    a, b, c = (_random_band(rng, shape, d, bits=m, bg=bg) for d, m, bg in ((0.5, True, (0.75, 0.5)), (0.3, False, (0.5, 0.5)), (0.6, True, (1.0, 0.25))))
    with _field(grid, a, True) as fa, _field(grid, b, True) as fb, _field(grid, c, True) as fc:
        with fa | fb as u, u - fc as r:                                    # the intermediate is a handle: nothing is exported in between
            _check(r, cm.csg(cm.csg(a, b, cm.UNION), c, cm.DIFFERENCE), "(A | B) - C")
        with fa & fb as i, fc.union(i) as r, r.intersection(fa) as r2, r2.difference(r2) as r3:
            want = cm.csg(c, cm.csg(a, b, cm.INTERSECTION), cm.UNION)
            _check(r, want, "C | (A & B)")
            want2 = cm.csg(want, a, cm.INTERSECTION)
            _check(r2, want2, "(C | (A & B)) & A")
            _check(r3, cm.csg(want2, want2, cm.DIFFERENCE), "X - X")


# ---- 3. the result as a field ------------------------------------------------------------------------------------------------------------
def test_a_result_samples_and_marches_as_the_dense_grid_it_stands_for():
    shape = (5, 7, 67)
    rng = np.random.default_rng(12)
    grid = Grid(rng.uniform(-1, 1, 3), rng.uniform(0.05, 0.3, 3), list(shape))
    q = gqm.GridQ.of(grid)
    lo, hi = q.start - q.cs, q.end + q.cs
    pts = torch.as_tensor((lo + rng.random((3000, 3)) * (hi - lo)).astype(F), device=DEV)
    org = torch.as_tensor((lo + rng.random((300, 3)) * (hi - lo)).astype(F), device=DEV)
    dirs = rng.normal(size=(300, 3))
    dirs = torch.as_tensor((dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(F), device=DEV)
    a = _random_band(rng, shape, 0.6, special=0.0, bg=(0.75, 0.5))
    b = _random_band(rng, shape, 0.5, special=0.0, bits=False, bg=(0.5, 0.25))
    with _field(grid, a, True) as fa, _field(grid, b, True) as fb:
        for op in OPS:
            want = cm.csg(a, b, int(op))
            dense = torch.as_tensor(cm.dense(want)[1].reshape(-1), device=DEV)                # D'_R of the model
            with fa.csg(fb, op) as fr:
                for mode in MODES:
                    gv, gn = fr.sample(pts, mode=mode, normals=True)
                    wv, wn = sample_grid(grid, dense, pts, mode=mode, normals=True)
                    assert gqm.same_bits(_np(gv), _np(wv)) and gqm.same_bits(_np(gn), _np(wn)), (op, mode)
                    got = fr.raymarch(org, dirs, mode=mode, max_steps=40, normals=True)
                    ref = raymarch_grid(grid, dense, org, dirs, mode=mode, max_steps=40, normals=True)
                    for g, w in zip(got, ref):
                        g, w = _np(g), _np(w)
                        assert gqm.same_bits(g, w) if g.dtype == F else np.array_equal(g, w), (op, mode)


# ---- 4. export ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 6, 7), (3, 2, 67), (1, 1, 65)], ids=lambda n: "x".join(map(str, n)))
def test_export_is_the_inverse_of_create(shape):
    rng = np.random.default_rng(13 + sum(shape))
    grid = _grid(shape)
    pts = (np.array([-0.6, 0.2, -0.1]) + rng.random((500, 3)) * (np.array(shape) * np.array([0.125, 0.25, 0.1875]) + 0.2)).astype(F)
    for device in (False, True):
        for bits in (True, False):
            band = _random_band(rng, shape, bits=bits, force=(63, 64))
            with _field(grid, band, device) as f:
                _check(f, band, f"{shape} device {device} bits {bits}")            # without a mask: all-zero bits, has_inside 0
                nb = f.to_band()
                assert (torch.is_tensor(nb.cells) and nb.cells.is_cuda and nb.distances.is_cuda and nb.bits.is_cuda) == device
                assert nb.grid is grid and tuple(nb.bits.shape) == (shape[0], shape[1], (shape[2] + 31) // 32)
                # a handle recreated from the export answers as the first one
                with nb.field(background=f.background, inside=nb.bits) as again:
                    for mode in MODES:
                        v1, n1 = f.sample(pts, mode=mode, normals=True)
                        v2, n2 = again.sample(pts, mode=mode, normals=True)
                        assert gqm.same_bits(_np(v1), _np(v2)) and gqm.same_bits(_np(n1), _np(n2))
                    _check(again, cm.Band(shape, band.cells, band.distances, band.bits if bits else np.zeros_like(_np(nb.bits).view(np.uint32)),
                                          band.bg_out, band.bg_in), "recreated")


def test_export_rejects_a_short_capacity_and_writes_nothing():
    shape = (3, 2, 67)
    rng = np.random.default_rng(14)
    band = _random_band(rng, shape)
    n = band.cells.size
    L = _lib.lib()
    with _field(_grid(shape), band, False) as f:
        cells, dist, bits = np.full(n, 7, np.uint64), np.full(n, 7, F), np.full((3, 2, 3), 7, np.uint32)
        assert L.m2s_band_export(f._h, cells.ctypes.data, dist.ctypes.data, n - 1, bits.ctypes.data, None) == _lib.ERR_BAD_ARG
        assert "capacity" in _lib.last_error()
        assert (cells == 7).all() and (dist == 7).all() and (bits == 7).all()
        assert L.m2s_band_export(f._h, None, None, n, None, None) == _lib.ERR_BAD_ARG
        # each output alone, and a capacity above the count: nothing past the count is written
        big = np.full(n + 5, 7, np.uint64)
        assert L.m2s_band_export(f._h, big.ctypes.data, None, n + 5, None, None) == _lib.M2S_OK
        assert np.array_equal(big[:n].astype(np.int64), band.cells) and (big[n:] == 7).all()
        assert L.m2s_band_export(f._h, None, dist.ctypes.data, n, None, None) == _lib.M2S_OK
        assert np.array_equal(dist.view(np.uint32), band.distances.view(np.uint32)) and (cells == 7).all()
        assert L.m2s_band_export(f._h, None, None, n, bits.ctypes.data, None) == _lib.M2S_OK
        assert np.array_equal(bits, cm.pack_bits(shape, cm.unpack_bits(shape, band.bits)))         # the mask given, the bits at k >= nz zero
        assert not np.array_equal(bits, band.bits)                                                 # (the random mask had some set)
        o = _lib.M2SOpts()
        o.struct_size, o.device, o.x_end = C.sizeof(o), -1, 2
        assert L.m2s_band_export(f._h, big.ctypes.data, None, n + 5, None, C.byref(o)) == _lib.ERR_BAD_ARG


# ---- 5. what m2s_band_csg rejects of two handles -----------------------------------------------------------------------------------------
def test_csg_rejects_mismatching_grids_devices_and_options():
    shape = (5, 6, 7)
    rng = np.random.default_rng(15)
    band = _random_band(rng, shape)
    L = _lib.lib()
    BAD = _lib.ERR_BAD_ARG

    def call(fa, fb, op=0, fo=None, opts=None):
        h = C.c_void_p(0x1234)
        rc = L.m2s_band_csg(fa._h, fb._h, op, fo, opts, C.byref(h))
        assert (rc == _lib.M2S_OK) == (h.value is not None)
        if h.value is not None:
            L.m2s_band_destroy(h)
        return rc

    def opts(**kw):
        o = _lib.M2SOpts()
        o.struct_size, o.device = C.sizeof(o), -1
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)

    with _field(_grid(shape), band, True) as fa:
        for other in (Grid([-0.5, 0.25, np.nextafter(F(0.0), F(1.0))], [0.125, 0.25, 0.1875], list(shape)),     # one bit of first_cell
                      Grid([-0.5, 0.25, 0.0], [0.125, np.nextafter(F(0.25), F(1.0)), 0.1875], list(shape)),     # one bit of cell_size
                      Grid([-0.5, 0.25, 0.0], [0.125, 0.25, 0.1875], [5, 7, 6])):                               # the same count of cells, another shape
            with BandField(other, band.cells.astype(np.uint64), band.distances, background=0.5) as fb:
                assert call(fa, fb) == BAD and "grid" in _lib.last_error()
                with pytest.raises(M2SError):
                    fa | fb
        assert call(fa, fa, opts=opts(device=1)) == BAD and "device" in _lib.last_error()
        assert call(fa, fa, opts=opts(device=0)) == _lib.M2S_OK
        for field, value in (("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4), ("mem_kind", 5)):
            assert call(fa, fa, opts=opts(**{field: value})) == BAD, field
        for size, out, ins in ((8, 0.5, 0.5), (12, -0.5, 0.5), (12, 0.5, float("inf")), (12, float("nan"), 0.5)):
            assert call(fa, fa, fo=C.byref(_lib.M2SBandFieldOpts(size, out, ins))) == BAD
        assert call(fa, fa, op=3) == BAD
        t = M2STimings()
        h = C.c_void_p()
        assert L.m2s_band_csg(fa._h, fa._h, 0, None, opts(timings=C.pointer(t)), C.byref(h)) == _lib.M2S_OK
        n = C.c_uint64(0)
        assert L.m2s_band_info(h, None, C.byref(n), None) == _lib.M2S_OK
        assert t.n_units == n.value == band.cells.size and t.seed_ms > 0 and t.total_ms == t.seed_ms
        L.m2s_band_destroy(h)


# ---- 6. mesh booleans end to end -----------------------------------------------------------------------------------------------------------
def _icosphere(radius, centre, subdivisions=3):
    p = (1 + 5 ** 0.5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius + np.array(centre)).astype(F), np.array(f, np.uint32).reshape(-1)


def test_mesh_booleans_of_two_spheres_equal_the_dense_pipeline():
    """Two icospheres of radius 0.6 whose centres are 0.5 apart (the surfaces cross) on a 48^3 grid: for every op the isosurface of the
    combined field is grid_isosurface of the op of the two dense grids the bands stand for, in both arrays and to the bit, with n_open == 0;
    boolean() returns it; and the mesh is closed: every directed edge as often as its reverse, twice at most (an ambiguous face)."""
    grid = Grid.from_bounding_box([-1.2, -1.2, -1.2], [1.2, 1.2, 1.2], [48, 48, 48])
    va, ia = _icosphere(0.6, (-0.25, 0.02, 0.03))
    vb, ib = _icosphere(0.6, (0.25, -0.04, 0.01))
    w = isosurface_band(grid)
    assert w[0] == w[1]
    tva, tvb = torch.as_tensor(va, device=DEV), torch.as_tensor(vb, device=DEV)
    tia, tib = (Topology.TriangleList(torch.as_tensor(i.astype(np.int32), device=DEV)) for i in (ia, ib))
    with Mesh(tva, tia) as ma, Mesh(tvb, tib) as mb, ma.narrow_band_field(grid, w, inside=True, background=w) as fa, \
            mb.narrow_band_field(grid, w, inside=True, background=w) as fb:
        dense, act = [], []
        for f in (fa, fb):
            nb = f.to_band()
            band = cm.Band((48, 48, 48), _np(nb.cells), _np(nb.distances), _np(nb.bits).view(np.uint32), f.background[1], f.background[0])
            act.append(cm.dense(band)[0])
            dense.append(cm.dense(band)[1])
        assert fa.background == (w[0], w[1]) == fb.background
        for op in OPS:
            b = -dense[1] if op == CsgOp.Difference else dense[1]
            want = cm.select(cm.UNION if op == CsgOp.Union else cm.INTERSECTION, dense[0], b, act[0])      # min / max as the definition selects
            wv, wi = grid_isosurface(grid, torch.as_tensor(want.reshape(-1), device=DEV))
            with fa.csg(fb, op) as fr:
                assert fr.background == (w[0], w[1])
                gv, gi, n_open = fr.isosurface(0.0)
            assert n_open == 0 and gv.shape[0] > 500
            assert gqm.same_bits(_np(gv), _np(wv)) and np.array_equal(_np(gi), _np(wi)), op
            for bv, bi in (boolean(tva, tia, tvb, tib, op, grid), ma.boolean(mb, op.name.lower(), grid)):
                assert gqm.same_bits(_np(bv), _np(gv)) and np.array_equal(_np(bi), _np(gi)), op
            tris = _np(gi).astype(np.int64).reshape(-1, 3)
            e = im.directed_edges(tris)
            n = gv.shape[0]
            keys, counts = np.unique(e[:, 0] * n + e[:, 1], return_counts=True)
            rev, rcounts = np.unique(e[:, 1] * n + e[:, 0], return_counts=True)
            assert np.array_equal(keys, rev) and np.array_equal(counts, rcounts) and counts.max() <= 2, op
            # the solid is the one the op names: its volume from the two balls' lens.  The bound is a tenth of a ball: an icosphere of
            # 1280 faces lacks under 2 % of its ball, and marching cubes on cells of 0.05 moves a surface of radius 0.6 by far less
            vol = im.volume(_np(gv), tris)
            r, d = 0.6, float(np.linalg.norm(np.array([0.5, -0.06, -0.02])))
            lens = np.pi * (2 * r - d) ** 2 * (d * d + 4 * d * r) / (12 * d)
            ball = 4 / 3 * np.pi * r ** 3
            ideal = {CsgOp.Union: 2 * ball - lens, CsgOp.Intersection: lens, CsgOp.Difference: ball - lens}[op]
            assert abs(vol - ideal) < 0.1 * ball, (op, vol, ideal)


def test_c_and_cpp_consumers_run_clean(tmp_path):
    for cc, std, src, extra in (("gcc", "-std=c99", "tests/c/band_csg_smoke.c", ["-lm"]), ("g++", "-std=c++17", "tests/cpp/band_csg_tests.cpp", [])):
        exe = str(tmp_path / os.path.basename(src).split(".")[0])
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                               os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                               "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", *extra, "-o", exe])
        r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
