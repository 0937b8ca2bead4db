"""m2s_band_from_capsules on the GPU (BandField.from_capsules / from_spheres / from_points / from_edges) against the numpy model of the
definition (tests/band_shapes_model.py): the cells, the values, the sign mask on every grid point and the call's info, all for EQUALITY.
The chains end in the existing models: band_measure_model, band_csg_model, band_components_model's raster labelling through the library."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import band_csg_model as cm
import band_measure_model as mm
import band_shapes_model as sm
import band_window as bw
from mesh_to_sdf_amd import BandField, Grid, M2SError, Mesh, SampleMode, ShapesInfo, Topology, _lib
from test_band_shapes_cpu import CONSUMERS, build_consumer

F = np.float32
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIRST = (-0.5, 0.25, 3.0)
CELL = (0.125, 0.25, 0.1875)


def _np(x):
    if hasattr(x, "cpu"):
        if x.dtype == getattr(torch, "uint32", None):
            x = x.view(torch.int32)
        x = x.cpu().numpy()
    return np.asarray(x)


def _box(first, cell, shape):
    lo = np.asarray(first, np.float64) - 0.5 * np.asarray(cell)
    return lo, lo + np.asarray(shape) * np.asarray(cell)


def _make(grid, a, b, r, band, device, **kw):
    """from_capsules from device tensors or host arrays; the radius a scalar or an array on the same side."""
    if device:
        a = torch.as_tensor(np.asarray(a, F).reshape(-1, 3), device=DEV)
        b = None if b is None else torch.as_tensor(np.asarray(b, F).reshape(-1, 3), device=DEV)
        r = r if np.isscalar(r) else torch.as_tensor(np.asarray(r, F), device=DEV)
    else:
        a, b = np.asarray(a, F).reshape(-1, 3), (None if b is None else np.asarray(b, F).reshape(-1, 3))
        r = r if np.isscalar(r) else np.asarray(r, F)
    return BandField.from_capsules(grid, a, b, r, band, **kw)


def _check(field, want, what, widths=None):
    """The handle against the model's Result on the whole grid: the export's three arrays, the info, the handle's counts."""
    nb = field.to_band()
    cells, dist, bits = _np(nb.cells).astype(np.int64), _np(nb.distances), _np(nb.bits).view(np.uint32)
    assert nb.count == want.cells.size == field.count, f"{what}: {nb.count} cells, the model has {want.cells.size}"
    assert np.array_equal(cells, want.cells), f"{what}: cells differ"
    assert dist.dtype == F and np.array_equal(dist.view(np.uint32), want.values.view(np.uint32)), \
        f"{what}: {int((dist.view(np.uint32) != want.values.view(np.uint32)).sum())} values differ"
    want_bits = sm.pack_bits(want.inside)
    assert bits.shape == want_bits.shape and np.array_equal(bits, want_bits), f"{what}: {int((bits != want_bits).sum())} sign words differ"
    assert field.shapes_info == ShapesInfo(want.cells.size, want.n_inside, want.n_skipped, want.n_off_grid), (what, field.shapes_info, want.n_inside, want.n_skipped, want.n_off_grid)
    words = (int(np.prod(want.shape)) + 63) // 64
    assert field.device_bytes == 24 * words + 4 * want.cells.size, what
    if widths is not None:
        assert field.background == (float(F(widths[0])), float(F(widths[1]))), what


def _random_shapes(rng, first, cell, shape, n, rmax):
    lo, hi = _box(first, cell, shape)
    a = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (n, 3))
    b = a + rng.normal(0, 0.2, (n, 3)) * (hi - lo)
    b[::3] = a[::3]                                     # a third are spheres
    r = rng.uniform(0, rmax, n)
    r[::7] = 0.0
    return a.astype(F), b.astype(F), r.astype(F)


# ---- 1. mixed shapes on two grids --------------------------------------------------------------------------------------------------------
# (9, 7, 70): rows straddle mask words (70 is no multiple of 64) and the last word is partial.  (48, 40, 44): 1320 words, more than one
# wave's unit of 256 and more than one workgroup; rows of 44 share words.
@pytest.mark.parametrize("shape,n", [((9, 7, 70), 12), ((48, 40, 44), 60)])
def test_mixed_shapes_equal_the_model(shape, n):
    rng = np.random.default_rng(sum(shape))
    grid = Grid(list(FIRST), list(CELL), list(shape))
    a, b, r = _random_shapes(rng, FIRST, CELL, shape, n, 0.7)
    for (interior, exterior), device, scalar in (((0.3, 0.45), True, False), ((0.5, 0.25), False, False), ((0.3, 0.45), False, True), ((0.2, 0.2), True, True)):
        rr = 0.4 if scalar else r
        want = sm.run(FIRST, CELL, shape, a, b, rr, exterior, interior)
        assert want.cells.size > 200 and want.n_inside > 50 and (~want.active & want.inside).any()
        with _make(grid, a, b, rr, (interior, exterior), device) as f:
            _check(f, want, f"{shape} widths ({interior}, {exterior}) device {device} scalar {scalar}", (interior, exterior))


# ---- 2. contention and order -------------------------------------------------------------------------------------------------------------
def test_heavy_overlap_equals_the_model_in_any_order():
    shape = (40, 36, 44)
    rng = np.random.default_rng(5)
    grid = Grid(list(FIRST), list(CELL), list(shape))
    lo, hi = _box(FIRST, CELL, shape)
    spot = lo + 0.4 * (hi - lo)
    centres = spot + rng.uniform(-2, 2, (500, 3)) * np.asarray(CELL)                      # 500 spheres within two cells of one place
    nodes = lo + (0.15 + 0.7 * rng.random((40, 3))) * (hi - lo)
    e = rng.integers(0, 40, (300, 2))                                                      # 300 struts that meet at 40 shared nodes
    a = np.concatenate([centres, nodes[e[:, 0]]]).astype(F)
    b = np.concatenate([centres, nodes[e[:, 1]]]).astype(F)
    r = np.concatenate([rng.uniform(0.1, 0.5, 500), rng.uniform(0.02, 0.12, 300)]).astype(F)
    want = sm.run(FIRST, CELL, shape, a, b, r, 0.3, 0.25)
    assert want.cells.size > 3000 and want.n_off_grid == 0
    perm = rng.permutation(800)
    with _make(grid, a, b, r, (0.25, 0.3), True) as f, _make(grid, a[perm], b[perm], r[perm], (0.25, 0.3), True) as fp, _make(grid, a, b, r, (0.25, 0.3), True) as f2:
        _check(f, want, "contention")
        _check(fp, want, "contention, permuted")
        _check(f2, want, "contention, again")


# ---- 3. depth ----------------------------------------------------------------------------------------------------------------------------
def test_depth_beyond_interior_is_inactive_with_its_sign_set():
    shape, cell, first = (28, 28, 28), (0.25, 0.25, 0.25), (0.0, 0.0, 0.0)
    grid = Grid(list(first), list(cell), list(shape))
    c = (3.4, 3.45, 3.3)
    big = sm.run(first, cell, shape, [c], None, 9 * 0.25, 0.5, 0.5)                         # radius 9 cells, interior 2 cells
    core = big.inside & ~big.active
    assert core.sum() > 1000 and big.n_inside == int(big.inside.sum())
    with _make(grid, [c], None, 2.25, 0.5, True) as f:
        _check(f, big, "a ball of 9 cells")
    # a ball of 2 cells at its centre adds nothing
    with _make(grid, [c, c], None, [2.25, 0.5], 0.5, True) as f:
        both = sm.run(first, cell, shape, [c, c], None, [2.25, 0.5], 0.5, 0.5)
        assert np.array_equal(both.cells, big.cells) and np.array_equal(both.values.view(np.uint32), big.values.view(np.uint32))
        _check(f, both, "a small ball inside")
    # a ball across the shell: where it is deeper than interior the shell's cells go
    c2 = (c[0] + 2.25, c[1], c[2])
    cut = sm.run(first, cell, shape, [c, c2], None, [2.25, 1.0], 0.5, 0.5)
    lost = np.setdiff1d(big.cells, cut.cells)
    d2 = sm.dist(np.asarray(c2, F), np.asarray(c2, F), F(1.0), np.meshgrid(*sm.centres(first, cell, (0, 0, 0), shape), indexing="ij")).reshape(-1)
    assert lost.size > 20 and np.array_equal(lost, np.intersect1d(big.cells, np.flatnonzero(d2 < -F(0.5))))
    with _make(grid, [c, c2], None, [2.25, 1.0], 0.5, False) as f:
        _check(f, cut, "a ball across the shell")
    for interior, exterior in ((0.0, 0.5), (0.5, 0.0), (0.0, 0.0)):
        want = sm.run(first, cell, shape, [c, c2], None, [2.25, 1.0], exterior, interior)
        assert (want.cells.size > 0) == (interior + exterior > 0)
        with _make(grid, [c, c2], None, [2.25, 1.0], (interior, exterior), True) as f:
            _check(f, want, f"widths ({interior}, {exterior})", (interior, exterior))


# ---- 4. degenerate input ---------------------------------------------------------------------------------------------------------------
def test_degenerate_shapes():
    shape = (20, 18, 40)
    rng = np.random.default_rng(9)
    grid = Grid(list(FIRST), list(CELL), list(shape))
    a, b, r = _random_shapes(rng, FIRST, CELL, shape, 30, 0.5)
    # b == a equals b = NULL bit for bit
    want = sm.run(FIRST, CELL, shape, a, None, r, 0.3, 0.3)
    with _make(grid, a, a, r, 0.3, True) as f, _make(grid, a, None, r, 0.3, True) as g:
        _check(f, want, "b == a")
        _check(g, want, "b NULL")
    # r = 0: points and bare segments, no sign bits
    want = sm.run(FIRST, CELL, shape, a, b, 0.0, 0.3, 0.3)
    assert want.n_inside == 0 and want.cells.size > 100
    with _make(grid, a, b, 0.0, 0.3, True) as f:
        _check(f, want, "r = 0")
    with BandField.from_points(grid, a, 0.0, 0.3) as f:
        _check(f, sm.run(FIRST, CELL, shape, a, None, 0.0, 0.3, 0.3), "from_points")
    # shapes that are not sound are counted and the rest is unchanged
    good = sm.run(FIRST, CELL, shape, a, b, r, 0.3, 0.3)
    a2, b2, r2 = (np.concatenate([x, x[:5]]) for x in (a, b, r))
    a2[30, 1], b2[31, 2], r2[32], r2[33], r2[34] = np.nan, np.inf, -0.25, np.nan, np.inf
    bad = sm.run(FIRST, CELL, shape, a2, b2, r2, 0.3, 0.3)
    assert bad.n_skipped == 5 and np.array_equal(bad.cells, good.cells) and np.array_equal(bad.values.view(np.uint32), good.values.view(np.uint32))
    for device in (True, False):
        with _make(grid, a2, b2, r2, 0.3, device) as f:
            _check(f, bad, f"unsound shapes, device {device}")
    # n = 0, and shapes that are all off the grid: an empty field that is a valid handle
    lo, hi = _box(FIRST, CELL, shape)
    off = np.concatenate([hi + 1.0 + rng.random((6, 3)), lo - 1.0 - rng.random((6, 3))]).astype(F)
    for aa, what in ((np.zeros((0, 3), F), "n = 0"), (off, "off the grid")):
        want = sm.run(FIRST, CELL, shape, aa, None, 0.2, 0.3, 0.3)
        assert want.cells.size == 0 and want.n_off_grid == aa.shape[0]
        for device in (True, False):
            with _make(grid, aa, None, 0.2, 0.3, device) as f:
                _check(f, want, what)
                pts = np.asarray([FIRST, [FIRST[m] + 2 * CELL[m] for m in range(3)]], F)
                assert f.count == 0 and _np(f.sample(pts, mode=SampleMode.Snap, outside=7.0)).tolist() == [F(0.3)] * 2 and f.to_band().count == 0


def test_shapes_cut_by_the_grids_faces_and_one_ball_larger_than_the_grid():
    shape = (20, 18, 40)
    grid = Grid(list(FIRST), list(CELL), list(shape))
    lo, hi = _box(FIRST, CELL, shape)
    mid = 0.5 * (lo + hi)
    a = []
    for axis in range(3):
        for end in (lo, hi):
            p = mid.copy()
            p[axis] = end[axis] + (0.1 if end is lo else -0.1) * CELL[axis]
            a.append(p)
    a = np.asarray(a, F)
    b = a + np.asarray([0.3, -0.2, 0.4], F)
    want = sm.run(FIRST, CELL, shape, a, b, 0.45, 0.3, 0.2)
    assert all(want.active.take(i, axis).any() for axis in range(3) for i in (0, -1))
    with _make(grid, a, b, 0.45, (0.2, 0.3), True) as f:
        _check(f, want, "six faces")
    # one ball larger than the whole grid and ten tiny ones: the rows of the large one are shared among the waves
    rng = np.random.default_rng(3)
    tiny = (lo + rng.random((10, 3)) * (hi - lo)).astype(F)
    centre = (mid + np.asarray([9.0, 0.0, 0.0])).astype(F)                                  # its surface passes through the grid
    aa = np.concatenate([tiny[:5], centre[None], tiny[5:]])
    rr = np.concatenate([np.full(5, 0.2), [9.0 + 0.3], np.full(5, 0.2)]).astype(F)
    want = sm.run(FIRST, CELL, shape, aa, None, rr, 0.3, 0.3)
    assert want.n_inside > 1000 and want.cells.size > 1000 and want.n_off_grid == 0
    with _make(grid, aa, None, rr, 0.3, True) as f:
        _check(f, want, "a ball larger than the grid")
    whole = sm.run(FIRST, CELL, shape, [mid], None, 100.0, 0.3, 0.3)                       # the grid deep inside one ball: no cell, every sign bit
    assert whole.cells.size == 0 and whole.n_inside == int(np.prod(shape))
    with _make(grid, [mid], None, 100.0, 0.3, True) as f:
        _check(f, whole, "the grid inside one ball")


# ---- 5. far from the origin --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n", [((9, 7, 70), 12), ((48, 40, 44), 60)])
def test_far_from_the_origin(shape, n):
    first = (1000.0, -250.0, 0.0)
    shift = np.asarray(first) - np.asarray(FIRST)
    rng = np.random.default_rng(sum(shape))
    grid = Grid(list(first), list(CELL), list(shape))
    a, b, r = _random_shapes(rng, FIRST, CELL, shape, n, 0.7)
    a, b = (a + shift).astype(F), (b + shift).astype(F)
    want = sm.run(first, CELL, shape, a, b, r, 0.45, 0.3)
    assert want.cells.size > 200
    with _make(grid, a, b, r, (0.3, 0.45), True) as f:
        _check(f, want, f"{shape} at {first}")


# ---- 6. past 2^32 points -----------------------------------------------------------------------------------------------------------------
def test_shapes_at_the_far_corner_of_a_grid_past_2_to_the_32():
    big = (1700, 1600, 1600)
    assert big[0] * big[1] * big[2] > 2 ** 32
    win = bw.Window(big, tuple(n - 20 for n in big), (20, 20, 20))
    at = lambda i, j, k: [FIRST[m] + (big[m] - 20 + v) * CELL[m] for m, v in enumerate((i, j, k))]   # noqa: E731
    a = np.asarray([at(15.3, 17.6, 16.9), at(5.2, 5.4, 5.1), at(6.0, 12.0, 6.0)], F)      # a ball the three far faces cut, a whole one, a capsule
    b = np.asarray([at(15.3, 17.6, 16.9), at(5.2, 5.4, 5.1), at(9.0, 14.0, 12.0)], F)
    r = np.asarray([6.2 * 0.125, 3.1 * 0.125, 1.6 * 0.125], F)
    widths = (0.25, 0.25)
    want = sm.run(FIRST, CELL, big, a, b, r, widths[1], widths[0], window=(win.lo, win.shape))
    # nothing of the shapes reaches the window's inner sides: the window is the whole result
    for axis in range(3):
        assert not np.take(want.active, 0, axis).any() and not np.take(want.inside, 0, axis).any() and not (np.take(want.D, 0, axis) <= F(widths[1])).any()
    cells = win.to_big(want.cells)
    assert cells.size > 500 and (cells > 2 ** 32).all() and int(cells[-1]) == big[0] * big[1] * big[2] - 1
    with BandField.from_capsules(Grid(list(FIRST), list(CELL), list(big)), torch.as_tensor(a, device=DEV), torch.as_tensor(b, device=DEV),
                                 torch.as_tensor(r, device=DEV), widths) as f:
        assert f.shapes_info == ShapesInfo(cells.size, want.n_inside, 0, 0)
        nb = f.to_band()
        assert np.array_equal(_np(nb.cells).astype(np.int64), cells)
        assert np.array_equal(_np(nb.distances).view(np.uint32), want.values.view(np.uint32))
        words = nb.bits if nb.bits.dtype == torch.int32 else nb.bits.view(torch.int32)
        got_bits = win.get_bits(_np(words[win.word_slices()]).view(np.uint32))
        assert np.array_equal(got_bits, want.inside)
        assert f.shapes_info.n_inside == int(got_bits.sum())               # the window holds every set bit of the grid: the device's count says so
        del words
        del nb
    torch.cuda.empty_cache()


# ---- 7. chains, exact against the existing models ------------------------------------------------------------------------------------------
def test_spheres_measure_as_the_measure_model_says():
    shape, cell, first = (40, 40, 40), (0.05, 0.05, 0.05), (0.0, 0.0, 0.0)
    grid = Grid(list(first), list(cell), list(shape))
    centres = np.asarray([(0.52, 0.51, 0.49), (1.43, 1.38, 1.47), (0.5, 1.5, 0.55)], F)
    r = np.asarray([0.31, 0.36, 0.22], F)
    want = sm.run(first, cell, shape, centres, None, r, 0.1, 0.1)
    with BandField.from_spheres(grid, torch.as_tensor(centres, device=DEV), torch.as_tensor(r, device=DEV), 0.1) as f:
        _check(f, want, "three balls")
        m = f.measure()
        raw = mm.measure(shape, cell, want.cells.astype(np.uint64), want.values)
        assert (m.n_triangles, m.n_vertices, m.n_open, m.n_border) == tuple(int(x[0]) for x in (raw.n_triangles, raw.n_vertices, raw.n_open, raw.n_border))
        assert (m.area_q, m.volume_q, m.moment_q) == (int(raw.area_q[0]), int(raw.volume_q[0]), tuple(int(v) for v in raw.moment_q[0]))
        assert m.closed and m.euler == 2 * 3
        parts = f.measure(0.0, f.components(26))
        assert len(parts) == 3 and all(p.closed and p.euler == 2 for p in parts)
        assert sum(p.volume for p in parts) == pytest.approx(float(4 / 3 * np.pi * (r.astype(np.float64) ** 3).sum()), rel=0.05)


def test_a_hole_drilled_through_a_mesh_field(suzanne):
    v, i = suzanne
    shape = (48, 48, 48)
    lo, hi = v.min(0) - 0.15, v.max(0) + 0.15
    cell = ((hi - lo) / np.asarray(shape)).astype(F)
    first = (lo + 0.5 * cell).astype(F)
    grid = Grid([float(x) for x in first], [float(x) for x in cell], list(shape))
    w = float(2.5 * cell.max())
    tv = torch.as_tensor(np.asarray(v, F), device=DEV)
    ti = Topology.TriangleList(torch.as_tensor(np.asarray(i).astype(np.int32), device=DEV))
    mid = 0.5 * (lo + hi)
    a, b = np.asarray([[mid[0], mid[1], lo[2] - 1.0]], F), np.asarray([[mid[0], mid[1], hi[2] + 1.0]], F)
    with Mesh(tv, ti) as mesh, mesh.narrow_band_field(grid, w, inside=True, background=w) as part, \
            BandField.from_capsules(grid, torch.as_tensor(a, device=DEV), torch.as_tensor(b, device=DEV), 0.25, w) as drill, part - drill as holed:
        bands = []
        for f in (part, drill, holed):
            nb = f.to_band()
            bands.append(cm.Band(shape, _np(nb.cells), _np(nb.distances), _np(nb.bits).view(np.uint32), f.background[1], f.background[0]))
        assert bands[1].cells.size > 1000 and drill.shapes_info.n_inside > 500
        assert cm.same(bands[2], cm.csg(bands[0], bands[1], cm.DIFFERENCE))
        assert holed.count > part.count * 0.5 and not np.array_equal(bands[2].cells, bands[0].cells)


def test_the_edges_of_a_cube_are_one_component_and_a_closed_mesh():
    shape, cell, first = (40, 40, 40), (0.05, 0.05, 0.05), (0.0, 0.0, 0.0)
    grid = Grid(list(first), list(cell), list(shape))
    corners = np.asarray([[x, y, z] for x in (0.5, 1.5) for y in (0.5, 1.5) for z in (0.5, 1.5)], F)
    edges = np.asarray([(p, q) for p in range(8) for q in range(p + 1, 8) if bin(p ^ q).count("1") == 1])
    assert edges.shape == (12, 2)
    want = sm.run(first, cell, shape, corners[edges[:, 0]], corners[edges[:, 1]], 0.12, 0.1, 0.1)
    for device in (True, False):
        vv = torch.as_tensor(corners, device=DEV) if device else corners
        with BandField.from_edges(grid, vv, edges, 0.12, 0.1) as f:
            _check(f, want, f"the cube's edges, device {device}")
            assert f.components(6).count == 1
            verts, idx, n_open = f.isosurface()
            m = f.measure()
            assert n_open == 0 and m.closed and m.n_triangles == len(_np(idx)) > 1000
            assert m.euler == 2 - 2 * 5                                                     # a cube's wireframe is a surface of genus 5
    with pytest.raises(M2SError):
        BandField.from_edges(grid, corners, [[0, 8]], 0.1, 0.1)


# ---- 8. what a real device rejects ---------------------------------------------------------------------------------------------------------
def test_the_call_rejects_bad_options_on_a_device_and_fills_the_timings():
    L = _lib.lib()
    BAD = _lib.ERR_BAD_ARG
    g = _lib.M2SGrid()
    for m in range(3):
        g.first_cell[m], g.cell_size[m], g.cell_count[m] = 0.0, 1.0, 16
    so = _lib.M2SBandShapesOpts(16, 1.0, 1.0, 3.0)
    dev_a = torch.as_tensor(np.asarray([[8, 8, 8]], F), device=DEV)
    host_a = np.asarray([[8, 8, 8]], F)

    def opts(**kw):
        o = _lib.M2SOpts()
        o.struct_size, o.device, o.mem_kind = C.sizeof(o), -1, _lib.MEM_DEVICE
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)

    def call(o, pa=dev_a.data_ptr(), tm=None):
        h = C.c_void_p()
        rc = L.m2s_band_from_capsules(C.byref(g), pa, None, None, 1, C.byref(so), None, o, C.byref(h), None, tm)
        if h.value:
            L.m2s_band_destroy(h)
        return rc

    assert call(opts()) == _lib.M2S_OK
    # a device the memory is not on: out of range on a machine with one device, another device's otherwise
    assert call(opts(device=torch.cuda.device_count())) == BAD and "device" in _lib.last_error()
    if torch.cuda.device_count() > 1:
        assert call(opts(device=1)) == BAD and "device" in _lib.last_error()
    # host memory passed as device memory
    assert call(opts(), pa=host_a.ctypes.data) == BAD and "not device memory" in _lib.last_error()
    for field, value in (("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4), ("mem_kind", 5)):
        assert call(opts(**{field: value})) == BAD, field
    tm = _lib.M2STimings()
    assert call(opts(), tm=C.byref(tm)) == _lib.M2S_OK
    assert tm.total_ms > 0 and tm.seed_ms > 0 and tm.distance_ms > 0 and tm.total_ms >= tm.seed_ms and tm.n_units > 0 and tm.n_triangles == 1
    t2 = _lib.M2STimings()
    with BandField.from_spheres(Grid([0.0] * 3, [1.0] * 3, [16] * 3), host_a, 3.0, 1.0, timings=t2) as f:
        assert t2.total_ms > 0 and t2.n_units == f.count == tm.n_units
    with pytest.raises(M2SError):
        BandField.from_spheres(Grid([0.0] * 3, [1.0] * 3, [16] * 3), host_a, [1.0, 2.0], 1.0)      # one radius per shape
    with pytest.raises(M2SError):
        BandField.from_spheres(Grid([0.0] * 3, [1.0] * 3, [16] * 3), host_a, 1.0, -1.0)


# ---- 9. the consumers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cc,std,src", CONSUMERS)
def test_consumers_run_clean_on_the_gpu(tmp_path, cc, std, src):
    r = subprocess.run([build_consumer(tmp_path, cc, std, src), "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
