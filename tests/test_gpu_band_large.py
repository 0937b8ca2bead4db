"""The band calls on grids past 2^32 points, where every cell index L = k + j * nz + i * ny * nz of the upper part needs more than 32 bits:
m2s_band_create / m2s_band_export, m2s_band_csg, m2s_band_redistance, m2s_band_filter, m2s_band_resample, m2s_band_components,
m2s_band_select, m2s_band_advect, m2s_narrow_band_sdf, m2s_voxelize, the chain from a mesh to an isosurface and the chain advect ->
select -> measure on G33 = 2048 x 2048 x 1100 (4.61e9 points, 72 089 600 mask words; L = 2^32 is
the point (1906, 1027, 796)), and create / export / csg / redistance on G34 = 4096 x 4096 x 1100 (1.845e10 points, above 2^34:
288 358 400 mask words and 587 202 560 sign words, both above 2^28, so every grid-stride loop behind a launch capped at 2^20
workgroups takes a second trip).

The dense numpy models cannot run at such sizes.  The active cells sit in two boxes, one across L = 2^32 (at the origin on G34) and one
that ends with the grid, and the models run on a window around each (tests/band_window.py has the rule per call for when that is exact
and checks it; tests/test_band_window_cpu.py proves the rules on small grids, and that these layouts meet the conditions asserted here).
Cells, values and sign masks are built on the device with torch; no host array is sized by the grid.  The result's sign mask is compared
on the device over every word: outside the windows it must be the inputs' masks combined with torch (bits at k >= nz zero).
Every comparison is exact equality of bits."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import band_advect_model as am
import band_components_model as ccm
import band_csg_model as cm
import band_filter_model as fm
import band_isosurface_model as bim
import band_measure_model as mm
import band_query_model as bqm
import band_redistance_model as rm
import band_resample_model as rsm
import band_window as bw
import grid_query_model as gqm
import isosurface_model as im
import voxel_model as vm
from mesh_to_sdf_amd import BandField, CsgOp, FilterKind, Grid, Mesh, SampleMode, SignMethod, Topology, _lib, band_isosurface
from test_gpu_band_csg import _icosphere
from test_gpu_band_isosurface import _same_mesh

F = np.float32
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPS = (CsgOp.Union, CsgOp.Intersection, CsgOp.Difference)
MODES = [SampleMode.Snap, SampleMode.Trilinear, SampleMode.Tetrahedral]
SIGNS = [SignMethod.Raycast, SignMethod.Normal]
GIB = 1 << 30


def _np(x):
    if hasattr(x, "cpu"):
        if x.dtype == getattr(torch, "uint32", None):
            x = x.view(torch.int32)
        x = x.cpu().numpy()
    return np.asarray(x)


def _need_free(gib, what):
    free, _ = torch.cuda.mem_get_info()
    print(f"{what}: {free / GIB:.1f} GiB of device memory free")
    if free < gib * GIB:
        pytest.skip(f"less than {gib} GiB of device memory free")


def _patch(mask, windows, bands):
    """The windows' bits of a device sign mask int32[nx, ny, ceil(nz / 32)] replaced by the Bands' (only the windows' words travel)."""
    for w, b in zip(windows, bands):
        sl = w.word_slices()
        cur = mask[sl].cpu().numpy().view(np.uint32)
        mask[sl] = torch.as_tensor(w.put_bits(cur, cm.unpack_bits(w.shape, b.bits)).view(np.int32), device=DEV)


def _clear_tail(mask, nz):
    if nz % 32:
        mask[:, :, -1] &= (1 << (nz % 32)) - 1


def _mask(lt, bands, slabs=(), windows=None):
    """A device sign mask: zeros, the slabs' words set to their patterns (in the last word of a row that sets bits at k >= nz too, which
    the library must ignore), then the windows' bits.  The slabs lie outside every window.  windows: those of `bands`, where they are
    not the layout's."""
    nx, ny, nz = lt.big
    windows = lt.windows if windows is None else windows
    m = torch.zeros((nx, ny, (nz + 31) // 32), dtype=torch.int32, device=DEV)
    for sl, pattern in slabs:
        m[sl] = pattern
    for w in windows:
        assert not m[w.word_slices()].any(), "a slab crosses a window"
    _patch(m, windows, bands)
    return m


def _grid(lt):
    return Grid(list(lt.first), list(lt.cell), list(lt.big))


def _field(lt, grid, bands, mask, windows=None):
    cells, dist = bw.embed(lt.windows if windows is None else windows, bands)
    return BandField(grid, torch.as_tensor(cells, device=DEV), torch.as_tensor(dist, device=DEV),
                     background=(float(bands[0].bg_in), float(bands[0].bg_out)), inside=mask)


def _check(field, lt, want, want_mask, what, created=False, windows=None, min_cells=50):
    """A handle against the window Bands embedded and the expected device sign mask (None: no mask was given, the export is zeros).
    windows: those of `want`, where they are not the layout's.  min_cells: what every window must contribute (more than that)."""
    cells, dist = bw.embed(lt.windows if windows is None else windows, want)
    for b in want:
        assert b.cells.size > min_cells, f"{what}: a window contributes {b.cells.size} cells"
    nb = field.to_band()
    assert nb.count == field.count == cells.size, f"{what}: {nb.count} cells, the windows hold {cells.size}"
    got_cells, got_dist = _np(nb.cells).astype(np.int64), _np(nb.distances)
    assert np.array_equal(got_cells, cells), f"{what}: cells differ, first at {int(np.flatnonzero(got_cells != cells)[0])}"
    differ = got_dist.view(np.uint32) != dist.view(np.uint32)
    assert not differ.any(), f"{what}: {int(differ.sum())} distances differ, first at cell {int(cells[np.flatnonzero(differ)[0]])}"
    bits = nb.bits.view(torch.int32)
    assert bits.is_cuda and tuple(bits.shape) == (lt.big[0], lt.big[1], (lt.big[2] + 31) // 32)
    if want_mask is None:
        assert not bits.any(), f"{what}: a handle without a sign mask exports set bits"
    else:
        wrong = int((bits != want_mask).sum()) if not torch.equal(bits, want_mask) else 0
        assert wrong == 0, f"{what}: {wrong} sign words differ"
    del bits, nb
    words = (lt.total + 63) // 64
    n, nbytes = C.c_uint64(0), C.c_uint64(0)
    assert _lib.lib().m2s_band_info(field._h, None, C.byref(n), C.byref(nbytes)) == _lib.M2S_OK
    per_word = 24 if (want_mask is not None or not created) else 16             # a result always has a sign mask
    assert n.value == cells.size and nbytes.value == per_word * words + 4 * n.value == field.device_bytes, what
    assert field.background == (float(want[0].bg_in), float(want[0].bg_out)), what


def _unmasked(bands):
    return [cm.Band(b.shape, b.cells, b.distances, None, b.bg_out, b.bg_in) for b in bands]


# ---- G33 -----------------------------------------------------------------------------------------------------------------------------------
class Case:
    pass


@pytest.fixture(scope="module")
def g33():
    """The layout, the grid and the three device sign masks (0.59 GB each), shared and left unchanged."""
    _need_free(16, "G33")
    c = Case()
    c.lt = lt = bw.layout_g33()
    assert lt.total > 2 ** 32
    big_a = lt.windows[0].to_big(lt.a[0].cells)
    assert (big_a < 2 ** 32).sum() > 50 and (big_a >= 2 ** 32).sum() > 50, "the first box does not straddle L = 2^32"
    assert int(lt.windows[1].to_big(lt.a[1].cells)[-1]) == lt.total - 1, "the second box does not end with the grid"
    c.grid = _grid(lt)
    # two different sets of slabs far from the boxes; they overlap in part, so that |, & and & ~ all differ from both inputs
    c.mask_a = _mask(lt, lt.a, ((slice(100, 110), -1), ((slice(None), slice(700, 703)), 0x5A5A5A5A)))
    c.mask_b = _mask(lt, lt.b, ((slice(105, 120), -1), ((slice(None), slice(701, 705)), 0x0FF00FF0)))
    c.mask_w = _mask(lt, lt.where)
    c.mask_f = _mask(lt, lt.full)
    yield c
    del c.mask_a, c.mask_b, c.mask_w, c.mask_f
    torch.cuda.empty_cache()


def test_create_and_export_round_trip(g33):
    """export(create(lists)) == lists in cells, values and sign mask (the bits at k >= nz zero), and device_bytes by the header's formula."""
    lt = g33.lt
    want = g33.mask_a.clone()
    _clear_tail(want, lt.big[2])
    assert not torch.equal(want, g33.mask_a), "the slab sets no bit at k >= nz"
    with _field(lt, g33.grid, lt.a, g33.mask_a) as f:
        _check(f, lt, lt.a, want, "G33 create with a mask", created=True)
        assert f.device_bytes == 24 * 72089600 + 4 * f.count
    del want
    with _field(lt, g33.grid, lt.b, None) as f:
        _check(f, lt, lt.b, None, "G33 create without a mask", created=True)
        assert f.device_bytes == 16 * 72089600 + 4 * f.count


@pytest.mark.parametrize("masked", [True, False], ids=["masks", "no-masks"])
def test_csg(g33, masked):
    """Union, intersection and difference, of A and B and of A with itself.  Outside the windows the result's sign mask is sA | sB,
    sA & sB or sA & ~sB of the input masks, which states s on the inactive points independently of the model."""
    lt = g33.lt
    wa, wb = (lt.a, lt.b) if masked else (_unmasked(lt.a), _unmasked(lt.b))
    ma, mb = (g33.mask_a, g33.mask_b) if masked else (None, None)
    with _field(lt, g33.grid, wa, ma) as fa, _field(lt, g33.grid, wb, mb) as fb:
        for second, wsecond, msecond, name in ((fb, wb, mb, "A op B"), (fa, wa, ma, "A op A")):
            for op in OPS:
                want = [cm.csg(x, y, int(op)) for x, y in zip(wa, wsecond)]
                if masked:
                    beyond = {CsgOp.Union: ma | msecond, CsgOp.Intersection: ma & msecond, CsgOp.Difference: ma & ~msecond}[op]
                    _clear_tail(beyond, lt.big[2])
                else:
                    beyond = torch.zeros_like(g33.mask_a)
                _patch(beyond, lt.windows, want)
                with fa.csg(second, op) as fr:
                    assert fr.count == sum(b.cells.size for b in want)
                    _check(fr, lt, want, beyond, f"G33 {name} {op.name} masked {masked}")
                del beyond


@pytest.mark.parametrize("widths", bw.G33_WIDTHS, ids=["two-sided", "one-sided"])
def test_redistance(g33, widths):
    lt = g33.lt
    ext, inn = widths
    for win, band in zip(lt.windows, lt.a):
        bw.check_redistance(win, band, lt.cell, ext, inn)
    parts = [rm.redistance(b, lt.cell, ext, inn) for b in lt.a]
    assert all(p[1].n_frozen > 0 for p in parts), "a window has no frozen cell"
    info = bw.sum_redistance([p[1] for p in parts])
    want_mask = g33.mask_a.clone()                               # redistance keeps s on every grid point
    _clear_tail(want_mask, lt.big[2])
    _patch(want_mask, lt.windows, [p[0] for p in parts])
    with _field(lt, g33.grid, lt.a, g33.mask_a) as f, f.redistance((inn, ext)) as r:
        ri = r.redistance_info
        assert (ri.sweeps, int(ri.converged), ri.n_frozen, ri.n_open, ri.n_candidates) == tuple(info), f"info {ri}, the windows give {info}"
        _check(r, lt, [p[0] for p in parts], want_mask, f"G33 redistance {widths}")


@pytest.mark.parametrize("restricted", [False, True], ids=["everywhere", "where"])
@pytest.mark.parametrize("kind", list(FilterKind), ids=lambda k: k.name)
def test_filter(g33, kind, restricted):
    lt = g33.lt
    for i, win in enumerate(lt.windows):
        bw.check_filter(win, lt.a[i], lt.where[i] if restricted else None)
        region = cm.dense(lt.a[i])[0] & cm.dense(lt.where[i])[2]
        assert 0 < region.sum() < lt.a[i].cells.size, "the region does not cut through the box"
    parts = [fm.band_filter(b, lt.cell, int(kind), 2, lt.where[i] if restricted else None) for i, b in enumerate(lt.a)]
    assert all(p[1].n_changed > 0 for p in parts), "a window has no changed cell"
    if restricted:
        assert all(p[1].n_changed < b.cells.size for p, b in zip(parts, lt.a))
    info = bw.sum_filter([p[1] for p in parts])
    want_mask = g33.mask_a.clone()
    _clear_tail(want_mask, lt.big[2])
    _patch(want_mask, lt.windows, [p[0] for p in parts])
    with _field(lt, g33.grid, lt.a, g33.mask_a) as f, (_field(lt, g33.grid, lt.where, g33.mask_w) if restricted else contextlib.nullcontext()) as w:
        with f.filter(kind, 2, where=w) as r:
            fi = r.filter_info
            assert (fi.passes, fi.n_changed, fi.n_sign_flips, fi.n_nonfinite) == (info.passes, info.n_changed, info.n_sign_flips, info.n_nonfinite), (fi, info)
            assert F(fi.max_change).view(np.uint32) == F(info.max_change).view(np.uint32), (fi, info)
            _check(r, lt, [p[0] for p in parts], want_mask, f"G33 filter {kind.name} restricted {restricted}")


# ---- components, select, advect ----------------------------------------------------------------------------------------------------------------
SLABS_OUTSIDE = ((slice(100, 110), -1), ((slice(None), slice(700, 703)), 0x5A5A5A5A))     # as mask_a's: far from every window of a G33 case


@pytest.fixture(scope="module")
def blobs(g33):
    """The bands of many components (band_window.blob_bands) and the device sign mask that holds their own bits and nothing else."""
    c = Case()
    c.bands = bw.blob_bands(g33.lt)
    c.mask = _mask(g33.lt, c.bands)
    yield c
    del c.mask
    torch.cuda.empty_cache()


def _check_components(got, want, what):
    """A Components of the library against the windows' merged (band_window.merge_components): labels, count and the five statistics."""
    assert got.count == want.count, f"{what}: {got.count} components, the windows hold {want.count}"
    labels = _np(got.labels).view(np.uint32)
    differ = labels != want.labels
    assert not differ.any(), f"{what}: {int(differ.sum())} labels differ, first at list place {int(np.flatnonzero(differ)[0])}"
    for name, g, w in (("first_cell", got.first_cell, want.first_cell), ("n_cells", got.n_cells, want.n_cells), ("n_negative", got.n_negative, want.n_negative),
                       ("box_lo", got.box_lo, want.lo), ("box_hi", got.box_hi, want.hi)):
        assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {name} differs, first at component {int(np.flatnonzero((g != w).reshape(want.count, -1).any(1))[0])}"


@pytest.mark.parametrize("connectivity", ccm.CONNECTIVITIES)
def test_components(g33, blobs, connectivity):
    """Labels, count and the statistics of bands that fall into dozens of components per window, the largest with cells on both sides
    of L = 2^32: the neighbour M = L + di * si + dj * sj + dk and its rank, first_cell as uint64, the boxes from (i, j, k)."""
    lt = g33.lt
    counts = {}
    for conn in ccm.CONNECTIVITIES:
        parts = [ccm.components(b, conn) for b in blobs.bands]
        assert all(p.count >= 3 for p in parts), "a window holds fewer than 3 components"
        counts[conn] = sum(p.count for p in parts)
        if conn == connectivity:
            for win, b in zip(lt.windows, blobs.bands):
                bw.check_components(win, b)
            want = bw.merge_components(lt.windows, blobs.bands, parts)[0]
    assert counts[6] > counts[18] > counts[26], counts
    cells = bw.embed(lt.windows, blobs.bands)[0]
    L = cells[want.labels == int(np.argmax(want.n_cells))]
    assert (L < 2 ** 32).sum() > 50 and (L >= 2 ** 32).sum() > 50, "no component has cells on both sides of L = 2^32"
    assert (want.first_cell >= 2 ** 32).sum() >= 3 and (want.first_cell < 2 ** 32).sum() >= 3
    with _field(lt, g33.grid, blobs.bands, blobs.mask) as f:
        _check_components(f.components(connectivity), want, f"G33 components {connectivity}")
        o = _lib.M2SOpts()
        o.struct_size, o.device, o.mem_kind = C.sizeof(o), -1, _lib.MEM_DEVICE
        n = C.c_uint64(0)
        co = _lib.M2SBandComponentsOpts(C.sizeof(_lib.M2SBandComponentsOpts), connectivity)
        assert _lib.lib().m2s_band_components(f._h, C.byref(co), C.byref(o), None, None, 0, C.byref(n)) == _lib.M2S_OK     # the count-only call
        assert n.value == want.count


def test_select(g33, blobs):
    """Every other 18-component erased, on windows of whole rows.  The input mask has an inside run of 800 points on every row through
    a box (below and above the first box, below the second, which ends with its rows), so that k_sel_mask's search for the nearest
    active cell crosses a dozen mask words without one, and slabs far from the windows, with bits at k >= nz, that must come back
    with those bits cleared and nothing else changed."""
    lt = g33.lt
    rows = bw.select_windows(lt)
    bands = bw.select_bands(lt, blobs.bands, bw.G33_RUNS)
    for win, b in zip(rows, bands):
        bw.check_select(win, b)
    parts = [ccm.components(b, 18) for b in bands]
    merged, maps = bw.merge_components(rows, bands, parts)
    keep = np.arange(merged.count) % 2 == 0
    res = [ccm.select(b, p.labels, keep[m]) for b, p, m in zip(bands, parts, maps)]
    assert all(r[1].n_dropped > 0 and r[1].n_sign_cleared > 64 and r[1].n_cells > 50 for r in res), [r[1] for r in res]
    mask = _mask(lt, bands, SLABS_OUTSIDE, windows=rows)
    want_mask = mask.clone()
    _clear_tail(want_mask, lt.big[2])
    assert not torch.equal(want_mask, mask), "the slabs set no bit at k >= nz"
    _patch(want_mask, rows, [r[0] for r in res])
    with _field(lt, g33.grid, bands, mask, windows=rows) as f:
        for labels in (torch.as_tensor(merged.labels.view(np.int32), device=DEV), f.components(18)):
            with f.select(labels, keep) as r:
                assert tuple(r.select_info) == tuple(bw.sum_select([x[1] for x in res])), f"info {r.select_info}, the windows give {[x[1] for x in res]}"
                _check(r, lt, [x[0] for x in res], want_mask, "G33 select", windows=rows)
    del mask, want_mask


def _advect_info_is(ai, info, what):
    assert (ai.steps, ai.n_moving, ai.n_changed, ai.n_sign_flips, ai.n_nonfinite) == (info.steps, info.n_moving, info.n_changed, info.n_sign_flips, info.n_nonfinite), \
        f"{what}: info {ai}, the windows give {info}"
    assert F(ai.max_change).view(np.uint32) == F(info.max_change).view(np.uint32) and F(ai.max_cfl).view(np.uint32) == F(info.max_cfl).view(np.uint32), \
        f"{what}: info {ai}, the windows give {info}"


def _advected(lt, bands, kind, background=None):
    """Three steps of the windows' bands by band_window.trig_field -> (the field in the big grid's list order on the device, dt, the
    models' (Band, Info) per window)."""
    dt = F(0.5 * min(lt.cell))
    fields = [bw.trig_field(win, b, kind, 20 + i) for i, (win, b) in enumerate(zip(lt.windows, bands))]
    for win, b in zip(lt.windows, bands):
        bw.check_advect(win, b)
    parts = [am.band_advect(b, lt.cell, kind, f, dt, 3, background) for b, f in zip(bands, fields)]
    assert all(0 < p[1].n_moving < b.cells.size and p[1].n_changed > 50 for p, b in zip(parts, bands)), [p[1] for p in parts]
    return torch.as_tensor(bw.embed_field(lt.windows, bands, fields), device=DEV), float(dt), parts


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "no-mask"])
@pytest.mark.parametrize("kind", am.KINDS, ids=["velocity", "speed"])
def test_advect(g33, kind, masked):
    """Three Jacobi steps of both kinds: the neighbour table comes from the 64-bit walk, the field and the two value buffers are in
    list order across L = 2^32, and the result's mask and offsets are copies of the input's."""
    lt = g33.lt
    bands = lt.a if masked else _unmasked(lt.a)
    background = None if kind == am.VELOCITY else (1.25, 0.375)                  # (outside, inside)
    given, dt, parts = _advected(lt, bands, kind, background)
    if masked:
        want_mask = g33.mask_a.clone()
        _clear_tail(want_mask, lt.big[2])
    else:
        want_mask = torch.zeros_like(g33.mask_a)
    _patch(want_mask, lt.windows, [p[0] for p in parts])
    with _field(lt, g33.grid, bands, g33.mask_a if masked else None) as f:
        with f.advect(dt, 3, background=None if background is None else (background[1], background[0]),
                      **{"velocity" if kind == am.VELOCITY else "speed": given}) as r:
            _advect_info_is(r.advect_info, bw.sum_advect([p[1] for p in parts]), f"G33 advect kind {kind} masked {masked}")
            _check(r, lt, [p[0] for p in parts], want_mask, f"G33 advect kind {kind} masked {masked}")
    del want_mask


def test_the_chain_advect_select_measure(g33, blobs):
    """advect -> components(26) -> select of the largest component -> measure, every handle on the device: a result made past 2^32 is
    consumed past 2^32.  The models run on the windows: advect on the layout's, select on windows of whole rows; the component that
    is left has cells on both sides of L = 2^32 and lies in the first window, whose box the measure model takes."""
    lt = g33.lt
    w, rows = lt.windows, bw.select_windows(lt)
    given, dt, moved = _advected(lt, blobs.bands, am.VELOCITY)
    on_rows = [bw.rehome(m[0], win, row) for m, win, row in zip(moved, w, rows)]
    for row, b in zip(rows, on_rows):
        bw.check_components(row, b)
        bw.check_select(row, b)
    parts = [ccm.components(b, 26) for b in on_rows]
    merged, maps = bw.merge_components(rows, on_rows, parts)
    keep = np.zeros(merged.count, bool)
    keep[int(np.argmax(merged.n_cells))] = True                                 # the first of the largest, as Components.largest
    res = [ccm.select(b, p.labels, keep[m]) for b, p, m in zip(on_rows, parts, maps)]
    left = rows[0].to_big(res[0][0].cells)
    assert res[1][1].n_cells == 0 and (left < 2 ** 32).sum() > 50 and (left >= 2 ** 32).sum() > 50 and all(r[1].n_dropped > 50 for r in res)
    measured = mm.measure(lt.big, lt.cell, left, res[0][0].distances, box=(w[0].lo, w[0].shape))
    assert int(measured.n_triangles[0]) > 50
    want_mask = blobs.mask.clone()
    _patch(want_mask, w, [m[0] for m in moved])
    with _field(lt, g33.grid, blobs.bands, blobs.mask) as f, f.advect(dt, 3, velocity=given) as fa:
        _advect_info_is(fa.advect_info, bw.sum_advect([m[1] for m in moved]), "the chain's advect")
        _check(fa, lt, [m[0] for m in moved], want_mask, "the chain's advect")
        comps = fa.components(26)
        _check_components(comps, merged, "the chain's components")
        assert np.array_equal(comps.largest(1), np.flatnonzero(keep))
        with fa.select(comps, comps.largest(1)) as fs:
            assert tuple(fs.select_info) == tuple(bw.sum_select([r[1] for r in res])), f"info {fs.select_info}, the windows give {[r[1] for r in res]}"
            _patch(want_mask, rows, [r[0] for r in res])
            _check(fs, lt, [r[0] for r in res], want_mask, "the chain's select", windows=rows, min_cells=-1)
            m = fs.measure()
            for name in mm.INT_FIELDS:
                x = getattr(measured, name)[0]
                x = tuple(int(v) for v in x) if name == "moment_q" else int(x)
                assert getattr(m, name) == x, f"the chain's measure: {name} = {getattr(m, name)}, the model has {x}"
            assert m.closed == mm.closed(measured) and m.euler == mm.euler(measured)
    del want_mask


# ---- resample ------------------------------------------------------------------------------------------------------------------------------
def _small_check(field, want, info, what):
    """A handle on a small grid against the model's (Band, Info), every array on the host."""
    nb = field.to_band()
    got = cm.Band(want.shape, _np(nb.cells).astype(np.int64), _np(nb.distances), _np(nb.bits).view(np.uint32), field.background[1], field.background[0])
    assert got.cells.size == want.cells.size == field.count and np.array_equal(got.cells, want.cells), f"{what}: cells differ"
    differ = got.distances.view(np.uint32) != want.distances.view(np.uint32)
    assert not differ.any(), f"{what}: {int(differ.sum())} distances differ"
    assert cm.same(got, want), f"{what}: sign mask or backgrounds differ"
    assert tuple(field.resample_info) == tuple(info), f"{what}: info {field.resample_info}, the model has {info}"


@pytest.mark.parametrize("mode", MODES, ids=lambda m: m.name)
def test_resample_from_g33_onto_a_small_grid(g33, mode):
    """A small target over each box, under band_resample_model.move()'s turn and scale about the box's centre: the source cells the
    walk fetches lie on both sides of L = 2^32 and at the end of the grid.  Expected: band_window.resample_window, whose values and
    support are band_query_model.sample's on the full-size grid."""
    lt = g33.lt
    spec = rsm.GridSpec(lt.first, lt.cell, lt.big)
    cells, dist = bw.embed(lt.windows, lt.full)
    x = bw.sparse_source(lt.big, cells, dist, bw.SparseBits(lt.windows, lt.full), lt.full[0].bg_out, lt.full[0].bg_in)
    with _field(lt, g33.grid, lt.full, g33.mask_f) as f:
        for i in range(len(lt.sites)):
            fwd, _, small = bw.placement(lt, i)
            want, info = bw.resample_window(x, spec, small, bw.Window(small.shape, (0, 0, 0), small.shape), *rsm.similarity(fwd), int(mode))
            assert info.n_cells > 50, f"site {i}: the model's result has {info.n_cells} cells"
            with f.resample(Grid(list(small.first), list(small.cell), list(small.shape)), fwd, mode=mode) as r:
                _small_check(r, want, info, f"G33 -> small, site {i}, {mode.name}")


@pytest.mark.parametrize("mode", MODES, ids=lambda m: m.name)
def test_resample_from_a_small_grid_into_g33(g33, mode):
    """The inverse placement: a random band on the small grid lands in G33, across L = 2^32 and (cut by three faces) in the high
    corner.  The expected result is a window of the target; beyond it no target point is on the source box."""
    lt = g33.lt
    spec = rsm.GridSpec(lt.first, lt.cell, lt.big)
    for i in range(len(lt.sites)):
        _, inv, small = bw.placement(lt, i)
        Y = bw.small_band(lt, i)
        win = bw.target_box_of_source(small, spec, inv)
        y = bw.sparse_source(small.shape, Y.cells, Y.distances, Y.bits, Y.bg_out, Y.bg_in)
        want, info = bw.resample_window(y, small, spec, win, *rsm.similarity(inv), int(mode))
        big = win.to_big(want.cells)
        if i == 0:
            assert (big < 2 ** 32).sum() > 50 and (big >= 2 ** 32).sum() > 50, "the result does not land on both sides of L = 2^32"
        else:
            assert int(big[0]) > 2 ** 32 and any(win.at_face(a, 1) for a in range(3))
        want_mask = torch.zeros_like(g33.mask_a)
        _patch(want_mask, [win], [want])
        bits = torch.as_tensor(np.ascontiguousarray(Y.bits).view(np.int32), device=DEV)
        with BandField(Grid(list(small.first), list(small.cell), list(small.shape)), torch.as_tensor(Y.cells, device=DEV),
                       torch.as_tensor(Y.distances, device=DEV), background=(float(Y.bg_in), float(Y.bg_out)), inside=bits) as fy:
            with fy.resample(g33.grid, inv, mode=mode) as r:
                assert tuple(r.resample_info) == tuple(info), f"site {i}: info {r.resample_info}, the model has {info}"
                _check(r, lt, [want], want_mask, f"small -> G33, site {i}, {mode.name}", windows=[win])
        del want_mask


def test_resample_snap_identity_gives_the_band_back(g33):
    """Consequence 1 of the header at full size: SNAP, the identity map and T == Gs return X in every bit, the sign mask being s_X on
    every point.  No model is needed for the band; n_open is the windows' count of open faces."""
    lt = g33.lt
    want_mask = g33.mask_a.clone()
    _clear_tail(want_mask, lt.big[2])
    _patch(want_mask, lt.windows, [bw.sign_band(b) for b in lt.a])
    n = sum(b.cells.size for b in lt.a)
    with _field(lt, g33.grid, lt.a, g33.mask_a) as f, f.resample(g33.grid, None, mode=SampleMode.Snap) as r:
        assert tuple(r.resample_info) == (n, 0, 0, sum(bw.open_faces(b) for b in lt.a)), r.resample_info
        _check(r, lt, lt.a, want_mask, "G33 SNAP identity")


# ---- narrow bands and voxelization of a mesh -------------------------------------------------------------------------------------------------
NB_WIDTHS = (2.0 * 2.0 ** -7, 2.5 * 2.0 ** -7)                   # (interior, exterior): 2 and 2.5 cells of hx
NB_RADIUS = 6.0 * 2.0 ** -7                                      # 6 cells of hx, 3 of hy, 12 of hz
NB_CENTRES = ((1906.37, 1027.21, 796.4), (2043.3, 2044.6, 1091.7))   # in cells: across L = 2^32, and cut by the three high faces
NB_SHIFT = (2.3, 1.2, 3.4)                                       # the chain's second copy, in cells


def _two_spheres(shift=(0.0, 0.0, 0.0)):
    """One mesh of two closed components, 320 triangles each, as device tensors."""
    v, idx = [], []
    for c in NB_CENTRES:
        centre = [bw.G33_FIRST[a] + (c[a] + shift[a]) * bw.G33_CELL[a] for a in range(3)]
        sv, si = _icosphere(NB_RADIUS, centre, subdivisions=2)
        idx.append(si.astype(np.int64) + sum(len(x) for x in v))
        v.append(sv)
    v, idx = np.concatenate(v).astype(F), np.concatenate(idx)
    return v, idx


def _sphere_windows(margin, reach_cells):
    """A window of G33 around each sphere (and its shifted copy): the spheres' cells grown by `reach_cells` of hx worth of distance and
    then by `margin` layers per axis, cut at the grid."""
    out = []
    for c in NB_CENTRES:
        lo, hi = [], []
        for a in range(3):
            r = (NB_RADIUS + reach_cells * bw.G33_CELL[0]) / bw.G33_CELL[a]
            lo.append(max(int(np.floor(c[a] - r)) - 1 - margin[a], 0))
            hi.append(min(int(np.ceil(c[a] + NB_SHIFT[a] + r)) + 2 + margin[a], bw.G33[a]))
        out.append(bw.Window(bw.G33, lo, [h - l for l, h in zip(lo, hi)]))
    bw.check_disjoint(out)
    return out


def _window_grid(win):
    """The window as a Grid of its own, first' = first + lo * size.  On the dyadic G33 its cell centres first' + (float)i * size are
    the big grid's, bit for bit, which is asserted here before anything relies on it."""
    first = [bw.G33_FIRST[a] + win.lo[a] * bw.G33_CELL[a] for a in range(3)]
    for a in range(3):
        mine = F(first[a]) + np.arange(win.shape[a]).astype(F) * F(bw.G33_CELL[a])
        theirs = F(bw.G33_FIRST[a]) + np.arange(win.lo[a], win.hi[a]).astype(F) * F(bw.G33_CELL[a])
        assert mine.dtype == F and np.array_equal(mine.view(np.uint32), theirs.view(np.uint32)), "the window's cell centres are not the big grid's"
    return Grid(first, list(bw.G33_CELL), list(win.shape))


def _dense_band(mesh, win, sign, bg):
    """The expected narrow band in a window: the dense call on the window grid, filtered to the widths, as a Band whose mask is the
    active cells, which is what bits_out holds.  The distances depend on the cell centres alone.  One grid-dependent quantity enters the
    Raycast sign (sign.hip, mark_line): a crossing's cell is floor(t / size) with t measured from the grid's first layer, so a window
    grid rounds t otherwise and may put a crossing that lies within an ulp of t of a cell centre on the other side of it.  That takes a
    surface within about 1e-4 cells of a centre on one axis, and the two-of-three vote over the axes outvotes a single such case; the
    spheres here, at non-dyadic centres, have none, which the exact comparison confirms."""
    D = _np(mesh.generate_grid_sdf(_window_grid(win), sign)).reshape(-1).astype(F)
    active = (F(-NB_WIDTHS[0]) <= D) & (D <= F(NB_WIDTHS[1]))
    a3 = active.reshape(win.shape)
    for axis in range(3):
        for side in (0, 1):
            assert win.at_face(axis, side) or not bw._layers(a3, axis, side, 1).any(), "the band reaches the window's side"
    return cm.Band(win.shape, np.flatnonzero(active), D[active], cm.pack_bits(win.shape, a3), bg[0], bg[1]), D


@pytest.fixture(scope="module")
def spheres(g33):
    v, idx = _two_spheres()
    with Mesh(torch.as_tensor(v, device=DEV), Topology.TriangleList(torch.as_tensor(idx, device=DEV))) as mesh:
        yield v, idx, mesh


@pytest.mark.parametrize("sign", SIGNS, ids=lambda s: s.name)
def test_narrow_band_sdf(g33, spheres, sign):
    """cells, distances and bits_out on the dyadic G33 against the dense call on the window grids, filtered.  Algorithm 1 is left out:
    it walks the dense grid into a workspace of 4 bytes per point (run_narrow_band: ws.take<float>(cells)), 18 GB here, which is what
    the band exists to avoid."""
    _, _, mesh = spheres
    wins = _sphere_windows((2, 2, 2), NB_WIDTHS[1] / bw.G33_CELL[0])
    want = [_dense_band(mesh, w, sign, (NB_WIDTHS[1], NB_WIDTHS[0]))[0] for w in wins]
    cells, dist = bw.embed(wins, want)
    assert all(b.cells.size > 50 for b in want) and (cells < 2 ** 32).sum() > 50 and (cells >= 2 ** 32).sum() > 50
    assert int(wins[1].to_big(want[1].cells)[0]) > 2 ** 32 and all(wins[1].at_face(a, 1) for a in range(3))
    nb =mesh.narrow_band_sdf(g33.grid, NB_WIDTHS, sign, bits=True)
    got = _np(nb.cells).astype(np.int64)
    assert nb.count == cells.size, f"{nb.count} cells, the windows hold {cells.size}"
    assert sum(p.size for p in bw.split(wins, got)) == got.size                    # none outside the windows
    assert np.array_equal(got, cells), "cells differ"
    differ = _np(nb.distances).view(np.uint32) != dist.view(np.uint32)
    assert not differ.any(), f"{int(differ.sum())} distances differ, first at cell {int(cells[np.flatnonzero(differ)[0]])}"
    want_mask = torch.zeros_like(g33.mask_a)
    _patch(want_mask, wins, want)
    assert torch.equal(nb.bits.view(torch.int32), want_mask), "bits_out differs"


@pytest.mark.parametrize("solid", [False, True], ids=["surface", "solid"])
def test_voxelize(g33, spheres, solid):
    """SURFACE against voxel_model.surface on the windows; SOLID is that or the Raycast sign of the dense call on the window grid.  The
    bits outside the windows are compared on the device; the 4.6 GB occupancy array is not asked for."""
    v, idx, mesh = spheres
    wins = _sphere_windows((2, 2, 2), 1.0)
    tris = vm.triangles_of(v, idx.astype(np.uint32))
    want = []
    for w in wins:
        g = _window_grid(w)
        occ = vm.surface(tris, np.array(g.get_first_cell(), F), np.array(g.get_cell_size(), F), w.shape)[0].astype(bool)
        if solid:
            occ |= np.signbit(_np(mesh.generate_grid_sdf(g, SignMethod.Raycast))).reshape(w.shape)
        assert occ.sum() > 50
        want.append(cm.Band(w.shape, np.flatnonzero(occ), np.zeros(int(occ.sum()), F), cm.pack_bits(w.shape, occ), 0.5, 0.5))
    got = mesh.voxelize(g33.grid, solid, bits=True, cells=True, occupancy=False)
    cells = bw.embed(wins, want)[0]
    assert got.count == cells.size and np.array_equal(_np(got.cells).astype(np.int64), cells), "cells differ"
    assert (cells < 2 ** 32).sum() > 50 and (cells >= 2 ** 32).sum() > 50
    want_mask = torch.zeros_like(g33.mask_a)
    _patch(want_mask, wins, want)
    assert torch.equal(got.bits.view(torch.int32), want_mask), "bits differ"


# ---- the chain -----------------------------------------------------------------------------------------------------------------------------
def test_the_chain_mesh_to_isosurface(g33, spheres):
    """mesh -> narrow_band_sdf (with bits_out) -> band_create -> union with a second, shifted copy -> redistance -> filter
    (MEAN_CURVATURE, restricted by `where`: the copy's inside) -> resample SNAP back onto G33 -> export -> band_isosurface and
    band_sample, every handle staying on the device.  Expected: the same chain through the numpy models on the windows, started from
    the dense call on the window grids.  bits_out marks the active cells, so as a sign mask it calls the deep interior outside: the
    band does not bracket its zero set there and n_open > 0, which the models repeat."""
    lt = g33.lt
    _, _, mesh = spheres
    ext, inn = bw.G33_WIDTHS[0]
    margin = bw.redistance_margin(lt.big, lt.cell, ext, inn)
    wins = _sphere_windows(margin, NB_WIDTHS[1] / bw.G33_CELL[0])
    v2, idx2 = _two_spheres(NB_SHIFT)
    bg = (NB_WIDTHS[1], NB_WIDTHS[0])                                            # (outside, inside)
    with Mesh(torch.as_tensor(v2, device=DEV), Topology.TriangleList(torch.as_tensor(idx2, device=DEV))) as mesh2:
        # the models
        stages = []
        for w in wins:
            n1, n2 = _dense_band(mesh, w, SignMethod.Raycast, bg)[0], _dense_band(mesh2, w, SignMethod.Raycast, bg)[0]
            u = cm.csg(n1, n2, cm.UNION)
            bw.check_redistance(w, u, lt.cell, ext, inn)
            r, ri = rm.redistance(u, lt.cell, ext, inn)
            bw.check_filter(w, r, n2)
            f, fi = fm.band_filter(r, lt.cell, fm.MEAN_CURVATURE, 2, n2)
            region = cm.dense(r)[0] & cm.dense(n2)[2]
            assert ri.n_frozen > 0 and fi.n_changed > 0 and 0 < region.sum() < r.cells.size and f.cells.size > 50
            stages.append((n1, n2, u, r, ri, f, fi))
        ri, fi = bw.sum_redistance([s[4] for s in stages]), bw.sum_filter([s[6] for s in stages])
        final = [bw.sign_band(s[5]) for s in stages]                               # SNAP, identity, T == Gs: X with s_X as its mask
        # the library
        nb1 = mesh.narrow_band_sdf(g33.grid, NB_WIDTHS, SignMethod.Raycast, bits=True)
        nb2 = mesh2.narrow_band_sdf(g33.grid, NB_WIDTHS, SignMethod.Raycast, bits=True)
        assert nb1.cells.is_cuda and nb1.bits.is_cuda
        with nb1.field(background=(bg[1], bg[0]), inside=nb1) as f1, nb2.field(background=(bg[1], bg[0]), inside=nb2) as f2:
            del nb1, nb2
            with f1 | f2 as fu, fu.redistance((inn, ext)) as fr, fr.filter(FilterKind.MeanCurvature, 2, where=f2) as ff, \
                    ff.resample(g33.grid, None, mode=SampleMode.Snap) as fs:
                g = fr.redistance_info
                assert (g.sweeps, int(g.converged), g.n_frozen, g.n_open, g.n_candidates) == tuple(ri), (g, ri)
                g = ff.filter_info
                assert (g.passes, g.n_changed, g.n_sign_flips, g.n_nonfinite) == (fi.passes, fi.n_changed, fi.n_sign_flips, fi.n_nonfinite), (g, fi)
                assert F(g.max_change).view(np.uint32) == F(fi.max_change).view(np.uint32)
                assert tuple(fs.resample_info) == (sum(b.cells.size for b in final), 0, 0, sum(bw.open_faces(b) for b in final))
                want_mask = torch.zeros_like(g33.mask_a)
                _patch(want_mask, wins, final)
                _check(fs, lt, final, want_mask, "the chain's result", windows=wins)
                del want_mask
                # the exported lists as an isosurface, and the handle sampled
                out = fs.to_band()
                assert out.cells.is_cuda
                got = band_isosurface(g33.grid, out.cells, out.distances)
                gi = im.GridI.of(g33.grid)
                parts = [bim.extract_box(gi, tuple(zip(w.lo, w.hi)), w.to_big(b.cells), b.distances, 0.0) for w, b in zip(wins, final)]
                assert all(len(p[1]) > 50 for p in parts)
                want = (np.concatenate([p[0] for p in parts]), np.concatenate([parts[0][1], parts[1][1] + np.uint32(len(parts[0][0]))]),
                        parts[0][2] + parts[1][2])
                _same_mesh(got, want, "the chain's isosurface")
                cells, dist = bw.embed(wins, final)
                model = bqm.Band(lt.big, cells, dist, final[0].bg_out, final[0].bg_in)
                model.bits = bw.SparseBits(wins, final)
                q = gqm.GridQ.of(g33.grid)
                rng = np.random.default_rng(8)
                pts = np.concatenate([(q.start + (np.array(c, F) + rng.uniform(-9, 9, (300, 3)).astype(F) * F(bw.G33_CELL[0]) / q.cs) * q.cs).astype(F)
                                      for c in NB_CENTRES]).astype(F)
                for mode in MODES:
                    wv, ws = bqm.sample(q, model, pts, int(mode))
                    gv, gs = fs.sample(torch.as_tensor(pts, device=DEV), mode=mode, support=True)
                    assert gqm.same_bits(_np(gv), wv) and np.array_equal(_np(gs), ws), f"the chain's result sampled, {mode.name}"
                    assert (ws[:300] == bqm.K_OF[mode]).any() and (ws[300:] == bqm.K_OF[mode]).any() and (ws == 0).any()


# ---- G34 -----------------------------------------------------------------------------------------------------------------------------------
def test_g34_second_trip_of_the_grid_stride_loops():
    """4096 x 4096 x 1100: launches over mask words or sign words are capped at 2^20 workgroups of 256 lanes, so at more than 2^28 words
    the loops of the sign-mask conversions (create, export), of the export's cells and of redistance's candidate selection take a second
    trip; the box in the high corner (L > 2^34) is handled by it.  create with a mask -> export; union of two bands made without masks;
    redistance of the union."""
    _need_free(48, "G34")
    lt = bw.layout_g34()
    words = (lt.total + 63) // 64
    assert lt.total > 2 ** 34 and words > 2 ** 28 and lt.big[0] * lt.big[1] * ((lt.big[2] + 31) // 32) > 2 ** 28
    assert int(lt.windows[0].to_big(lt.b[0].cells)[0]) == 0 and int(lt.windows[1].to_big(lt.a[1].cells)[0]) > 2 ** 34
    assert int(lt.windows[1].to_big(lt.a[1].cells)[-1]) == lt.total - 1
    grid = _grid(lt)
    mask = _mask(lt, lt.a, ((slice(500, 504), -1), ((slice(4000, 4090), slice(10, 12)), 0x5A5A5A5A)))    # the second slab lies in the second trip
    want = mask.clone()
    _clear_tail(want, lt.big[2])
    with _field(lt, grid, lt.a, mask) as f:
        _check(f, lt, lt.a, want, "G34 create with a mask", created=True)
    del mask, want
    torch.cuda.empty_cache()
    wa, wb = _unmasked(lt.a), _unmasked(lt.b)
    union = [cm.csg(x, y, cm.UNION) for x, y in zip(wa, wb)]
    ext, inn = lt.widths[0]
    for win, band in zip(lt.windows, union):
        bw.check_redistance(win, band, lt.cell, ext, inn)
    parts = [rm.redistance(b, lt.cell, ext, inn) for b in union]
    assert all(p[1].n_frozen > 0 for p in parts)
    info = bw.sum_redistance([p[1] for p in parts])
    with _field(lt, grid, wa, None) as fa, _field(lt, grid, wb, None) as fb, fa.csg(fb, CsgOp.Union) as fu:
        want = torch.zeros((lt.big[0], lt.big[1], (lt.big[2] + 31) // 32), dtype=torch.int32, device=DEV)
        _patch(want, lt.windows, union)
        _check(fu, lt, union, want, "G34 union")
        with fu.redistance((inn, ext)) as r:
            ri = r.redistance_info
            assert (ri.sweeps, int(ri.converged), ri.n_frozen, ri.n_open, ri.n_candidates) == tuple(info), f"info {ri}, the windows give {info}"
            _check(r, lt, [p[0] for p in parts], want, "G34 redistance")       # s is the union's on every point
