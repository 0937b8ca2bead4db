"""tests/band_window.py proved on the CPU: on grids small enough for the dense numpy models, the model on the whole grid equals, bit for
bit, the models on the windows embedded (or, for components, merged), for csg, redistance, filter, advect, components and select; a layout that breaks a margin rule by one layer makes the
helper raise; and the layouts of tests/test_gpu_band_large.py meet, with the models alone, the conditions that keep those tests from
passing vacuously.  This is what makes the expected values of the large GPU tests trustworthy."""
import numpy as np
import pytest

import band_advect_model as am
import band_components_model as ccm
import band_csg_model as cm
import band_filter_model as fm
import band_redistance_model as rm
import band_resample_model as rsm
import band_window as bw

F = np.float32
CELL = (0.125, 0.125, 0.0625)
WIDTHS = ((0.125, 0.0625), (0.1875, 0.0))        # K = (2, 2, 3) outside and (2, 2, 2) inside; K = (3, 3, 4) and (1, 1, 1)
# nz above and below 64 (the shared walk steps differently); one box in the interior, one that ends with the grid in the high corner
GRIDS = {(23, 19, 70): ((5, 5, 6), (18, 14, 64)), (40, 37, 21): ((5, 5, 6), (35, 32, 15))}
OPS = (cm.UNION, cm.INTERSECTION, cm.DIFFERENCE)


def _layout(big):
    return bw.layout(big, (-1.0, 0.5, 0.25), CELL, GRIDS[big], WIDTHS, sum(big), box_shape=(5, 5, 6))


def _random_bits(rng, shape, windows):
    """A random mask with the bits at k >= nz zero and the windows' bits zero."""
    s = rng.random(shape) < 0.5
    for w in windows:
        s[w.lo[0]:w.hi[0], w.lo[1]:w.hi[1], w.lo[2]:w.hi[2]] = False
    return cm.pack_bits(shape, s)


@pytest.fixture(scope="module", params=list(GRIDS), ids=lambda n: "x".join(map(str, n)))
def lay(request):
    lt = _layout(request.param)
    w = lt.windows
    assert not any(w[0].at_face(a, s) for a in range(3) for s in (0, 1)), "the first window is not interior"
    assert all(w[1].at_face(a, 1) for a in range(3)) and int(w[1].to_big(lt.a[1].cells)[-1]) == lt.total - 1
    return lt


# ---- the index maps ------------------------------------------------------------------------------------------------------------------------
def test_index_maps_and_mask_words():
    big = (2048, 2048, 1100)
    w = bw.Window(big, (1902, 1023, 791), (8, 9, 43))
    L = np.arange(8 * 9 * 43)
    i, j, k = w.ijk(L)
    assert (i.min(), i.max(), j.min(), j.max(), k.min(), k.max()) == (1902, 1909, 1023, 1031, 791, 833)
    B = w.to_big(L)
    assert B.dtype == np.int64 and [int(v) for v in B[[0, -1]]] == [791 + 1023 * 1100 + 1902 * 2048 * 1100, 833 + 1031 * 1100 + 1909 * 2048 * 1100]
    assert int(B[-1]) > 2 ** 32 > int(B[0]) and np.array_equal(w.from_big(B), L) and w.contains(B).all()
    assert not w.contains([int(B[0]) - 1, int(B[-1]) + 1, 0, 2 ** 32 + 43]).any() and w.contains([2 ** 32]).all()   # (1906, 1027, 796)
    with pytest.raises(bw.LayoutError):
        w.from_big([0])
    with pytest.raises(bw.LayoutError):
        bw.Window(big, (2041, 0, 0), (8, 1, 1))
    # the words of a small grid's mask, against the dense unpacking
    rng = np.random.default_rng(1)
    shape = (6, 5, 70)
    s = rng.random(shape) < 0.5
    bits = cm.pack_bits(shape, s)
    for lo, n in (((1, 2, 3), (4, 2, 30)), ((0, 0, 31), (6, 5, 39)), ((2, 1, 64), (1, 1, 1)), ((0, 0, 0), shape)):
        v = bw.Window(shape, lo, n)
        sl = v.word_slices()
        part = s[lo[0]:lo[0] + n[0], lo[1]:lo[1] + n[1], lo[2]:lo[2] + n[2]]
        assert np.array_equal(v.get_bits(bits[sl]), part)
        new = rng.random(n) < 0.5
        want = s.copy()
        want[lo[0]:lo[0] + n[0], lo[1]:lo[1] + n[1], lo[2]:lo[2] + n[2]] = new
        patched = bits.copy()
        patched[sl] = v.put_bits(bits[sl], new)
        assert np.array_equal(patched, cm.pack_bits(shape, want))
    with pytest.raises(bw.LayoutError):
        bw.check_disjoint([bw.Window(shape, (0, 0, 0), (3, 3, 3)), bw.Window(shape, (2, 2, 2), (2, 2, 2))])
    with pytest.raises(bw.LayoutError):
        bw.split([bw.Window(shape, (0, 0, 0), (3, 3, 3))], [5 * 70 * 5])


# ---- each call: the dense model on the whole grid equals the windows embedded ---------------------------------------------------------------
def test_csg(lay):
    """Defined per grid point: the mask beyond the windows is random and differs between the operands."""
    rng = np.random.default_rng(2)
    w = lay.windows
    out_a, out_b = _random_bits(rng, lay.big, w), _random_bits(rng, lay.big, w)
    sa, sb = cm.unpack_bits(lay.big, out_a), cm.unpack_bits(lay.big, out_b)
    for masked in (True, False):
        strip = (lambda bands: bands) if masked else (lambda bands: [cm.Band(b.shape, b.cells, b.distances, None, b.bg_out, b.bg_in) for b in bands])
        wa, wb = strip(lay.a), strip(lay.b)
        A = bw.embed_band(w, wa, out_a, masked)
        B = bw.embed_band(w, wb, out_b, masked)
        for second, wsecond in ((B, wb), (A, wa)):                                   # a op b, and a op a
            for op in OPS:
                got = cm.csg(A, second, op)
                want = [cm.csg(x, y, op) for x, y in zip(wa, wsecond)]
                s2 = sa if second is A else sb
                beyond = {cm.UNION: sa | s2, cm.INTERSECTION: sa & s2, cm.DIFFERENCE: sa & ~s2}[op] if masked else np.zeros(lay.big, bool)
                if not masked and op == cm.DIFFERENCE:
                    beyond = np.zeros(lay.big, bool)                                 # 0 & ~0
                assert bw.same_as_embedded(got, w, want, cm.pack_bits(lay.big, beyond)), (masked, op)
                assert got.cells.size == sum(b.cells.size for b in want)
                assert got.bg_out == want[0].bg_out and got.bg_in == want[0].bg_in


def test_redistance(lay):
    w = lay.windows
    A = bw.embed_band(w, lay.a)
    for ext, inn in WIDTHS:
        for win, band in zip(w, lay.a):
            bw.check_redistance(win, band, CELL, ext, inn)
        got, info = rm.redistance(A, CELL, ext, inn)
        parts = [rm.redistance(b, CELL, ext, inn) for b in lay.a]
        assert bw.same_as_embedded(got, w, [p[0] for p in parts]), (ext, inn)
        assert info == bw.sum_redistance([p[1] for p in parts]), (info, [p[1] for p in parts])
        assert info.converged and all(p[1].n_frozen > 0 and p[1].sweeps > 1 for p in parts)
        assert all(p[0].cells.size > b.cells.size for p, b in zip(parts, lay.a)) or inn == 0.0      # the band grew into the margin


@pytest.mark.parametrize("kind", fm.KINDS)
def test_filter(lay, kind):
    w = lay.windows
    A = bw.embed_band(w, lay.a)
    for where in (None, lay.where):
        for i, (win, band) in enumerate(zip(w, lay.a)):
            bw.check_filter(win, band, None if where is None else where[i])
        W = None if where is None else bw.embed_band(w, where)
        got, info = fm.band_filter(A, CELL, kind, 2, W)
        parts = [fm.band_filter(b, CELL, kind, 2, None if where is None else where[i]) for i, b in enumerate(lay.a)]
        assert bw.same_as_embedded(got, w, [p[0] for p in parts]), (kind, where is not None)
        want = bw.sum_filter([p[1] for p in parts])
        assert info[0] == want[0] and F(info.max_change).view(np.uint32) == F(want.max_change).view(np.uint32) and info[2:] == want[2:]
        assert all(p[1].n_changed > 0 for p in parts)
        if where is not None:
            assert all(0 < p[1].n_changed < b.cells.size for p, b in zip(parts, lay.a))


@pytest.mark.parametrize("mode", rsm.MODES)
def test_resample(lay, mode):
    """The sparse restatement against the dense model, both ways: the whole grid as the source of a small turned and scaled target over
    each box, and a small source placed into the whole grid by the inverse map, where the result is a window of the target."""
    w = lay.windows
    spec = rsm.GridSpec(lay.first, lay.cell, lay.big)
    X = bw.embed_band(w, lay.full)
    x = bw.sparse_source(lay.big, X.cells, X.distances, bw.SparseBits(w, lay.full), X.bg_out, X.bg_in)
    rng = np.random.default_rng(3)
    for i in range(len(w)):
        fwd, inv, small = bw.placement(lay, i)
        to_source, scale = rsm.similarity(fwd)
        want, info = rsm.resample(X, spec, small, to_source, scale, mode)
        got, ginfo = bw.resample_window(x, spec, small, bw.Window(small.shape, (0, 0, 0), small.shape), to_source, scale, mode)
        assert cm.same(got, want) and ginfo == info and info.n_cells > 20, (i, mode, info)
        assert info.n_partial > 0 or mode == rsm.SNAP
        # the other way: a random band on the small grid, placed into the whole grid
        total = small.shape[0] * small.shape[1] * small.shape[2]
        cells = np.flatnonzero(rng.random(total) < 0.9)
        bits = cm.pack_bits(small.shape, rng.random(small.shape) < 0.5)
        Y = cm.Band(small.shape, cells, (rng.uniform(-1, 1, cells.size) * 0.05).astype(F), bits, 0.75, 0.5)
        to_source, scale = rsm.similarity(inv)
        want, info = rsm.resample(Y, small, spec, to_source, scale, mode)
        win = bw.target_box_of_source(small, spec, inv)
        y = bw.sparse_source(small.shape, Y.cells, Y.distances, Y.bits, Y.bg_out, Y.bg_in)
        got, ginfo = bw.resample_window(y, small, spec, win, to_source, scale, mode)
        assert bw.same_as_embedded(want, [win], [got]) and ginfo == info and info.n_cells > 20, (i, mode, info, ginfo)
        assert want.bg_out.view(np.uint32) == got.bg_out.view(np.uint32) and want.bg_in.view(np.uint32) == got.bg_in.view(np.uint32)


# slabs of the 5 x 5 x 6 boxes: sparse, dense, and in the second box two sparse ones
SLABS = ((((0, 2), 0.3), ((3, 5), 0.85)), (((0, 2), 0.3), ((3, 5), 0.4)))


def _runs(lay):
    return ((1, lay.big[2] - 2), (2, lay.big[2]))


@pytest.mark.parametrize("kind", am.KINDS)
def test_advect(lay, kind):
    w = lay.windows
    rng = np.random.default_rng(4)
    outside = _random_bits(rng, lay.big, w)
    dt = F(0.5 * min(CELL))
    fields = [bw.trig_field(win, b, kind, 10 + i) for i, (win, b) in enumerate(zip(w, lay.a))]
    for masked in (True, False):
        bands = lay.a if masked else [cm.Band(b.shape, b.cells, b.distances, None, b.bg_out, b.bg_in) for b in lay.a]
        for win, b in zip(w, bands):
            bw.check_advect(win, b)
        A = bw.embed_band(w, bands, outside, masked)
        for background in (None, (1.25, 0.375)):
            got, info = am.band_advect(A, CELL, kind, bw.embed_field(w, bands, fields), dt, 3, background)
            parts = [am.band_advect(b, CELL, kind, f, dt, 3, background) for b, f in zip(bands, fields)]
            assert bw.same_as_embedded(got, w, [p[0] for p in parts], outside if masked else None), (kind, masked)
            assert got.bg_out == parts[0][0].bg_out and got.bg_in == parts[0][0].bg_in
            want = bw.sum_advect([p[1] for p in parts])
            assert info[0] == want[0] == 3 and info[3:] == want[3:] and all(F(x).view(np.uint32) == F(y).view(np.uint32) for x, y in zip(info[1:3], want[1:3]))
            assert all(0 < p[1].n_moving < b.cells.size and p[1].n_changed > 0 for p, b in zip(parts, bands))
    # the maxima are the larger window's, taken on the bits: +inf is above every finite value
    x = am.Info(3, F(0.5), F(np.inf), 1, 2, 3, 4)
    assert bw.sum_advect([x, am.Info(3, F(0.75), F(2.0), 10, 20, 30, 40)]) == am.Info(3, F(0.75), F(np.inf), 11, 22, 33, 44)
    with pytest.raises(bw.LayoutError):
        bw.sum_advect([x, am.Info(2, F(0), F(0), 0, 0, 0, 0)])


def _same_components(got, want):
    return (got.count == want.count and all(np.array_equal(g, x) and g.dtype == x.dtype and g.shape == x.shape
                                            for g, x in zip((got.labels,) + tuple(got[2:]), (want.labels,) + tuple(want[2:]))))


@pytest.mark.parametrize("connectivity", ccm.CONNECTIVITIES)
def test_components(lay, connectivity):
    w = lay.windows
    counts = {}
    for name, bands in (("blobs", bw.blob_bands(lay, 1, SLABS)), ("a", lay.a)):
        for win, b in zip(w, bands):
            bw.check_components(win, b)
        parts = [ccm.components(b, connectivity) for b in bands]
        merged, maps = bw.merge_components(w, bands, parts)
        assert _same_components(ccm.components(bw.embed_band(w, bands), connectivity), merged), (name, connectivity)
        assert all(np.array_equal(np.sort(m), m) and m.size == p.count for m, p in zip(maps, parts)) and merged.count == sum(p.count for p in parts)
        counts[name] = [p.count for p in parts]
    assert all(c >= 2 for c in counts["blobs"])


def test_select(lay):
    w = lay.windows
    blobs = bw.blob_bands(lay, 1, SLABS)
    rows = bw.select_windows(lay, (2, 2))
    bands = bw.select_bands(lay, blobs, _runs(lay), (2, 2))
    rng = np.random.default_rng(6)
    outside = _random_bits(rng, lay.big, rows)
    A = bw.embed_band(rows, bands, outside)
    for win, b in zip(rows, bands):
        bw.check_select(win, b)
    for connectivity in ccm.CONNECTIVITIES:
        parts = [ccm.components(b, connectivity) for b in bands]
        merged, maps = bw.merge_components(rows, bands, parts)
        keep = np.arange(merged.count) % 2 == 0
        for background in (None, (1.25, 0.375)):
            got, info = ccm.select(A, merged.labels, keep, background)
            res = [ccm.select(b, p.labels, keep[m], background) for b, p, m in zip(bands, parts, maps)]
            assert bw.same_as_embedded(got, rows, [r[0] for r in res], outside), connectivity
            assert got.bg_out == res[0][0].bg_out and got.bg_in == res[0][0].bg_in
            assert info == bw.sum_select([r[1] for r in res]) and all(r[1].n_dropped > 0 and r[1].n_cells > 0 for r in res)
            assert sum(r[1].n_sign_cleared for r in res) > 0


def test_rehome_moves_a_band_between_windows():
    lt = _layout((23, 19, 70))
    st = lt.sites[0]
    rows = bw.select_windows(lt, (2, 2))[0]
    moved = bw.rehome(lt.a[0], st.window, rows)
    assert np.array_equal(rows.to_big(moved.cells), st.window.to_big(lt.a[0].cells)) and np.array_equal(moved.distances, lt.a[0].distances)
    assert bw.same_as_embedded(bw.embed_band([st.window], [lt.a[0]]), [rows], [moved])     # the box's bits travel, the rest is clear on both
    with pytest.raises(bw.LayoutError):
        bw.rehome(lt.a[0], st.window, bw.Window(lt.big, st.window.lo, (3, 3, 3)))


def test_a_resample_window_that_cuts_the_source_box_raises():
    lt = _layout((40, 37, 21))
    spec = rsm.GridSpec(lt.first, lt.cell, lt.big)
    fwd, inv, small = bw.placement(lt, 0)
    y = bw.sparse_source(small.shape, np.arange(small.shape[0] * small.shape[1] * small.shape[2]), np.full(small.shape, 0.01, F), None, 0.5, 0.5)
    win = bw.target_box_of_source(small, spec, inv)
    thin = bw.Window(spec.shape, [l + 3 for l in win.lo], [n - 3 for n in win.shape])
    with pytest.raises(bw.LayoutError, match="on the source box"):
        bw.resample_window(y, small, spec, thin, *rsm.similarity(inv), rsm.SNAP)
    bw.resample_window(y, small, spec, win, *rsm.similarity(inv), rsm.SNAP)


# ---- a layout that breaks a rule by one layer makes the helper raise -----------------------------------------------------------------------
def _one_cell(win, at, value=0.01, s=None):
    act = np.zeros(win.shape, bool)
    act[at] = True
    s = np.zeros(win.shape, bool) if s is None else s
    return cm.Band(win.shape, np.flatnonzero(act.reshape(-1)), np.array([value], F), cm.pack_bits(win.shape, s), 0.5, 0.5)


def test_a_margin_one_layer_too_thin_raises():
    big = (23, 19, 70)
    win = bw.Window(big, (3, 3, 3), (12, 12, 14))
    ext, inn = WIDTHS[0]                                       # K = (2, 2, 3): three, three and four free layers are needed
    ok = _one_cell(win, (3, 3, 4))
    bw.check_redistance(win, ok, CELL, ext, inn)
    bw.check_filter(win, ok)
    for at in ((2, 3, 4), (3, 2, 4), (3, 3, 3), (9, 3, 4), (3, 9, 4), (3, 3, 10)):       # K layers free on one side
        with pytest.raises(bw.LayoutError, match="layers without active points"):
            bw.check_redistance(win, _one_cell(win, at), CELL, ext, inn)
        bw.check_filter(win, _one_cell(win, at))                                          # the filter needs one layer only
    for at in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (11, 5, 5), (5, 11, 5), (5, 5, 13)):     # no free layer
        with pytest.raises(bw.LayoutError, match="holds an active point"):
            bw.check_filter(win, _one_cell(win, at))
    # the sign bits: a set bit in the outermost layer (filter), a set bit outside the block (redistance)
    s = np.zeros(win.shape, bool)
    s[0, 4, 4] = True
    with pytest.raises(bw.LayoutError, match="sign bits"):
        bw.check_filter(win, _one_cell(win, (5, 5, 5), s=s))
    with pytest.raises(bw.LayoutError, match="sign bits"):
        bw.check_filter(win, ok, where=_one_cell(win, (5, 5, 5), s=s))
    with pytest.raises(bw.LayoutError, match="not uniform"):
        bw.check_redistance(win, _one_cell(win, (5, 5, 5), s=s), CELL, ext, inn)
    # the window's n must exceed K (3 along z here), or min(ceil(W / h) + 1, n) picks the other branch on the window
    thin = bw.Window(big, (3, 3, 0), (12, 12, 3))
    with pytest.raises(bw.LayoutError, match="does not exceed"):
        bw.check_redistance(thin, _one_cell(thin, (5, 5, 0)), CELL, 0.125, 0.0)
    # at a face of the big grid no margin is asked for
    corner = bw.Window(big, (11, 7, 56), (12, 12, 14))
    bw.check_redistance(corner, _one_cell(corner, (11, 11, 13)), CELL, ext, inn)
    bw.check_filter(corner, _one_cell(corner, (11, 11, 13)))
    # advect has the filter's rule, components needs the free layer only, select whole rows
    bw.check_advect(win, ok)
    bw.check_components(win, ok)
    bw.check_advect(corner, _one_cell(corner, (11, 11, 13)))
    bw.check_components(corner, _one_cell(corner, (11, 11, 13)))
    for at in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (11, 5, 5), (5, 11, 5), (5, 5, 13)):
        with pytest.raises(bw.LayoutError, match="advect: .* holds an active point"):
            bw.check_advect(win, _one_cell(win, at))
        with pytest.raises(bw.LayoutError, match="components: .* holds an active point"):
            bw.check_components(win, _one_cell(win, at))
    with pytest.raises(bw.LayoutError, match="advect: .* sign bits"):
        bw.check_advect(win, _one_cell(win, (5, 5, 5), s=s))
    bw.check_components(win, _one_cell(win, (5, 5, 5), s=s))                                 # components reads no sign bit
    with pytest.raises(bw.LayoutError, match="select: the window covers"):
        bw.check_select(win, ok)
    for lo, n in (((3, 3, 1), (4, 4, 69)), ((3, 3, 0), (4, 4, 69))):
        cut = bw.Window(big, lo, n)
        with pytest.raises(bw.LayoutError, match="select: the window covers"):
            bw.check_select(cut, _one_cell(cut, (1, 1, 1)))
    rows = bw.row_window(big, (3, 3), (4, 4))
    bw.check_select(rows, _one_cell(rows, (0, 0, 0)))


def test_a_margin_too_thin_changes_the_result():
    """Why the rules are there: with no free layer the filter's clamped read differs from the big grid's, and the embedded window no
    longer equals the model on the whole grid; with fewer than K free layers the window cuts the candidate box of redistance."""
    big = (23, 19, 70)
    rng = np.random.default_rng(7)
    st = bw.site(big, (8, 7, 30), (4, 4, 4), (0, 0, 0))                                   # the window is the box: no free layer
    band = bw.random_band(rng, st, (0, 0, 0), (4, 4, 4), 0.05, density=1.0)
    A = bw.embed_band([st.window], [band])
    with pytest.raises(bw.LayoutError):
        bw.check_filter(st.window, band)
    got = fm.band_filter(A, CELL, fm.LAPLACIAN, 1)[0]
    assert not bw.same_as_embedded(got, [st.window], [fm.band_filter(band, CELL, fm.LAPLACIAN, 1)[0]])
    st = bw.site(big, (8, 7, 30), (4, 4, 4), (1, 1, 1))
    band = bw.random_band(rng, st, (0, 0, 0), (4, 4, 4), 0.05, density=1.0)
    with pytest.raises(bw.LayoutError):
        bw.check_redistance(st.window, band, CELL, *WIDTHS[0])
    whole, cut = rm.redistance(bw.embed_band([st.window], [band]), CELL, *WIDTHS[0]), rm.redistance(band, CELL, *WIDTHS[0])
    assert whole[1].n_candidates > cut[1].n_candidates                                    # the info no longer adds up


def test_windows_that_break_the_new_rules_change_the_result():
    """Two windows whose bands touch across their sides are one component on the whole grid and two when merged; a select window that
    cuts a row does not see the kept cell beyond the cut and clears what the whole row keeps."""
    big = (23, 19, 70)
    w = [bw.Window(big, (4, 4, 4), (3, 3, 3)), bw.Window(big, (7, 4, 4), (3, 3, 3))]
    bands = [_one_cell(w[0], (2, 1, 1)), _one_cell(w[1], (0, 1, 1))]
    with pytest.raises(bw.LayoutError):
        bw.check_components(w[0], bands[0])
    merged, _ = bw.merge_components(w, bands, [ccm.components(b, 6) for b in bands])
    assert merged.count == 2 and ccm.components(bw.embed_band(w, bands), 6).count == 1
    # a row with a dropped cell at k = 10, inside bits above it, and a kept cell at k = 40: nothing is cleared; cut at k = 30, all is
    s = np.zeros(big, bool)
    s[5, 5, 11:40] = True
    whole = cm.Band(big, [10 + 5 * 70 + 5 * 19 * 70, 40 + 5 * 70 + 5 * 19 * 70], [0.01, 0.01], cm.pack_bits(big, s), 0.5, 0.5)
    assert ccm.select(whole, [0, 1], [False, True])[1] == ccm.SelectInfo(1, 1, 0)
    cut = bw.Window(big, (5, 5, 0), (1, 1, 30))
    part = cm.Band(cut.shape, [10], [0.01], cm.pack_bits(cut.shape, s[5:6, 5:6, :30]), 0.5, 0.5)
    with pytest.raises(bw.LayoutError):
        bw.check_select(cut, part)
    assert ccm.select(part, [0], [False])[1] == ccm.SelectInfo(0, 1, 19)


# ---- the layouts of the large GPU tests, with the models alone -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g33", "g34"])
def test_the_large_layouts_meet_their_conditions(name):
    lt = bw.layout_g33() if name == "g33" else bw.layout_g34()
    w = lt.windows
    big_a = [win.to_big(b.cells) for win, b in zip(w, lt.a)]
    assert int(big_a[1][-1]) == lt.total - 1
    if name == "g33":
        assert lt.total > 2 ** 32 and (lt.total + 63) // 64 == 72089600
        assert 796 + 1027 * 1100 + 1906 * 2048 * 1100 == 2 ** 32
        assert (big_a[0] < 2 ** 32).sum() > 50 and (big_a[0] >= 2 ** 32).sum() > 50 and int(big_a[1][0]) > 2 ** 32
    else:
        assert lt.total > 2 ** 34 and (lt.total + 63) // 64 > 2 ** 28 and 4096 * 4096 * 35 > 2 ** 28
        assert int(big_a[0][-1]) < 2 ** 28 and int(big_a[1][0]) > 2 ** 34
        assert int(w[0].to_big(lt.b[0].cells)[0]) == 0
    for i, win in enumerate(w):
        for op in OPS:
            assert cm.csg(lt.a[i], lt.b[i], op).cells.size > 50
        for ext, inn in lt.widths:
            bw.check_redistance(win, lt.a[i], lt.cell, ext, inn)
            bw.check_redistance(win, cm.csg(lt.a[i], lt.b[i], cm.UNION), lt.cell, ext, inn)
            r, info = rm.redistance(lt.a[i], lt.cell, ext, inn)
            assert info.n_frozen > 0 and info.converged and r.cells.size > 50
        bw.check_filter(win, lt.a[i], lt.where[i])
        region = cm.dense(lt.a[i])[0] & cm.dense(lt.where[i])[2]
        assert 0 < region.sum() < lt.a[i].cells.size
        for kind in fm.KINDS:
            for where in (None, lt.where[i]):
                r, info = fm.band_filter(lt.a[i], lt.cell, kind, 2, where)
                assert info.n_changed > 0 and r.cells.size > 50
    if name == "g34":
        return
    # resample: both ways at each site, in every mode
    spec = rsm.GridSpec(lt.first, lt.cell, lt.big)
    cells, dist = bw.embed(w, lt.full)
    x = bw.sparse_source(lt.big, cells, dist, bw.SparseBits(w, lt.full), lt.full[0].bg_out, lt.full[0].bg_in)
    for i in range(len(w)):
        fwd, inv, small = bw.placement(lt, i)
        Y = bw.small_band(lt, i)
        y = bw.sparse_source(small.shape, Y.cells, Y.distances, Y.bits, Y.bg_out, Y.bg_in)
        win = bw.target_box_of_source(small, spec, inv)
        for mode in rsm.MODES:
            r, info = bw.resample_window(x, spec, small, bw.Window(small.shape, (0, 0, 0), small.shape), *rsm.similarity(fwd), mode)
            assert info.n_cells > 50, (i, mode, info)
            r, info = bw.resample_window(y, small, spec, win, *rsm.similarity(inv), mode)
            big = win.to_big(r.cells)
            assert info.n_cells > 50 and (i != 0 or ((big < 2 ** 32).sum() > 50 and (big >= 2 ** 32).sum() > 50)), (i, mode, info)


def test_the_g33_layouts_of_components_select_and_advect_meet_their_conditions():
    """What tests/test_gpu_band_large.py asserts of its components, select, advect and chain cases, with the models alone."""
    lt = bw.layout_g33()
    w = lt.windows
    blobs = bw.blob_bands(lt)
    cells = bw.embed(w, blobs)[0]
    counts = []
    for connectivity in ccm.CONNECTIVITIES:
        for win, b in zip(w, blobs):
            bw.check_components(win, b)
        parts = [ccm.components(b, connectivity) for b in blobs]
        merged, maps = bw.merge_components(w, blobs, parts)
        assert all(p.count >= 3 for p in parts) and (merged.first_cell >= 2 ** 32).sum() >= 3 and (merged.first_cell < 2 ** 32).sum() >= 3
        largest = int(np.argmax(merged.n_cells))
        L = cells[merged.labels == largest]
        assert (L < 2 ** 32).sum() > 50 and (L >= 2 ** 32).sum() > 50, "the largest component does not straddle L = 2^32"
        counts.append(merged.count)
    assert counts[0] > counts[1] > counts[2]
    # select: whole rows, long runs, an alternating keep mask
    rows = bw.select_windows(lt)
    bands = bw.select_bands(lt, blobs, bw.G33_RUNS)
    assert all(r.shape[0] * r.shape[1] * r.shape[2] <= 250000 for r in rows)
    for win, b in zip(rows, bands):
        bw.check_select(win, b)
    parts = [ccm.components(b, 18) for b in bands]
    merged, maps = bw.merge_components(rows, bands, parts)
    keep = np.arange(merged.count) % 2 == 0
    for b, p, m in zip(bands, parts, maps):
        info = ccm.select(b, p.labels, keep[m])[1]
        assert info.n_cells > 50 and info.n_dropped > 10 and info.n_sign_cleared > 64, info
    # advect: the bands of the filter cases and the blobs, fields with cells at rest
    dt = F(0.5 * min(lt.cell))
    for bands in (lt.a, blobs):
        for kind in am.KINDS:
            for i, (win, b) in enumerate(zip(w, bands)):
                bw.check_advect(win, b)
                bw.check_advect(win, cm.Band(b.shape, b.cells, b.distances, None, b.bg_out, b.bg_in))
                r, info = am.band_advect(b, lt.cell, kind, bw.trig_field(win, b, kind, 20 + i), dt, 3)
                assert 0 < info.n_moving < b.cells.size and info.n_changed > 50 and info.n_sign_flips > 0 and r.cells.size > 50, (kind, i, info)
