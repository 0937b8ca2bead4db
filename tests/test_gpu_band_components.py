"""m2s_band_components and m2s_band_select on the GPU, bit for bit against tests/band_components_model.py (the definition in numpy):
random bands at three densities, empty and full bands, a one-cell-wide serpentine and cubes that touch along an edge or at a corner, on
the shapes where the walk over the mask words can go wrong, for each connectivity, with and without a sign mask, from device tensors and
host arrays; the keep sets of the header; select inside solids (rows of 64 points or more, few cells, a sign mask that is mostly set:
the words with no active cell, which one lane searches, many of them holding the start of a row, with searches over several words);
the chain that motivates the calls (a union with debris -> keep_largest -> isosurface / sample; split; boolean and remesh with
keep_largest=1); what the calls reject of a real handle; and the C and C++ consumers.  Every comparison with
the model is exact equality."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import band_components_model as ccm
import band_csg_model as cm
import band_redistance_model as rm
from mesh_to_sdf_amd import BandField, Components, Connectivity, Grid, M2SError, Mesh, SampleMode, SelectInfo, Topology, _lib, boolean, isosurface_band, meshes, remesh

F = np.float32
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMAX = np.finfo(F).max
FIRST = (-0.5, 0.25, 0.0)
CELL = (0.125, 0.25, 0.1875)
SPECIAL = np.array([0.0, -0.0, 0.5, -0.5, 0.75, -0.75, 2.0, -2.0, FMAX, -FMAX], F)   # zeros of both signs, values beyond the backgrounds, +-f32::MAX
# a single word, and a second word holding one point; one partial word; rows that straddle words; several rows per word; more than one
# wave unit of 256 words; more than one workgroup with a total that is no multiple of 64
SHAPES = [(1, 1, 1), (1, 1, 64), (1, 1, 65), (3, 4, 5), (2, 3, 70), (5, 7, 67), (6, 9, 31), (2, 300, 129), (40, 41, 43)]
CONNS = (6, 18, 26)


def _np(x):
    if hasattr(x, "cpu"):
        if x.dtype == getattr(torch, "uint32", None):
            x = x.view(torch.int32)
        x = x.cpu().numpy()
    return np.asarray(x)


def _grid(shape):
    return Grid(list(FIRST), list(CELL), list(shape))


def _values(rng, n, special=0.3):
    d = rng.uniform(-1, 1, n).astype(F)
    pick = rng.random(n) < special
    d[pick] = rng.choice(SPECIAL, int(pick.sum()))
    return d


def _bits(rng, shape):
    return rng.integers(0, 2 ** 32, (shape[0], shape[1], (shape[2] + 31) // 32), dtype=np.uint64).astype(np.uint32)


def _band_of(rng, shape, active, bits):
    cells = np.flatnonzero(np.asarray(active, bool).reshape(-1))
    return cm.Band(shape, cells, _values(rng, cells.size), _bits(rng, shape) if bits else None, 0.75, 0.5)


def _serpentine(shape):
    """One cell wide: in every other i-layer the even j-rows whole and the odd ones at alternating ends; the layers between hold one cell."""
    nx, ny, nz = shape
    a = np.zeros(shape, bool)
    for i in range(0, nx, 2):
        a[i, 0::2, :] = True
        for j in range(1, ny, 2):
            a[i, j, nz - 1 if (j // 2) % 2 == 0 else 0] = True
    a[1::2, 0, 0] = True
    return a


def _field(grid, band, device):
    """The BandField of a model Band, from device tensors or host arrays."""
    bg = (float(band.bg_in), float(band.bg_out))
    if device:
        bits = None if band.bits is None else torch.as_tensor(np.ascontiguousarray(band.bits).view(np.int32), device=DEV)
        return BandField(grid, torch.as_tensor(band.cells, device=DEV), torch.as_tensor(band.distances, device=DEV), background=bg, inside=bits)
    return BandField(grid, band.cells.astype(np.uint64), band.distances, background=bg, inside=band.bits)


def _band(field):
    """A handle's lists as a model Band (a result always has a sign mask)."""
    nb = field.to_band()
    return cm.Band(tuple(int(v) for v in field.grid.get_cell_count()), _np(nb.cells).astype(np.int64), _np(nb.distances),
                   _np(nb.bits).view(np.uint32), field.background[1], field.background[0])


def _raw_components(field, conn, labels=True, capacity=None, host=None):
    """m2s_band_components itself -> (rc, count, labels uint32[n] or None, stats structured array or None)."""
    host = field._dev is None if host is None else host
    n = field.count
    o = _lib.M2SOpts()
    o.struct_size, o.device, o.synchronous = C.sizeof(o), -1, 1
    o.mem_kind = _lib.MEM_HOST if host else _lib.MEM_DEVICE
    co = _lib.M2SBandComponentsOpts(8, int(conn))
    count = C.c_uint64(0xdead)
    lab = stats = None
    p_l = p_s = None
    if labels:
        lab = np.full(max(n, 1), 0xabababab, np.uint32) if host else torch.full((max(n, 1),), 0x2b2b2b2b, dtype=torch.int32, device=DEV)
        p_l = lab.ctypes.data if host else lab.data_ptr()
    if capacity is not None:
        stats = np.full((max(capacity, 1), 6), 0xee, np.uint64) if host else torch.full((max(capacity, 1), 6), 0xee, dtype=torch.int64, device=DEV)
        p_s = stats.ctypes.data if host else stats.data_ptr()
    rc = _lib.lib().m2s_band_components(field._h, C.byref(co), C.byref(o), p_l, p_s, capacity or 0, C.byref(count))
    return rc, int(count.value), None if lab is None else _np(lab).view(np.uint32)[:n], None if stats is None else _np(stats).view(np.uint64)


def _check_components(got, want, what):
    assert isinstance(got, Components) and got.count == want.count, f"{what}: {got.count} components, the model has {want.count}"
    labels = _np(got.labels).view(np.uint32)
    differ = labels != want.labels
    assert not differ.any(), f"{what}: {int(differ.sum())} labels differ, first at list place {np.flatnonzero(differ)[0]}"
    for name, g, w in (("first_cell", got.first_cell, want.first_cell), ("n_cells", got.n_cells, want.n_cells),
                       ("n_negative", got.n_negative, want.n_negative), ("box_lo", got.box_lo, want.lo), ("box_hi", got.box_hi, want.hi)):
        assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {name} differs"


def _check_select(field, want, info, what):
    """A selected handle against the model's (Band, SelectInfo): the export's three arrays, the backgrounds, every info field, m2s_band_info."""
    got = _band(field)
    assert got.cells.size == want.cells.size == field.count, f"{what}: {got.cells.size} cells, the model has {want.cells.size}"
    assert np.array_equal(got.cells, want.cells), f"{what}: cells differ"
    differ = got.distances.view(np.uint32) != want.distances.view(np.uint32)
    assert not differ.any(), f"{what}: {int(differ.sum())} distances differ"
    wrong = cm.unpack_bits(want.shape, got.bits) != cm.unpack_bits(want.shape, want.bits)
    assert np.array_equal(got.bits, want.bits), f"{what}: the sign mask differs on {int(wrong.sum())} points, first at {np.argwhere(wrong)[:1]}"
    assert cm.same(got, want), f"{what}: backgrounds differ: {got.bg_out, got.bg_in}, the model has {want.bg_out, want.bg_in}"
    si = field.select_info
    assert isinstance(si, SelectInfo) and tuple(si) == tuple(info), f"{what}: info {si}, the model has {info}"
    n, nbytes = C.c_uint64(0), C.c_uint64(0)
    assert _lib.lib().m2s_band_info(field._h, None, C.byref(n), C.byref(nbytes)) == _lib.M2S_OK
    words = (want.total + 63) // 64
    assert n.value == want.cells.size and nbytes.value == 24 * words + 4 * n.value == field.device_bytes, what


# ---- 1. the model's side, once per shape -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plan(shape):
    """-> [(name, Band, device?, {connectivity: model Components}, [(keep name, labels, keep, background, model Band, model SelectInfo)])]."""
    rng = np.random.default_rng(1000 * shape[0] + 10 * shape[1] + shape[2])
    total = shape[0] * shape[1] * shape[2]
    big = total > 20000
    masks = [("d0.15", rng.random(shape) < 0.15), ("d0.31", rng.random(shape) < 0.31), ("d0.70", rng.random(shape) < 0.7),
             ("empty", np.zeros(shape, bool)), ("full", np.ones(shape, bool)), ("serpentine", _serpentine(shape))]
    plan = []
    for at, (name, active) in enumerate(masks):
        band = _band_of(rng, shape, active, bits=at % 2 == 0)
        comps = {c: ccm.components(band, c) for c in CONNS}
        conn = CONNS[at % 3]
        cc = comps[conn]
        n, count = band.cells.size, cc.count
        half = rng.random(count) < 0.5
        largest = np.zeros(count, bool)
        if count:
            largest[np.argsort(-cc.n_cells.astype(np.int64), kind="stable")[0]] = True
        holes = cc.labels.copy()
        holes[rng.random(n) < 0.2] = ccm.LABEL_NONE
        keeps = [("none", cc.labels, np.zeros(count, bool), None), ("all", cc.labels, np.ones(count, bool), (2.0, 0.125)),
                 ("half", cc.labels, half, None), ("largest", cc.labels, largest, (0.0, 3.0)),
                 ("short", cc.labels, np.ones(count // 2, bool), None), ("label-none", holes, np.ones(count, bool), None)]
        if big:
            keeps = [keeps[(at + 2) % 6], keeps[(at + 5) % 6]]                     # the model is dense: two keep sets per band there
        sel = [(kn, lab, keep, bg) + ccm.select(band, lab, keep, bg) for kn, lab, keep, bg in keeps]
        plan.append((name, band, at % 3 != 1, conn, comps, sel))
    return plan


@pytest.mark.parametrize("shape", SHAPES, ids=lambda n: "x".join(map(str, n)))
def test_components_of_random_empty_full_and_serpentine_bands(shape):
    total = shape[0] * shape[1] * shape[2]
    plan = _plan(shape)
    if total > 100:
        assert max(c.count for p in plan for c in p[4].values()) > 5 and any(p[4][6].count == 1 and p[1].cells.size > total // 3 for p in plan)
    for name, band, device, _, comps, _ in plan:
        with _field(_grid(shape), band, device) as f:
            for conn in CONNS:
                what = f"{shape} {name} connectivity {conn} {'device' if device else 'host'}"
                want = comps[conn]
                got = f.components(conn)
                _check_components(got, want, what)
                if conn == 6:
                    _check_components(f.components(Connectivity.Faces), want, what + " again")      # the same bits from the same handle
                # the count-only call
                rc, count, _, _ = _raw_components(f, conn, labels=False)
                assert rc == _lib.M2S_OK and count == want.count, what
                # a capacity one below the count
                if want.count >= 1:
                    rc, count, _, stats = _raw_components(f, conn, capacity=want.count - 1)
                    assert rc == _lib.ERR_BAD_ARG and count == want.count and "capacity" in _lib.last_error(), what
                    assert (stats == 0xee).all(), f"{what}: the statistics were touched"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda n: "x".join(map(str, n)))
def test_select_against_the_model(shape):
    plan = _plan(shape)
    if shape[0] * shape[1] * shape[2] > 100:
        assert any(s[-1].n_sign_cleared > 0 for p in plan for s in p[5]) and any(0 < s[-1].n_dropped < p[1].cells.size for p in plan for s in p[5])
    for name, band, device, conn, comps, sel in plan:
        with _field(_grid(shape), band, device) as f:
            for kn, lab, keep, bg, want, info in sel:
                what = f"{shape} {name} connectivity {conn} keep {kn} {'device' if device else 'host'}"
                labels = torch.as_tensor(lab.view(np.int32), device=DEV) if device else lab
                with f.select(labels, keep, None if bg is None else (bg[1], bg[0])) as r:
                    _check_select(r, want, info, what)
            for kn, lab, keep, bg, want, info in sel:                                  # through a Components, with numbers rather than a mask
                if kn == "half":
                    with f.select(f.components(conn), np.flatnonzero(keep)) as r:
                        _check_select(r, want, info, f"{shape} {name}: numbers")


# ---- 1b. select inside solids: words with no active cell, searched once by the lane that loaded them --------------------------------------
# Rows of 64 points or more, few active cells and a sign mask that is mostly set: nearly every word is an interior word, many hold the
# end of one row and the start of the next, and the searches run over several words (rows of 129 and 200 points span 3 and 4 words).
INTERIOR_SHAPES = [(1, 1, 64), (1, 1, 65), (2, 3, 70), (5, 7, 67), (3, 5, 200), (2, 300, 129)]


def _mostly(rng, shape, p=0.95):
    return cm.pack_bits(shape, rng.random(shape) < p)


def _interior_words(band):
    """-> (the words with no active cell and some inactive-inside point, those of them in which a row starts past bit 0)."""
    nz = band.shape[2]
    act, _, _ = cm.dense(band)
    loose = cm.unpack_bits(band.shape, band.bits) & ~act
    words = (band.total + 63) // 64
    pad = np.zeros(words * 64, bool)
    a, lo = pad.copy(), pad.copy()
    a[:band.total], lo[:band.total] = act.reshape(-1), loose.reshape(-1)
    interior = ~a.reshape(words, 64).any(1) & lo.reshape(words, 64).any(1)
    starts = np.arange(0, band.total, nz)
    mid = np.zeros(words, bool)
    mid[(starts[starts % 64 != 0]) // 64] = True
    return int(interior.sum()), int((interior & mid).sum())


@functools.lru_cache(maxsize=None)
def _interior_plan(shape):
    """-> [(name, Band, device?, [(keep name, labels, keep, model Band, model SelectInfo)])], the model's side, once."""
    rng = np.random.default_rng(7000 + 100 * shape[0] + 10 * shape[1] + shape[2])
    total = shape[0] * shape[1] * shape[2]

    def band(active, bits):
        cells = np.flatnonzero(np.asarray(active, bool).reshape(-1))
        return cm.Band(shape, cells, _values(rng, cells.size), bits, 0.75, 0.5)

    few = np.zeros(total, bool)
    few[rng.choice(total, max(2, total // 200), replace=False)] = True               # density 0.005, two cells at least
    bands = [("empty, mask mostly set", band(np.zeros(shape, bool), _mostly(rng, shape)), True),
             ("serpentine, mask mostly set", band(_serpentine(shape), _mostly(rng, shape)), True),
             ("density 0.005, mask mostly set", band(few.reshape(shape), _mostly(rng, shape)), True),
             ("density 0.005, mask all set", band(few.reshape(shape), cm.pack_bits(shape, np.ones(shape, bool))), False),
             ("density 0.02, random mask, host", band(rng.random(shape) < 0.02, _bits(rng, shape)), False),
             ("density 0.15, random mask, host", band(rng.random(shape) < 0.15, _bits(rng, shape)), False)]
    plan = []
    for name, b, device in bands:
        cc = ccm.components(b, 26)
        half = rng.random(cc.count) < 0.5
        keeps = [("none", np.zeros(cc.count, bool)), ("half", half), ("other half", ~half), ("all", np.ones(cc.count, bool))]
        plan.append((name, b, device, [(kn, cc.labels, keep) + ccm.select(b, cc.labels, keep) for kn, keep in keeps]))
    return plan


@pytest.mark.parametrize("shape", INTERIOR_SHAPES, ids=lambda n: "x".join(map(str, n)))
def test_select_inside_solids(shape):
    plan = _interior_plan(shape)
    words = (shape[0] * shape[1] * shape[2] + 63) // 64
    interior, second_row = (sum(v) for v in zip(*(_interior_words(p[1]) for p in plan)))
    assert interior >= words                                           # summed over the bands: as many interior words as the grid has words
    if shape[0] * shape[1] > 1 and shape[2] % 64:
        assert second_row >= 3, "no interior word holds the start of a row"
    if words > 2:
        assert sum(s[-1].n_sign_cleared for p in plan for s in p[3]) > 0 and any(0 < s[-1].n_sign_cleared for s in plan[2][3] + plan[3][3])
    for name, band, device, sel in plan:
        with _field(_grid(shape), band, device) as f:
            for kn, lab, keep, want, info in sel:
                labels = torch.as_tensor(lab.view(np.int32), device=DEV) if device else lab
                with f.select(labels, keep) as r:
                    _check_select(r, want, info, f"{shape} {name}, keep {kn}, {'device' if device else 'host'}")


def test_touching_cubes_are_joined_by_the_connectivity_that_sees_the_contact():
    for shape in ((6, 9, 31), (40, 41, 43)):
        rng = np.random.default_rng(3)
        edge = np.zeros(shape, bool)
        edge[0:2, 1:3, 3:5] = True
        edge[0:2, 3:5, 5:7] = True                                                   # shares an edge along i with the first: j and k step
        corner = np.zeros(shape, bool)
        corner[1:3, 1:3, 1:3] = True
        corner[3:5, 3:5, 3:5] = True
        for active, counts in ((edge, {6: 2, 18: 1, 26: 1}), (corner, {6: 2, 18: 2, 26: 1})):
            band = _band_of(rng, shape, active, bits=False)
            with _field(_grid(shape), band, True) as f:
                for conn in CONNS:
                    want = ccm.components(band, conn)
                    assert want.count == counts[conn]
                    _check_components(f.components(conn), want, f"{shape} cubes {counts} connectivity {conn}")


# ---- 2. the chain that motivates the calls -------------------------------------------------------------------------------------------------
HALF = ccm.CHAIN_HALF
SPHERES = ccm.CHAIN_SPHERES


@functools.lru_cache(maxsize=None)
def _chain():
    return ccm.chain_bands()


def test_the_chain_in_the_models_first():
    """(A | B) | D with all but the two largest components erased is A | B in every bit: confirmed in the numpy models on the CPU."""
    a, b, d, ab, abd = _chain()
    cc = ccm.components(abd, 6)
    assert cc.count == 3 and sorted(cc.n_cells.tolist()) == sorted([a.cells.size, b.cells.size, d.cells.size])
    keep = np.zeros(3, bool)
    keep[np.argsort(-cc.n_cells.astype(np.int64), kind="stable")[:2]] = True
    out, info = ccm.select(abd, cc.labels, keep)
    assert cm.same(out, ab) and info.n_dropped == d.cells.size and info.n_sign_cleared > 0


def test_keep_largest_removes_the_debris_from_a_union():
    a, b, d, ab, abd = _chain()
    grid = Grid(list(rm.FIRST), list(rm.CELLS), list(rm.SHAPE))
    centre = torch.as_tensor(np.array([SPHERES["D"][0]], F), device=DEV)
    with _field(grid, a, True) as fa, _field(grid, b, True) as fb, _field(grid, d, True) as fd, (fa | fb) as fab, (fab | fd) as fall:
        assert cm.same(_band(fall), abd)
        with fall.keep_largest(2) as kept:
            assert cm.same(_band(kept), ab), "keep_largest(2) of (A | B) | D is not A | B"
            assert kept.select_info.n_dropped == d.cells.size and kept.select_info.n_sign_cleared > 0
            v, i, n_open = kept.isosurface()
            v = _np(v)
            lo = np.array(SPHERES["D"][0]) - SPHERES["D"][1] - HALF
            hi = np.array(SPHERES["D"][0]) + SPHERES["D"][1] + HALF
            assert n_open == 0 and v.shape[0] > 1000 and not ((v >= lo) & (v <= hi)).all(1).any()
            assert float(_np(kept.sample(centre, mode=SampleMode.Snap))[0]) == float(F(HALF))                # outside now
            assert float(_np(fall.sample(centre, mode=SampleMode.Snap))[0]) == -float(F(HALF))               # the island's solid interior
        with fall.remove_islands(d.cells.size + 1) as kept:
            assert cm.same(_band(kept), ab)
        parts = fall.split()
        try:
            assert len(parts) == 3 and sum(p.count for p in parts) == fall.count == abd.cells.size
            assert sorted(p.count for p in parts) == sorted([a.cells.size, b.cells.size, d.cells.size])
        finally:
            for p in parts:
                p.close()


def test_boolean_with_keep_largest_drops_the_small_part():
    big_v, big_i = meshes.blob(24, 12)
    small_v = (big_v * 0.2 + np.array([2.2, 0.0, 0.0])).astype(F)
    other_v = (big_v * 0.9 + np.array([0.3, 0.1, 0.0])).astype(F)
    va = np.concatenate([big_v, small_v]).astype(F)
    ia = np.concatenate([big_i, big_i + big_v.shape[0]]).astype(np.uint32)
    lo, hi = meshes.extended_bbox(np.concatenate([va, other_v]), 0.15)
    grid = Grid.from_bounding_box(lo, hi, [56, 40, 40])
    v0, i0 = boolean(va, Topology.TriangleList(ia), other_v, Topology.TriangleList(big_i), "union", grid)
    v0b, i0b = boolean(va, Topology.TriangleList(ia), other_v, Topology.TriangleList(big_i), "union", grid, keep_largest=0)
    assert np.array_equal(_np(v0).view(np.uint32), _np(v0b).view(np.uint32)) and np.array_equal(_np(i0), _np(i0b))
    v1, i1 = boolean(va, Topology.TriangleList(ia), other_v, Topology.TriangleList(big_i), "union", grid, keep_largest=1)
    v0, v1 = _np(v0), _np(v1)
    # the largest component's box, from the same fields the call makes
    w = isosurface_band(grid, 0.0)
    with Mesh(va, Topology.TriangleList(ia)) as ma, Mesh(other_v, Topology.TriangleList(big_i)) as mb, \
            ma.narrow_band_field(grid, w, background=w) as fa, mb.narrow_band_field(grid, w, background=w) as fb, fa.union(fb) as fr:
        cc = fr.components()
        assert cc.count == 2
        c = int(cc.largest(1)[0])
        first, cell = np.asarray(grid.get_first_cell(), np.float64), np.asarray(grid.get_cell_size(), np.float64)
        box_lo, box_hi = first + cc.box_lo[c] * cell - 1e-5, first + cc.box_hi[c] * cell + 1e-5
        v2, i2 = ma.boolean(mb, "union", grid, keep_largest=1)
    assert 0 < v1.shape[0] < v0.shape[0] and ((v1 >= box_lo) & (v1 <= box_hi)).all()
    assert not ((v0 >= box_lo) & (v0 <= box_hi)).all()
    assert np.array_equal(v1.view(np.uint32), _np(v2).view(np.uint32)) and np.array_equal(_np(i1), _np(i2))


def test_remesh_with_keep_largest_drops_the_small_part():
    big_v, big_i = meshes.blob(24, 12)
    small_v = (big_v * 0.2 + np.array([2.2, 0.0, 0.0])).astype(F)
    va = np.concatenate([big_v, small_v]).astype(F)
    ia = np.concatenate([big_i, big_i + big_v.shape[0]]).astype(np.uint32)
    lo, hi = meshes.extended_bbox(va, 0.15)
    grid = Grid.from_bounding_box(lo, hi, [56, 36, 36])
    topo = Topology.TriangleList(ia)
    v0, i0 = remesh(va, topo, grid)
    v0b, i0b = remesh(va, topo, grid, keep_largest=0)
    assert np.array_equal(_np(v0).view(np.uint32), _np(v0b).view(np.uint32)) and np.array_equal(_np(i0), _np(i0b))    # the default changes nothing
    v1, i1 = remesh(va, topo, grid, keep_largest=1)
    v0, v1, i1 = _np(v0), _np(v1), _np(i1)
    with Mesh(va, topo) as m:
        with m.narrow_band_sdf(grid, isosurface_band(grid, 0.0)).field() as f:
            cc = f.components()
            assert cc.count == 2
            c = int(cc.largest(1)[0])
        first, cell = np.asarray(grid.get_first_cell(), np.float64), np.asarray(grid.get_cell_size(), np.float64)
        box_lo, box_hi = first + cc.box_lo[c] * cell - 1e-5, first + cc.box_hi[c] * cell + 1e-5
        v2, i2 = m.remesh(grid, keep_largest=1)
    assert 0 < v1.shape[0] < v0.shape[0] and ((v1 >= box_lo) & (v1 <= box_hi)).all() and not ((v0 >= box_lo) & (v0 <= box_hi)).all()
    assert i1.size and int(i1.max()) < v1.shape[0]
    inside = ((v0 >= box_lo) & (v0 <= box_hi)).all(1)
    assert np.array_equal(v1.view(np.uint32), v0[inside].view(np.uint32))             # the large part's vertices, every bit, in their order
    assert np.array_equal(v1.view(np.uint32), _np(v2).view(np.uint32)) and np.array_equal(i1, _np(i2))


# ---- 3. what the calls reject of a real handle ---------------------------------------------------------------------------------------------
def test_the_calls_reject_bad_options():
    shape = (7, 9, 11)
    rng = np.random.default_rng(15)
    band = _band_of(rng, shape, rng.random(shape) < 0.4, bits=True)
    L = _lib.lib()
    BAD = _lib.ERR_BAD_ARG

    def opts(**kw):
        o = _lib.M2SOpts()
        o.struct_size, o.device, o.mem_kind = C.sizeof(o), -1, _lib.MEM_DEVICE
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)

    with _field(_grid(shape), band, True) as f:
        cc = f.components(6)
        n = C.c_uint64(0)
        assert L.m2s_band_components(f._h, None, opts(), None, None, 0, C.byref(n)) == _lib.M2S_OK and n.value == cc.count   # NULL opts = 6
        assert L.m2s_band_components(f._h, None, opts(), None, None, 0, None) == BAD
        for size, conn in ((4, 6), (12, 6), (8, 0), (8, 7), (8, 27), (8, -6)):
            assert L.m2s_band_components(f._h, C.byref(_lib.M2SBandComponentsOpts(size, conn)), opts(), None, None, 0, C.byref(n)) == BAD, (size, conn)
        assert L.m2s_band_components(f._h, None, opts(device=1), None, None, 0, C.byref(n)) == BAD and "device" in _lib.last_error()
        for field, value in (("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4), ("mem_kind", 5)):
            assert L.m2s_band_components(f._h, None, opts(**{field: value}), None, None, 0, C.byref(n)) == BAD, field
        labels = cc.labels.view(torch.int32) if cc.labels.dtype != torch.int32 else cc.labels
        keep = torch.ones(cc.count, dtype=torch.uint8, device=DEV)

        def select(lab=labels.data_ptr(), kp=keep.data_ptr(), n_keep=cc.count, fo=None, o=None, info=None, out=True):
            h = C.c_void_p(0x1234)
            rc = L.m2s_band_select(f._h, lab, kp, n_keep, fo, o or opts(), C.byref(h) if out else None, info)
            if out:
                assert (rc == _lib.M2S_OK) == (h.value is not None)            # *out = NULL on every failure
                if h.value is not None:
                    L.m2s_band_destroy(h)
            return rc

        assert select() == _lib.M2S_OK and select(kp=None, n_keep=0) == _lib.M2S_OK
        assert select(lab=None) == BAD and select(kp=None) == BAD and select(out=False) == BAD
        for size, out, ins in ((8, 0.5, 0.5), (12, -0.5, 0.5), (12, 0.5, float("inf")), (12, float("nan"), 0.5)):
            assert select(fo=C.byref(_lib.M2SBandFieldOpts(size, out, ins))) == BAD
        assert select(info=C.byref(_lib.M2SBandSelectInfo(8))) == BAD
        assert select(o=opts(device=1)) == BAD
        for field, value in (("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4), ("mem_kind", 5)):
            assert select(o=opts(**{field: value})) == BAD, field
        with pytest.raises(M2SError):
            f.components(8)
        with pytest.raises(M2SError):
            f.select(cc, [cc.count])
        with pytest.raises(M2SError):
            f.select(np.zeros(3, np.uint32), [0])


def test_c_and_cpp_consumers_run_clean(tmp_path):
    for cc, std, src, extra in (("gcc", "-std=c99", "tests/c/band_components_smoke.c", ["-lm"]),
                                ("g++", "-std=c++17", "tests/cpp/band_components_tests.cpp", [])):
        exe = str(tmp_path / os.path.basename(src).split(".")[0])
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                               os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                               "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", *extra, "-o", exe])
        r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
