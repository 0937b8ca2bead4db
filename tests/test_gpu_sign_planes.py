"""The ray-cast sign planes (csrc/sign.hip) path by path, against the CPU oracle bit for bit.

sign.hip takes one of several paths, chosen by compile-time constants (sign.hip.h sign_path): sixteen lanes or one lane per triangle, big
windows walked by the owner's wave or handed to a work list in chunks, windows small enough for the lane(s) or big, the z scan + majority
with segmented shuffles or with a serial carry, the whole grid or a contiguous or an interleaved x-slab.  A wrong marker flips the sign of
a run of cells along a grid line, so every case compares the whole SDF with oracle.generate_grid_sdf(sign=0, EXACT semantics) bit for bit;
the sign bit is the point.  Before any device call a case asks the host probe of sign.hip.h which cell of the path matrix it stands in — lanes
per triangle, list or not, the largest window of the huge triangles (above 64 x lanes on every axis) and of the blob's (at most that) — so
a case that stops reaching its path fails on the CPU side; test_the_cases_cover_every_path lists every cell with the case that owns it.

Meshes: "few" = meshes.blob(20, 11) (400 triangles) and "many" = meshes.blob(100, 101) (20 000 triangles: above 16 384, and no multiple of
256, so the last workgroup has idle lanes), each with three huge triangles, one roughly normal to each axis, reaching far past the grid —
a dense scan standing on a floor.  The grids are thin in z so that the oracle stays affordable.  Oracle times on an 8-core CPU machine
(seconds, each reference computed once per session):
    few, no list 40x36x30: 0.05        few, list 72x68x16: 0.10            many, no list 40x36x8: 0.57      many, list 72x68x8: 1.81
    few, interleaved 128x32x30: 0.14   many, interleaved 128x40x16: 3.15   the z forms (14 triangles, up to 194 560 cells): 0.01 each
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import oracle as orc
from mesh_to_sdf_amd import Grid, Mesh, SignMethod, Topology, _lib, generate_grid_sdf, interleaved_slab, meshes, narrow_band_sdf, voxelize

pytestmark = pytest.mark.gpu
F = np.float32
U32 = np.uint32
PROBE = os.path.join(os.path.dirname(_lib.SO_PATH), "libm2s_probe.so")
WHOLE = (0, 0, 31, 0, 1)            # SlabX of a call on the whole grid: lo, hi, chunk_log, period, all
FILL = F(12345.0)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
# huge triangles roughly normal to z, y and x (the first two are test_huge_and_tiny_triangles_mixed's)
HUGE = np.array([[-50, -50, 0.3], [50, -50, 0.31], [0, 60, 0.29], [-40, 0.2, -45], [45, 0.21, -44], [0.5, 0.19, 70],
                 [0.25, -45, -40], [0.26, 44, -45], [0.24, 0.5, 70]], F)
BLOBS = {"few": (20, 11), "many": (100, 101)}
# name -> (mesh, cell counts, contiguous x-slab).  Faces of at most 4 096 lines: no list; 72 x 68 = 4 896 lines: three chunks of the list, the last
# one partial.  Sixteen lanes per triangle make a window big above 1 024 lines, so the grids of "few" are thick enough for that on every axis.
CASES = {"few, no list": ("few", (40, 36, 30), (13, 31)),
         "few, list": ("few", (72, 68, 16), (21, 59)),
         "many, no list": ("many", (40, 36, 8), (13, 31)),
         "many, list": ("many", (72, 68, 8), (21, 59))}
# the z forms: counts -> words per row 1, 2, 3, 64, 65
Z_COUNTS = [(7, 9, 1), (9, 7, 33), (9, 7, 65), (6, 5, 2048), (5, 6, 2049)]
# ... and the two whose slabs are run (three words: serial carry; 64 words: rows), wide enough in x for the scan's unrolled body and its tail
Z_SLABS = {(21, 7, 65): (4, 18), (19, 5, 2048): (5, 16)}
# interleaved slabs: mesh, ny, nz, shard of two; x is widened until m2s_interleaved_slab cuts the grid into chunks
INTERLEAVED = {"few, interleaved": ("few", 32, 30, 1), "many, interleaved": ("many", 40, 16, 0)}


def mesh_of(kind):
    v, idx = meshes.blob(*BLOBS[kind])
    vv = np.ascontiguousarray(np.concatenate([v, HUGE]), F)
    ii = np.ascontiguousarray(np.concatenate([idx, len(v) + np.arange(len(HUGE), dtype=np.uint32)]), np.uint32)
    return vv, ii, idx.size // 3


def prism_and_sheet():
    """A closed, slightly tilted prism that runs the length of z (hits of the X- and Y-lines in every word of a row, caps for the Z-lines
    at both ends) and a skew open sheet across it (Z-line hits in a different word from row to row; an open surface: odd counts).  The sheet
    falls along x and rises along y: a cell under it is also in front of it along x and past it along y, so the X- and the Y-lines' parities
    differ there and the Z-lines' parity, which the sheet's marker high up in the row sets through the carry, decides the majority."""
    z0, z1 = -0.985, 0.975
    bottom = np.array([[-0.52, -0.47], [0.45, -0.55], [0.58, 0.41], [-0.43, 0.53]]) + [-0.09, -0.05]
    top = bottom * 0.93 + [0.19, 0.12]
    v = [[x, y, z0] for x, y in bottom] + [[x, y, z1] for x, y in top]
    quads = [(0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7), (3, 2, 1, 0), (4, 5, 6, 7)]
    idx = [t for a, b, c, d in quads for t in (a, b, c, a, c, d)]
    n = len(v)
    v += [[-0.83, -0.79, 0.05], [0.81, -0.84, -0.97], [0.86, 0.77, 0.33], [-0.78, 0.82, 1.24]]       # one corner above the grid: those hits land in the last cell
    idx += [n, n + 1, n + 2, n, n + 2, n + 3]
    return np.array(v, F), np.array(idx, np.uint32)


def grid_of(count, half=2.0):
    return Grid.from_bounding_box([-half] * 3, [half] * 3, [int(c) for c in count])


def raw(grid):
    return np.array(grid.get_first_cell(), F), np.array(grid.get_cell_size(), F), np.array([int(c) for c in grid.get_cell_count()], U32)


def interleaved_grid(ny, nz, k):
    for nx in (64, 128, 256):
        grid = grid_of((nx, ny, nz))
        x0, x1, period = interleaved_slab(grid, 2, k)
        if period:
            return grid, (x0, x1), period
    raise AssertionError("no grid of up to 256 layers can be cut into interleaved chunks")


# ---- the probe: which path a case takes -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        pytest.fail(f"{PROBE} missing: run __graft_entry__.build()")
    L = C.CDLL(PROBE)
    L.probe_sign_path.restype = None
    L.probe_sign_path.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.probe_sign_max_window.restype = None
    L.probe_sign_max_window.argtypes = [C.c_size_t] + [C.c_void_p] * 6
    return L


def path_of(probe, n_tris, count):
    out, consts, cnt = np.zeros(3, U32), np.zeros(4, np.uint64), np.array(count, U32)
    probe.probe_sign_path(n_tris, cnt.ctypes.data, out.ctypes.data, consts.ctypes.data)
    assert tuple(consts) == (64, 16384, 4096, 2048)
    return int(out[0]), bool(out[1]), "rows" if out[2] else "serial"


def max_windows(probe, v, tri_idx, grid, slab=WHOLE):
    tris = np.ascontiguousarray(v[tri_idx.reshape(-1)], F).reshape(-1, 9)
    first, size, n = raw(grid)
    slab, out = np.array(slab, U32), np.zeros(3, U32)
    probe.probe_sign_max_window(len(tris), tris.ctypes.data, first.ctypes.data, size.ctypes.data, n.ctypes.data, slab.ctypes.data, out.ctypes.data)
    return [int(x) for x in out]


def cells_of(probe, v, idx, n_blob, grid, lanes, listed, slab=WHOLE):
    """The cells of the path matrix a call on (mesh, grid) stands in, each claim checked through the probe.  On the whole grid the huge
    triangles' windows are big on every axis; a slab clips the Y- and Z-lines' windows to its layers, so there one big window is asked for."""
    n_tris = idx.size // 3
    count = tuple(int(c) for c in grid.get_cell_count())
    got_lanes, got_list, form = path_of(probe, n_tris, count)
    assert (got_lanes, got_list) == (lanes, listed), (n_tris, count, got_lanes, got_list)
    big = max_windows(probe, v, idx[3 * n_blob:], grid, slab)
    small = max_windows(probe, v, idx[:3 * n_blob], grid, slab)
    whole = tuple(slab) == WHOLE
    assert (min(big) if whole else max(big)) > 64 * lanes, f"the huge triangles' windows {big} do not exceed {64 * lanes} lines"
    assert 0 < max(small) <= 64 * lanes, f"the blob's windows {small} exceed {64 * lanes} lines"
    if listed:                                             # the last chunk partial; on the whole grid at least three chunks
        assert max(big) % 2048 != 0 and (max(big) > 2 * 2048 or not whole), big
    return {(lanes, listed, "small"), (lanes, listed, "big"), ("combine", form)}


LANES = {"few": 16, "many": 1}


def case_cells(probe, name):
    kind, count, _ = CASES[name]
    v, idx, n_blob = mesh_of(kind)
    return cells_of(probe, v, idx, n_blob, grid_of(count), LANES[kind], "no list" not in name)


def z_cells(probe, count):
    v, idx = prism_and_sheet()
    lanes, _, form = path_of(probe, idx.size // 3, count)
    nzw = (count[2] + 31) // 32
    assert lanes == 16 and form == ("rows" if nzw in (1, 2, 64) else "serial"), (count, form)
    return {("combine", form), ("words per row", nzw)}


# ---- references, each computed once ----------------------------------------------------------------------------------------------------------
_REFERENCES = {}


def reference(key, v, idx, grid):
    if key not in _REFERENCES:
        want = orc.generate_grid_sdf(v, idx, grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count(), sign=0, semantics=orc.EXACT)
        want.setflags(write=False)
        assert (want < 0).any() and (want > 0).any(), key
        _REFERENCES[key] = want
    return _REFERENCES[key]


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a, F).view(U32).reshape(-1)


def assert_bit_equal(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    flips = np.flatnonzero((g ^ w) >> 31)
    assert bad.size == 0, f"{what}: {bad.size}/{g.size} cells differ, {flips.size} of them in the sign bit; first {bad[:6].tolist()}"


def slab_mask(grid, xs):
    nx, ny, nz = (int(c) for c in grid.get_cell_count())
    m = np.zeros((nx, ny, nz), bool)
    m[list(xs)] = True
    return m.reshape(-1)


def check_slab(call, grid, want, xs, what, **kw):
    """`call(out=..., **kw)` fills the layers xs of a pre-filled whole-grid array with the whole call's bits and leaves the rest alone."""
    out = np.full(want.size, FILL, F)
    call(out=out, **kw)
    inside = slab_mask(grid, xs)
    assert 0 < inside.sum() < inside.size
    assert_bit_equal(out[inside], want[inside], f"{what}: inside the slab")
    assert (out[~inside] == FILL).all(), f"{what}: cells outside the slab were written"


# ---- whole grids: lanes per triangle x list x window size ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_whole_grid(probe, name):
    kind, count, _ = CASES[name]
    v, idx, _ = mesh_of(kind)
    grid = grid_of(count)
    assert (idx.size // 3 > 16384) == (kind == "many") and (kind == "few" or (idx.size // 3) % 256 != 0)
    case_cells(probe, name)
    got = generate_grid_sdf(v, Topology.TriangleList(idx), grid, SignMethod.Raycast)
    assert_bit_equal(got, reference(name, v, idx, grid), name)


# ---- the z scan + majority: rows form and serial carry ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", Z_COUNTS, ids=lambda c: "x".join(map(str, c)))
def test_z_forms(probe, count):
    v, idx = prism_and_sheet()
    grid = grid_of(count, 1.0)
    z_cells(probe, count)
    want = reference(count, v, idx, grid)
    parity = orc.grid_ray_parity(v, idx, grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count()).reshape(*count, 3)
    assert all(parity[..., axis].any() and not parity[..., axis].all() for axis in range(3)), "every plane carries parity"
    nzw = (count[2] + 31) // 32
    odd_words = {int(z) // 32 for z in np.flatnonzero(parity[..., 2].any(axis=(0, 1)))}
    assert len(odd_words) >= min(nzw, 64), "the Z-lines' parity reaches every word of a row (but the one cell of a 65th)"
    decides = (parity[..., 0] != parity[..., 1]) & (parity[..., 2] == 1)        # inside by the Z-lines' vote
    deciding_words = {int(z) // 32 for z in np.flatnonzero(decides.any(axis=(0, 1)))}
    assert len(deciding_words) >= max(1, (nzw * 3) // 5) and min(deciding_words) <= 2, "the Z-lines' parity decides the majority in most words of a row, low ones included"
    got = generate_grid_sdf(v, Topology.TriangleList(idx), grid, SignMethod.Raycast)
    assert_bit_equal(got, want, f"prism and sheet in {count}")


# ---- slabs -----------------------------------------------------------------------------------------------------------------------------------------
def check_slab_shape(nx, x0, x1):
    """The x scan walks from nx - 1 down to x0 in steps of eight and a tail: both run, and neither as on the whole grid."""
    assert 0 < x0 < x1 < nx and (nx - x0) >= 8 and (nx - x0) % 8 not in (0, nx % 8), (nx, x0, x1)


@pytest.mark.parametrize("name", list(CASES))
def test_contiguous_slab(probe, name):
    kind, count, (x0, x1) = CASES[name]
    v, idx, n_blob = mesh_of(kind)
    grid = grid_of(count)
    check_slab_shape(count[0], x0, x1)
    cells_of(probe, v, idx, n_blob, grid, LANES[kind], "no list" not in name, (x0, x1, 31, 1, 0))      # big windows inside the slab too
    topo = Topology.TriangleList(idx)
    check_slab(lambda **kw: generate_grid_sdf(v, topo, grid, SignMethod.Raycast, **kw), grid, reference(name, v, idx, grid), range(x0, x1),
               f"{name}, slab ({x0}, {x1})", x_slab=(x0, x1))


@pytest.mark.parametrize("count", list(Z_SLABS), ids=lambda c: "x".join(map(str, c)))
def test_contiguous_slab_z_forms(probe, count):
    x0, x1 = Z_SLABS[count]
    v, idx = prism_and_sheet()
    grid = grid_of(count, 1.0)
    check_slab_shape(count[0], x0, x1)
    z_cells(probe, count)
    topo = Topology.TriangleList(idx)
    check_slab(lambda **kw: generate_grid_sdf(v, topo, grid, SignMethod.Raycast, **kw), grid, reference(count, v, idx, grid), range(x0, x1),
               f"prism and sheet in {count}, slab ({x0}, {x1})", x_slab=(x0, x1))


@pytest.mark.parametrize("name", list(INTERLEAVED))
def test_interleaved_slab(probe, name):
    kind, ny, nz, k = INTERLEAVED[name]
    grid, (x0, x1), period = interleaved_grid(ny, nz, k)
    assert period > 0
    nx = int(grid.get_cell_count()[0])
    xs = [x for x in range(nx) if x >= x0 and (x - x0) % period < x1 - x0]
    assert 0 < len(xs) < nx and max(xs) - min(xs) + 1 > len(xs), "the slab leaves layers out between its chunks"
    v, idx, n_blob = mesh_of(kind)
    listed = path_of(probe, idx.size // 3, (nx, ny, nz))[1]
    chunk_log = (x1 - x0).bit_length() - 1
    assert 1 << chunk_log == x1 - x0
    cells_of(probe, v, idx, n_blob, grid, LANES[kind], listed, (x0, max(xs) + 1, chunk_log, period, 0))
    dv, di = torch.as_tensor(v, device="cuda:0"), torch.as_tensor(idx.astype(np.int64), device="cuda:0")
    want = reference(name, v, idx, grid)
    out = torch.full((want.size,), float(FILL), dtype=torch.float32, device="cuda:0")
    generate_grid_sdf(dv, Topology.TriangleList(di), grid, SignMethod.Raycast, x_slab=(x0, x1), x_period=period, out=out)
    got, inside = out.cpu().numpy(), slab_mask(grid, xs)
    assert_bit_equal(got[inside], want[inside], f"{name}: inside the slab ({x0}, {x1}) every {period}")
    assert (got[~inside] == FILL).all(), f"{name}: cells outside the slab were written"


# ---- a resident mesh keeps whole-grid planes ----------------------------------------------------------------------------------------------------------
def test_resident_mesh(probe):
    name, other = "many, list", "many, no list"
    kind, count, (x0, x1) = CASES[name]
    v, idx, _ = mesh_of(kind)
    grid, grid2 = grid_of(count), grid_of(CASES[other][1])
    case_cells(probe, name)
    want, want2 = reference(name, v, idx, grid), reference(other, v, idx, grid2)
    with Mesh(v, Topology.TriangleList(idx)) as m:
        assert_bit_equal(m.generate_grid_sdf(grid, SignMethod.Raycast), want, "Mesh, first call")
        assert_bit_equal(m.generate_grid_sdf(grid2, SignMethod.Raycast), want2, "Mesh, another grid")
        assert_bit_equal(m.generate_grid_sdf(grid, SignMethod.Raycast), want, "Mesh, after a call on another grid")
        check_slab(lambda **kw: m.generate_grid_sdf(grid, SignMethod.Raycast, **kw), grid, want, range(x0, x1), "Mesh, slab", x_slab=(x0, x1))
    dv, di = torch.as_tensor(v, device="cuda:0"), torch.as_tensor(idx.astype(np.int64), device="cuda:0")
    with Mesh(dv, Topology.TriangleList(di)) as m:
        got = m.generate_grid_sdf(grid, SignMethod.Raycast)
        assert got.is_cuda
        assert_bit_equal(got, want, "Mesh, device tensors")


# ---- what reads the plane --------------------------------------------------------------------------------------------------------------------------
def test_consumers_of_the_plane(probe):
    name = "many, list"
    kind, count, _ = CASES[name]
    v, idx, _ = mesh_of(kind)
    grid = grid_of(count)
    case_cells(probe, name)
    want = reference(name, v, idx, grid)
    topo = Topology.TriangleList(idx)
    inside = (want < 0).reshape(count).astype(np.uint8)
    surface, solid = voxelize(v, topo, grid).occupancy, voxelize(v, topo, grid, True).occupancy
    assert np.array_equal(solid, surface | inside), "solid voxelization is not surface OR the oracle's ray-cast sign"
    assert (solid != surface).any() and inside.sum() > 0
    width = 0.3
    band = narrow_band_sdf(v, topo, grid, width, SignMethod.Raycast)
    cells = np.asarray(band.cells).astype(np.int64)
    assert np.array_equal(cells, np.flatnonzero((want >= -F(width)) & (want <= F(width)))), "the band's cells"
    assert np.array_equal(np.signbit(band.distances), np.signbit(want[cells])), "the band's signs"
    assert_bit_equal(band.distances, want[cells], "the band's distances")
    assert np.signbit(band.distances).any() and not np.signbit(band.distances).all()


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_cases_cover_every_path(probe, capsys):
    """Needs no device: every cell of {16 lanes, 1 lane} x {no list, list} x {small, big} windows, both combine forms and every count of
    words per row, with the case that owns it."""
    owner = {}
    for name in CASES:
        for cell in case_cells(probe, name):
            owner.setdefault(cell, name)
    for count in Z_COUNTS + list(Z_SLABS):
        for cell in z_cells(probe, count):
            owner.setdefault(cell, "z form " + "x".join(map(str, count)))
    matrix = {(lanes, listed, size) for lanes in (16, 1) for listed in (False, True) for size in ("small", "big")}
    matrix |= {("combine", "rows"), ("combine", "serial")} | {("words per row", w) for w in (1, 2, 3, 64, 65)}
    assert set(owner) == matrix, (matrix - set(owner), set(owner) - matrix)
    with capsys.disabled():
        print()
        for cell in sorted(matrix, key=str):
            print(f"[sign planes] {cell}: {owner[cell]}")
