"""The walks with their per-call constants resolved on the host (GridParams::sb_xl, nby, nbz, sy, sz; CutList::start_bits) and k_packet's
list word decoded behind the seed evaluation: the same bits as the oracle's EXACT semantics and as the same call made without cut lists, on
the smallest shapes at which a wrong constant shows — padding bricks and ragged last bricks, the narrow super-bricks of thin slabs, slabs
and interleaved slabs, brick shapes other than 4 x 4 x 4, trees on both sides of a change of the list words' start bits, and every walk
form that decodes bricks or list words.

An x-slab of 18 layers cannot be interleaved (a chunk is a power of two and a multiple of four packet bricks): the x_period cases use the
chunks of 16 layers that a 40^3 grid allows, one call with a single chunk from layer 5 and one with two chunks."""
import ctypes as C

import numpy as np
import pytest

import oracle as orc
from mesh_to_sdf_amd import _lib
from mesh_to_sdf_amd import AccelerationMethod, Grid, SignMethod, Topology, generate_grid_sdf, generate_sdf, meshes
from mesh_to_sdf_amd._lib import M2SGrid, M2SOpts

pytestmark = pytest.mark.gpu

PACKET_WALK = {"M2S_LANE_WALK": 0, "M2S_BRUTE_MAX": 0, "M2S_GROUP": 0, "M2S_SPLIT": 0}
LISTS = {"M2S_CUT_MIN_PACKETS": 0}
NO_LISTS = {"M2S_CUT_MIN_PACKETS": 4000000000}
SIGNS = [SignMethod.Raycast, SignMethod.Normal]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    got, want = np.asarray(got, np.float32).ravel(), np.asarray(want, np.float32).ravel()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: {bad.size}/{want.size} differ, first {bad[:5]}: got {got[bad[:5]]} want {want[bad[:5]]}"


_mesh = {}
_want = {}


def mesh_prefix(n_tris=None):
    """blob-6k, or the first n_tris triangles of its list (an open surface: the tree has 2 n_tris - 1 records)."""
    if "full" not in _mesh:
        _mesh["full"] = meshes.named("blob-6k")
    v, idx = _mesh["full"]
    return (v, idx) if n_tris is None else (v, np.ascontiguousarray(idx[: 3 * n_tris]))


def cubic_grid(counts):
    """`counts` cubic cells around the mesh, as small as still cover its extended box: the packet brick is 4 x 4 x 4 cells whatever the counts."""
    lo, hi = meshes.extended_bbox(mesh_prefix()[0], 0.1)
    s = np.float32(max((hi[k] - lo[k]) / counts[k] for k in range(3)))
    first = [np.float32(0.5) * (lo[k] + hi[k]) - np.float32(0.5 * (counts[k] - 1)) * s for k in range(3)]
    return Grid(first, [s, s, s], list(counts))


def oracle_grid(key, v, idx, grid, sign):
    """The oracle's EXACT grid (every cell the brute-force minimum over all triangles), computed once per case and left unchanged."""
    key = (key, int(sign))
    if key not in _want:
        _want[key] = orc.generate_grid_sdf(v, idx, grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count(), sign=int(sign),
                                           semantics=orc.EXACT)
        _want[key].setflags(write=False)
    return _want[key]


def walk_consts(grid, slab=None, x_period=0):
    """What the host resolves for this call (test hook m2s_debug_walk_consts)."""
    fn = _lib.lib().m2s_debug_walk_consts
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(M2SGrid), C.POINTER(M2SOpts), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    o = M2SOpts()
    o.struct_size = C.sizeof(M2SOpts)
    if slab is not None:
        o.x_begin, o.x_end = slab
    o.x_period = x_period
    out = (C.c_uint32 * 12)()
    assert fn(C.byref(grid._g), C.byref(o), 0, 1, out) == 0, _lib.last_error()
    return dict(zip(("sb_xl", "nby", "nbz", "sy", "sz", "sz_magic", "sy_magic", "start_bits", "bl0", "bl1", "bl2", "nbx"), (int(x) for x in out)))


def run_whole_grid(key, v, idx, grid, sign, forms):
    """The call under each knob set of `forms`, each against the oracle; then all against the first."""
    want = oracle_grid(key, v, idx, grid, sign)
    got = {}
    for name, extra in forms.items():
        with _lib.knobs(**{**PACKET_WALK, **extra}):
            got[name] = np.asarray(generate_grid_sdf(v, Topology.TriangleList(idx), grid, sign))
        assert_same_bits(got[name], want, f"{key} {sign.name} {name} against the oracle")
    first = next(iter(forms))
    for name in forms:
        assert_same_bits(got[name], got[first], f"{key} {sign.name}: {name} against {first}")


@pytest.mark.parametrize("sign", SIGNS, ids=lambda s: s.name)
@pytest.mark.parametrize("counts", [(20, 36, 52), (8, 64, 64), (4, 40, 40)], ids=lambda c: "x".join(map(str, c)))
def test_grid_shapes(counts, sign):
    # 20 x 36 x 52: 5 x 9 x 13 bricks, no axis a whole number of super-bricks (padding bricks in y and z, super-bricks one brick wide);
    # 8 x 64 x 64 and 4 x 40 x 40: two bricks and one along x, the narrow super-bricks
    v, idx = mesh_prefix()
    grid = cubic_grid(counts)
    c = walk_consts(grid)
    assert c["sb_xl"] == {20: 0, 8: 1, 4: 0}[counts[0]] and (c["nby"], c["nbz"]) == ((counts[1] + 3) // 4, (counts[2] + 3) // 4)
    run_whole_grid(counts, v, idx, grid, sign, {"cut lists": LISTS, "whole tree": NO_LISTS})


@pytest.mark.parametrize("sign", SIGNS, ids=lambda s: s.name)
@pytest.mark.parametrize("slab", [(5, 23, 0), (5, 21, 48), (8, 24, 16)], ids=["x 5..23", "x 5..21 period 48", "x 8..24 period 16"])
def test_x_slabs(slab, sign):
    # (5, 23): a slab that starts and ends inside bricks of the grid; with a period the call owns chunks of 16 layers: [5, 21) alone
    # (the next one would start beyond the grid), [8, 24) and [24, 40)
    import torch

    xb, xe, period = slab
    v, idx = mesh_prefix()
    grid = cubic_grid((40, 40, 40))
    want = oracle_grid((40, 40, 40), v, idx, grid, sign).reshape(40, 1600)
    owned = np.zeros(40, bool)
    for start in range(xb, 40, period or 40):
        owned[start:start + (xe - xb)] = True
    assert owned.sum() == (32 if period == 16 else xe - xb)
    dv, di = torch.as_tensor(v, device="cuda:0"), torch.as_tensor(idx.astype(np.int64), device="cuda:0")
    got = {}
    for name, extra in (("cut lists", LISTS), ("whole tree", NO_LISTS)):
        out = torch.full((40 * 1600,), float("nan"), dtype=torch.float32, device="cuda:0")
        with _lib.knobs(**{**PACKET_WALK, **extra}):
            generate_grid_sdf(dv, Topology.TriangleList(di), grid, sign, x_slab=(xb, xe), x_period=period, out=out)
        got[name] = out.cpu().numpy().reshape(40, 1600)
        assert_same_bits(got[name][owned], want[owned], f"slab {slab} {sign.name} {name} against the oracle")
        assert np.isnan(got[name][~owned]).all(), f"slab {slab} {sign.name} {name}: cells outside the slab were written"
    assert_same_bits(got["cut lists"], got["whole tree"], f"slab {slab} {sign.name}: cut lists against the whole tree")


@pytest.mark.parametrize("sign", SIGNS, ids=lambda s: s.name)
@pytest.mark.parametrize("ratio", [(4, 2, 1), (1, 2, 4)], ids=["bricks 2x4x8", "bricks 8x4x2"])
def test_anisotropic_bricks(ratio, sign):
    # cell sizes 4 : 2 : 1 make the packet brick 2 x 4 x 8 cells (logs 1, 2, 3), 1 : 2 : 4 the other way round; ragged on every axis
    v, idx = mesh_prefix()
    lo, hi = meshes.extended_bbox(v, 0.1)
    s = np.float32((hi - lo).max() / 45.0)
    size = np.array(ratio, np.float32) * s
    counts = [int(np.ceil((hi[k] - lo[k]) / size[k])) for k in range(3)]
    grid = Grid(lo + np.float32(0.5) * size, size, counts)
    c = walk_consts(grid)
    assert (c["bl0"], c["bl1"], c["bl2"]) == ((1, 2, 3) if ratio[0] == 4 else (3, 2, 1)), c
    run_whole_grid(("anisotropic", ratio), v, idx, grid, sign, {"cut lists": LISTS, "whole tree": NO_LISTS})


@pytest.mark.parametrize("sign", SIGNS, ids=lambda s: s.name)
@pytest.mark.parametrize("n_tris", [512, 513, 4096, 4097])
def test_tree_sizes_around_a_change_of_the_start_bits(n_tris, sign):
    # 2 T - 1 records: 1 023 and 1 025, 8 191 and 8 193 — 10 and 11, 13 and 14 start bits
    v, idx = mesh_prefix(n_tris)
    grid = cubic_grid((40, 40, 40))
    want_bits = {512: 10, 513: 11, 4096: 13, 4097: 14}[n_tris]
    fn = _lib.lib().m2s_debug_walk_consts
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(M2SGrid), C.POINTER(M2SOpts), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    out = (C.c_uint32 * 12)()
    assert fn(C.byref(grid._g), None, 0, 2 * n_tris - 1, out) == 0 and int(out[7]) == want_bits
    run_whole_grid(("prefix", n_tris), v, idx, grid, sign, {"cut lists": LISTS, "whole tree": NO_LISTS})


FORMS = {
    "two-level lists": {**LISTS, "M2S_CUT_COARSE": 1},
    "packet groups": {**NO_LISTS, "M2S_GROUP": 1},
    # (a budget of 24 work units: every packet that lasts longer hands the rest of its ranges to k_split_round, which decodes the list again)
    "split walk": {**LISTS, "M2S_SPLIT": 2, "M2S_SPLIT_BUDGET": 24, "M2S_SPLIT_MIN_RECORDS": 4, "M2S_SPLIT_MAX_RECORDS": 64, "M2S_SPLIT_ROUNDS": 3},
    "lane walk": {"M2S_LANE_WALK": 1},
}


@pytest.mark.parametrize("sign", SIGNS, ids=lambda s: s.name)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_forced_forms(form, sign):
    # every kernel that decodes bricks or list words besides the plain k_packet: k_cut in two levels, k_packet_group, the split walk's
    # k_packet / k_split_round / k_split_finish, k_lane — on the grid with padding bricks
    v, idx = mesh_prefix()
    grid = cubic_grid((20, 36, 52))
    run_whole_grid((20, 36, 52), v, idx, grid, sign, {"whole tree": NO_LISTS, form: FORMS[form]})


@pytest.mark.parametrize("accel", ["RtreeBvh", "Bvh(Normal)"])
def test_queries(accel):
    # 5 000 queries scattered over the box (the call sorts them along the Morton curve into packets), one cut list per packet
    v, idx = mesh_prefix()
    lo, hi = meshes.extended_bbox(v, 0.1)
    q = meshes.uniform_queries(lo, hi, 5000)
    method, o_accel, o_sign = {"RtreeBvh": (AccelerationMethod.RtreeBvh, 3, 0), "Bvh(Normal)": (AccelerationMethod.Bvh(SignMethod.Normal), 1, 1)}[accel]
    want = orc.generate_sdf(v, idx, q, accel=o_accel, sign=o_sign)
    got = {}
    for name, extra in (("cut lists", {"M2S_QUERY_CUT_MIN": 0}), ("whole tree", {"M2S_QUERY_CUT_MIN": 4000000000})):
        with _lib.knobs(**{**PACKET_WALK, **extra}):
            got[name] = np.asarray(generate_sdf(v, Topology.TriangleList(idx), q, method))
        assert_same_bits(got[name], want, f"5 000 queries {accel} {name} against the oracle")
    assert_same_bits(got["cut lists"], got["whole tree"], f"5 000 queries {accel}: cut lists against the whole tree")
