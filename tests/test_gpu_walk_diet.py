"""The packet walk's node loop after its scalar bookkeeping was trimmed (distance.hip walk_span: the visit's three outcomes, the leaf's byte
cursor in place of the triangle count, the ring slot carried in byte units, the owner fetches by raw lane permutes): every grid and every
query bit-equal to the oracle, in the forced packet walk with M2S_GATHER_AHEAD 0 and 1, on the smallest shapes that reach each piece —
trees that are one leaf, leaves of every size the grid's leaf rule produces, ranges that end on a leaf, rings that fill several times per
packet, wrap past 128 and fill again inside one leaf, and the other forms that share walk_span (Normal fold, packet groups, split walk,
the queries' form)."""
import numpy as np
import pytest

import oracle as orc
from mesh_to_sdf_amd import _lib
from mesh_to_sdf_amd import AccelerationMethod, Grid, SignMethod, Topology, generate_grid_sdf, generate_sdf, meshes

pytestmark = pytest.mark.gpu

PACKET_WALK = {"M2S_DEFER": 3, "M2S_LANE_WALK": 0, "M2S_BRUTE_MAX": 0, "M2S_GROUP": 0, "M2S_SPLIT": 0}

# one, two and three triangles in general position (no axis-aligned edge, no shared plane): the tree is a single leaf record, a leaf of
# two, and a leaf of two beside a single one (or one leaf of three records' worth, by the grid's leaf size)
_V = np.array([[0.1, 0.2, 0.3], [1.3, 0.1, 0.5], [0.4, 1.2, 0.2], [1.1, 1.4, 1.0], [0.2, 0.9, 1.3], [1.5, 0.3, 1.4], [0.7, 0.6, 1.6]], np.float32)
TINY = {"1 triangle": (_V, np.array([0, 1, 2], np.uint32)),
        "2 triangles": (_V, np.array([0, 1, 2, 1, 3, 2], np.uint32)),
        "3 triangles": (_V, np.array([0, 1, 2, 1, 3, 2, 4, 5, 6], np.uint32))}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size}/{want.size} differ, first {bad[:5]}"


_cache = {}


def grid_case(name, mesh, counts, sign):
    """(vertices, indices, grid, the oracle's grid) — computed once per shape and shared by the knob settings."""
    key = (name, tuple(counts), int(sign))
    if key not in _cache:
        v, idx = mesh
        lo, hi = meshes.extended_bbox(v, 0.1)
        grid = Grid.from_bounding_box(lo, hi, list(counts))
        want = orc.generate_grid_sdf(v, idx, grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count(), sign=int(sign),
                                     semantics=orc.EXACT_BVH)
        _cache[key] = (v, idx, grid, want)
    return _cache[key]


def run_grid(name, mesh, counts, sign, extra, base=PACKET_WALK):
    v, idx, grid, want = grid_case(name, mesh, counts, sign)
    for ahead in (0, 1):
        with _lib.knobs(**{**base, **extra, "M2S_GATHER_AHEAD": ahead}):
            got = np.asarray(generate_grid_sdf(v, Topology.TriangleList(idx), grid, sign))
        assert_same_bits(got, want, f"{name} {counts} {sign.name} {extra} M2S_GATHER_AHEAD={ahead} against the oracle")


@pytest.mark.parametrize("n", [16, 40])
@pytest.mark.parametrize("name", list(TINY))
def test_trees_of_one_two_and_three_triangles(name, n):
    # the whole tree is one leaf (or a root over two): the range ends on the leaf it starts with
    run_grid(name, TINY[name], (n, n, n), SignMethod.Raycast, {})


@pytest.mark.parametrize("leaf_max", [None, 2, 4, 8, 16])
@pytest.mark.parametrize("n", [16, 40])
def test_suzanne_every_leaf_size(suzanne, n, leaf_max):
    # None: the size the grid's own rule picks (16^3: 15 triangles per brick -> 8; 40^3: one per brick -> 4); the others force every size the
    # rule can pick, so the cursor walks leaves of 1 .. 16 triangles with and without cut lists
    extra = {} if leaf_max is None else {"M2S_LEAF_MAX": leaf_max}
    run_grid("suzanne", suzanne, (n, n, n), SignMethod.Raycast, extra)
    run_grid("suzanne", suzanne, (n, n, n), SignMethod.Raycast, {**extra, "M2S_CUT_MIN_PACKETS": 8})


@pytest.mark.parametrize("counts", [(48, 48, 48), (33, 17, 9)])
@pytest.mark.parametrize("leaf_max", [None, 16])
def test_rings_fill_wrap_and_fill_again_inside_a_leaf(counts, leaf_max):
    # tens of triangles per brick: the first ring fills several times per packet and wraps past 128; with leaves of 16 and ~30 lanes per leaf
    # triangle it fills again inside one leaf while a batch is pending (the in-leaf consume of the gather-ahead form).  33 x 17 x 9: ragged
    # bricks, lanes without a voxel take part in the permutes.
    # Counted once with a library whose gather-ahead form counted them (an atomic per issue, not part of the product): of the batches issued,
    # those issued while an earlier batch of the SAME leaf was still pending (the in-leaf consume), and those whose ring had passed slot 128 —
    #   48^3, leaf size by the grid's rule (8)     67 957 issued, 43 808 in-leaf consumes, 31 810 past 128  (the same counts with cut lists + 5)
    #   48^3, leaves of 16                         114 750 / 93 861 / 53 853
    #   33 x 17 x 9 (the rule gives 16)             11 542 /  8 181 /  4 743
    extra = {} if leaf_max is None else {"M2S_LEAF_MAX": leaf_max}
    run_grid("blob-6k", meshes.named("blob-6k"), counts, SignMethod.Raycast, extra)
    run_grid("blob-6k", meshes.named("blob-6k"), counts, SignMethod.Raycast, {**extra, "M2S_CUT_MIN_PACKETS": 8})


def test_normal_fold():
    run_grid("blob-6k", meshes.named("blob-6k"), (32, 32, 32), SignMethod.Normal, {})
    run_grid("blob-6k", meshes.named("blob-6k"), (32, 32, 32), SignMethod.Normal, {"M2S_DEFER": 2})


def walk_choice(grid, n_tris):
    """(path, seeds, cut levels, group waves, split, split forced, defer, ...) the library picks for this grid under the knobs in force, for a
    resident tree with the leaf size the grid's own rule gives (host arithmetic: the test hooks of tests/test_capi_cpu.py)."""
    import ctypes as C

    lib = _lib.lib()
    leaves, out = (C.c_uint32 * 3)(), (C.c_uint32 * 8)()
    lib.m2s_debug_leaf_sizes.restype = lib.m2s_debug_grid_walk_choice.restype = C.c_int
    assert lib.m2s_debug_leaf_sizes(C.byref(grid._g), C.c_size_t(n_tris), C.c_size_t(0), leaves) == 0
    assert lib.m2s_debug_grid_walk_choice(C.byref(grid._g), C.c_size_t(n_tris), C.c_size_t(2 * n_tris - 1), C.c_uint32(leaves[0]), C.c_int(0), out) == 0
    return tuple(out)


def test_packet_groups():
    # M2S_DEFER stays automatic: a forced leaf-work form is a single-wave packet walk's and switches the groups off
    GROUP = 4
    base = {k: v for k, v in PACKET_WALK.items() if k != "M2S_DEFER"}
    extra = {"M2S_GROUP": 1, "M2S_CUT_MIN_PACKETS": 4000000000}
    v, idx, grid, _ = grid_case("blob-6k", meshes.named("blob-6k"), (32, 32, 32), SignMethod.Raycast)
    with _lib.knobs(**{**base, **extra}):
        choice = walk_choice(grid, idx.size // 3)
    assert choice[0] == GROUP and choice[3] == 4 and choice[6] == 3, choice     # k_packet_group, four waves per packet, leaf work fully queued
    with _lib.knobs(**{**PACKET_WALK, **extra}):
        assert walk_choice(grid, idx.size // 3)[0] != GROUP                     # (what this test ran before: not the groups)
    run_grid("blob-6k", meshes.named("blob-6k"), (32, 32, 32), SignMethod.Raycast, extra, base=base)
    run_grid("blob-6k", meshes.named("blob-6k"), (32, 32, 32), SignMethod.Normal, extra, base=base)


def test_split_walk():
    split = {"M2S_SPLIT": 2, "M2S_SPLIT_BUDGET": 24, "M2S_SPLIT_MIN_RECORDS": 4, "M2S_SPLIT_MAX_RECORDS": 64, "M2S_SPLIT_ROUNDS": 3}
    v, idx, grid, _ = grid_case("blob-6k", meshes.named("blob-6k"), (32, 32, 32), SignMethod.Raycast)
    with _lib.knobs(**{**PACKET_WALK, **split, "M2S_CUT_MIN_PACKETS": 8}):
        choice = walk_choice(grid, idx.size // 3)
    assert choice[4] == 1 and choice[5] == 1 and choice[6] == 3, choice         # the split walk, its flags raised from the start, DEFER 3
    run_grid("blob-6k", meshes.named("blob-6k"), (32, 32, 32), SignMethod.Raycast, {**split, "M2S_CUT_MIN_PACKETS": 8})
    run_grid("blob-6k", meshes.named("blob-6k"), (32, 32, 32), SignMethod.Normal, {**split, "M2S_CUT_MIN_PACKETS": 8})


def test_query_form(suzanne):
    v, idx = suzanne
    lo, hi = meshes.extended_bbox(v, 0.1)
    q = meshes.uniform_queries(lo, hi, 20000)
    want = orc.generate_sdf(v, idx, q, accel=3, fast=True)
    for ahead in (0, 1):
        for extra in ({}, {"M2S_QUERY_CUT_MIN": 1}):
            with _lib.knobs(**PACKET_WALK, **extra, M2S_GATHER_AHEAD=ahead):
                got = np.asarray(generate_sdf(v, Topology.TriangleList(idx), q, AccelerationMethod.RtreeBvh))
            assert_same_bits(got, want, f"20 000 queries against suzanne, {extra} M2S_GATHER_AHEAD={ahead}")
