"""The packet walk with its queued pre-tests' gathers issued ahead of their use (distance.hip PretestAhead, M2S_GATHER_AHEAD): the same bits as
the oracle and as the walk that issues them where it uses them, on the smallest shapes that reach each edge of the pipeline — no batch ever
issued, a batch pending at the end of a range and at the drain, several insertions per leaf while one is pending, the Normal fold's three-slot
layout, the query form of the kernel, and bricks whose last lanes have no voxel."""
import numpy as np
import pytest

import oracle as orc
from mesh_to_sdf_amd import _lib
from mesh_to_sdf_amd import AccelerationMethod, Grid, SignMethod, Topology, generate_grid_sdf, generate_sdf, meshes

pytestmark = pytest.mark.gpu

PACKET_WALK = {"M2S_DEFER": 3, "M2S_LANE_WALK": 0, "M2S_BRUTE_MAX": 0, "M2S_GROUP": 0, "M2S_SPLIT": 0}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size}/{want.size} differ, first {bad[:5]}"


def ga_launches():
    """Launches of k_packet's gather-ahead form by this process so far (test hook of the library)."""
    import ctypes

    fn = _lib.lib().m2s_debug_gather_ahead_launches
    fn.restype, fn.argtypes = ctypes.c_uint64, []
    return int(fn())


def run_with_knob(ahead, knobs, call):
    """call() under the forced packet walk with M2S_GATHER_AHEAD=ahead; checks that the form the knob names is the one that was launched."""
    with _lib.knobs(**PACKET_WALK, **knobs, M2S_GATHER_AHEAD=ahead):
        before = ga_launches()
        got = np.asarray(call())
        launched = ga_launches() - before
    assert (launched > 0) == (ahead == 1), f"M2S_GATHER_AHEAD={ahead}: {launched} launches of the gather-ahead form"
    return got


_cache = {}


def grid_case(mesh, counts, sign):
    """(vertices, indices, grid, the oracle's grid) — computed once per shape and shared by the knob settings."""
    key = (mesh, tuple(counts), int(sign))
    if key not in _cache:
        v, idx = meshes.cube() if mesh == "cube" else meshes.named(mesh)
        lo, hi = meshes.extended_bbox(v, 0.1)
        grid = Grid.from_bounding_box(lo, hi, list(counts))
        want = orc.generate_grid_sdf(v, idx, grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count(), sign=int(sign),
                                     semantics=orc.EXACT_BVH)
        _cache[key] = (v, idx, grid, want)
    return _cache[key]


def run_grid(mesh, counts, sign, extra):
    v, idx, grid, want = grid_case(mesh, counts, sign)
    got = {}
    for ahead in (0, 1):
        got[ahead] = run_with_knob(ahead, extra, lambda: generate_grid_sdf(v, Topology.TriangleList(idx), grid, sign))
        assert_same_bits(got[ahead], want, f"{mesh} {counts} {sign.name} {extra} M2S_GATHER_AHEAD={ahead} against the oracle")
    assert_same_bits(got[1], got[0], f"{mesh} {counts} {sign.name} {extra}: knob 1 against knob 0")


def test_never_fills_a_batch():
    # 12 triangles, 64 bricks: nothing is ever issued ahead and the drain sees fewer than 64 pairs
    run_grid("cube", (16, 16, 16), SignMethod.Raycast, {})


@pytest.mark.parametrize("n", [24, 40])
@pytest.mark.parametrize("lists", ["cut lists", "whole tree"])
def test_batches_pending_across_ranges_and_at_the_drain(n, lists):
    # tens of triangles per brick: many batches per packet, the rings wrap; with lists a packet walks several ranges and a batch stays pending
    # from one into the next
    run_grid("blob-6k", (n, n, n), SignMethod.Raycast, {"M2S_CUT_MIN_PACKETS": 8} if lists == "cut lists" else {})


def test_long_leaves():
    # leaves of up to 8 triangles: several insertions per leaf, the ring fills again while a batch is pending
    run_grid("blob-6k", (24, 24, 24), SignMethod.Raycast, {"M2S_LEAF_MAX": 8})


def test_normal_fold():
    run_grid("blob-11k", (32, 32, 32), SignMethod.Normal, {})


def test_non_cubic_grid_with_partial_bricks():
    # 21 x 18 x 10: the last bricks of every axis reach outside, their lanes without a voxel take part in the permutes
    run_grid("blob-6k", (21, 18, 10), SignMethod.Raycast, {})


def test_query_form():
    v, idx = meshes.named("blob-6k")
    lo, hi = meshes.extended_bbox(v, 0.1)
    q = meshes.uniform_queries(lo, hi, 20000)
    want = orc.generate_sdf(v, idx, q, accel=3, fast=True)
    got = {}
    for ahead in (0, 1):
        got[ahead] = run_with_knob(ahead, {"M2S_QUERY_CUT_MIN": 1}, lambda: generate_sdf(v, Topology.TriangleList(idx), q, AccelerationMethod.RtreeBvh))
        assert_same_bits(got[ahead], want, f"20 000 queries, M2S_GATHER_AHEAD={ahead} against the oracle")
    assert_same_bits(got[1], got[0], "20 000 queries: knob 1 against knob 0")


def test_automatic_setting_takes_the_measured_forms_only():
    # -1: the grid walk of the unsigned distance and the queries' walk with the three-ray sign run the gather-ahead form, the Normal fold does not
    v, idx, grid, _ = grid_case("blob-6k", (24, 24, 24), SignMethod.Raycast)
    lo, hi = meshes.extended_bbox(v, 0.1)
    q = meshes.uniform_queries(lo, hi, 20000)
    calls = {"grid Raycast": (lambda: generate_grid_sdf(v, Topology.TriangleList(idx), grid, SignMethod.Raycast), True),
             "grid Normal": (lambda: generate_grid_sdf(v, Topology.TriangleList(idx), grid, SignMethod.Normal), False),
             "queries RtreeBvh": (lambda: generate_sdf(v, Topology.TriangleList(idx), q, AccelerationMethod.RtreeBvh), True),
             "queries Rtree": (lambda: generate_sdf(v, Topology.TriangleList(idx), q, AccelerationMethod.Rtree), False)}
    with _lib.knobs(**PACKET_WALK, M2S_GATHER_AHEAD=-1):
        for what, (call, ahead) in calls.items():
            before = ga_launches()
            call()
            assert (ga_launches() - before > 0) == ahead, what
    with _lib.knobs(M2S_GATHER_AHEAD=7):
        assert int(_lib.describe_knobs()["M2S_GATHER_AHEAD"]) == 1     # clamped to the documented values
