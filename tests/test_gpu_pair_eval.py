"""The queued pairs' unsigned evaluation after it was rebuilt (distance.hip defer_flush: the three vertices and the class gathered in one
stage, the edge vectors formed per lane, the degenerate classes in a cold block behind the regular body — geo.hip.h
point_triangle_pair_dist2): every grid and every query bit-equal to the oracle, in every form that queues pairs — the packet walk with
M2S_DEFER 1, 2 and 3 and M2S_GATHER_AHEAD 0 and 1, the forced split walk, the packet groups, the queries' form — on trees of one to three
triangles, on a mesh whose batches mix regular and degenerate pairs (with and without a NaN and an inf vertex) and on blob-6k; on 16^3 and on
33 x 17 x 9, whose ragged bricks have lanes without a voxel in the permutes.  SignMethod.Normal, which keeps the gathered record, once."""
import numpy as np
import pytest

import oracle as orc
from mesh_to_sdf_amd import _lib
from mesh_to_sdf_amd import AccelerationMethod, Grid, SignMethod, Topology, generate_grid_sdf, generate_sdf, meshes

pytestmark = pytest.mark.gpu

PACKET_WALK = {"M2S_LANE_WALK": 0, "M2S_BRUTE_MAX": 0, "M2S_GROUP": 0, "M2S_SPLIT": 0}
SPLIT = {"M2S_DEFER": 3, "M2S_SPLIT": 2, "M2S_SPLIT_BUDGET": 24, "M2S_SPLIT_MIN_RECORDS": 4, "M2S_SPLIT_MAX_RECORDS": 64, "M2S_SPLIT_ROUNDS": 3,
         "M2S_CUT_MIN_PACKETS": 8}
GROUP = {"M2S_GROUP": 1, "M2S_CUT_MIN_PACKETS": 4000000000}     # M2S_DEFER stays automatic: a forced leaf-work form switches the groups off
GRIDS = [(16, 16, 16), (33, 17, 9)]

# the one-, two- and three-triangle meshes of tests/test_gpu_walk_diet.py
_V = np.array([[0.1, 0.2, 0.3], [1.3, 0.1, 0.5], [0.4, 1.2, 0.2], [1.1, 1.4, 1.0], [0.2, 0.9, 1.3], [1.5, 0.3, 1.4], [0.7, 0.6, 1.6]], np.float32)


def _mixed():
    """40 triangles over 60 random vertices of the unit cube, their classes alternating: regular, a == b == c, a == b, b == c (every
    fourth of that kind: a == c instead).  Small triangles scattered through the box, so every brick's pairs mix the classes, and the points
    and segments stand free of the regular triangles: nearest for the voxels around them, never for the others."""
    rng = np.random.default_rng(40)
    centre = rng.uniform(0.15, 0.85, (40, 1, 3))
    v = (centre + rng.uniform(-0.15, 0.15, (40, 3, 3))).astype(np.float32).reshape(-1, 3)
    idx = np.arange(120, dtype=np.uint32).reshape(40, 3)
    for t in range(40):
        a, b, c = idx[t]
        if t % 4 == 1: idx[t] = [a, a, a]
        elif t % 4 == 2: idx[t] = [a, a, c]
        elif t % 4 == 3: idx[t] = [a, b, b] if t % 16 != 15 else [a, b, a]
    return v, idx.reshape(-1)


def _mixed_nonfinite():
    v, idx = _mixed()
    v = v.copy()
    v[idx[3 * 8 + 1]] = [np.nan, 0.4, 0.5]      # a regular triangle's b
    v[idx[3 * 22 + 2]] = [0.5, np.inf, 0.5]     # an a == b segment's c
    return v, idx


MESHES = {"1 triangle": lambda: (_V, np.array([0, 1, 2], np.uint32)),
          "2 triangles": lambda: (_V, np.array([0, 1, 2, 1, 3, 2], np.uint32)),
          "3 triangles": lambda: (_V, np.array([0, 1, 2, 1, 3, 2, 4, 5, 6], np.uint32)),
          "mixed classes": _mixed,
          "mixed classes, NaN and inf": _mixed_nonfinite,
          "blob-6k": lambda: meshes.named("blob-6k")}


def bbox(name, v):
    if name.startswith("mixed"): v = _mixed()[0]          # the box of the finite form
    return meshes.extended_bbox(v, 0.1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size}/{want.size} differ, first {bad[:5]}"


_cache = {}


def grid_case(name, counts, sign=SignMethod.Raycast):
    """(vertices, indices, grid, the oracle's grid), computed once per shape and shared by the knob settings."""
    key = (name, tuple(counts), int(sign))
    if key not in _cache:
        v, idx = MESHES[name]()
        lo, hi = bbox(name, v)
        grid = Grid.from_bounding_box(lo, hi, list(counts))
        want = orc.generate_grid_sdf(v, idx, grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count(), sign=int(sign),
                                     semantics=orc.EXACT_BVH)
        _cache[key] = (v, idx, grid, want)
    return _cache[key]


def check_grid(name, counts, knobs, sign=SignMethod.Raycast):
    v, idx, grid, want = grid_case(name, counts, sign)
    with _lib.knobs(**{**PACKET_WALK, **knobs}):
        got = np.asarray(generate_grid_sdf(v, Topology.TriangleList(idx), grid, sign))
    assert_same_bits(got, want, f"{name} {counts} {sign.name} {knobs} against the oracle")


def test_the_mixed_mesh_is_what_it_says():
    # host only: the classes as the build will see them, and the degenerate triangles nearest for some voxels of the 16^3 grid and not for others
    v, idx = _mixed()
    t = v[idx.reshape(-1, 3).astype(np.int64)]
    ab, bc, ac = ((t[:, i] == t[:, j]).all(1) for i, j in ((0, 1), (1, 2), (0, 2)))
    cls = np.where(ab & bc, 1, np.where(ab, 2, np.where(bc | ac, 3, 0)))
    assert (cls == np.array([0, 1, 2, 3] * 10)).all() and ac.sum() == 10 + 2      # ten points, a == c twice
    _, _, grid, want = grid_case("mixed classes", GRIDS[0])
    regular = idx.reshape(-1, 3)[cls == 0].reshape(-1)
    alone = orc.generate_grid_sdf(v, regular, grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count(), sign=0, semantics=orc.EXACT_BVH)
    nearer = np.abs(want) < np.abs(alone)
    assert 0.2 < nearer.mean() < 0.8, nearer.mean()


@pytest.mark.parametrize("counts", GRIDS, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("name", list(MESHES))
def test_packet_walk_every_queued_form(name, counts):
    for defer in (1, 2, 3):
        for ahead in (0, 1):
            check_grid(name, counts, {"M2S_DEFER": defer, "M2S_GATHER_AHEAD": ahead})
            check_grid(name, counts, {"M2S_DEFER": defer, "M2S_GATHER_AHEAD": ahead, "M2S_CUT_MIN_PACKETS": 8})


@pytest.mark.parametrize("counts", GRIDS, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("name", list(MESHES))
def test_split_walk(name, counts):
    for ahead in (0, 1):
        check_grid(name, counts, {**SPLIT, "M2S_GATHER_AHEAD": ahead})


@pytest.mark.parametrize("counts", GRIDS, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("name", list(MESHES))
def test_packet_groups(name, counts):
    for ahead in (0, 1):
        check_grid(name, counts, {**GROUP, "M2S_GATHER_AHEAD": ahead})


@pytest.mark.parametrize("name", list(MESHES))
def test_query_form(name):
    v, idx = MESHES[name]()
    q = meshes.uniform_queries(*bbox(name, v), 5000)
    want = orc.generate_sdf(v, idx, q, accel=3, fast=True)
    for defer in (1, 2, 3):
        for ahead in (0, 1):
            for extra in ({}, {"M2S_QUERY_CUT_MIN": 1}):
                with _lib.knobs(**PACKET_WALK, **extra, M2S_DEFER=defer, M2S_GATHER_AHEAD=ahead):
                    got = np.asarray(generate_sdf(v, Topology.TriangleList(idx), q, AccelerationMethod.RtreeBvh))
                assert_same_bits(got, want, f"5 000 queries against {name}, M2S_DEFER={defer} M2S_GATHER_AHEAD={ahead} {extra}")


def test_normal_fold_keeps_the_gathered_record():
    for counts in GRIDS:
        for defer in (1, 2, 3):
            check_grid("blob-6k", counts, {"M2S_DEFER": defer}, SignMethod.Normal)
