"""The packet walks pass over their packet's seed triangle (distance.hip walk_span SEEDED, M2S_SEED_SKIP): the prologue has evaluated it for
every lane, every fold of the search state is an idempotent minimum, so leaving it out of the walk changes no bit.  Every grid and every query
under M2S_SEED_SKIP=1 is compared bit for bit with the oracle and with the same call under M2S_SEED_SKIP=0 — in every form of the packet walk
that evaluates a seed (M2S_DEFER 0 - 3, M2S_GATHER_AHEAD 0 and 1 where the form exists, cut lists on and off, the greedy-descent seed of a grid
too small for a seed lattice), the packet groups, the forced split walk (its first launch and its follow-up rounds never pass over the seed),
SignMethod Raycast and Normal, the queries' three-ray and nearest-with-normal forms — on trees of one to three triangles (one triangle: the
walk evaluates nothing, every value is the prologue's), a triangle present twice under two indices (same and opposite winding, either one
first: the lower index's sign must win the tie whichever of them is the seed), a mesh whose seeds can be points, segments or non-finite, and
blob-6k; with leaves of 1 to 16 triangles, so that the seed stands first, inside and last in a collapsed leaf; on 16^3, the ragged
33 x 17 x 9 and one x-slab call.  The lane walks did not get the skip."""
import ctypes

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
LISTS_ON, LISTS_OFF = {"M2S_CUT_MIN_PACKETS": 8}, {"M2S_CUT_MIN_PACKETS": 4000000000}
FORMS = [(0, 0), (1, 0), (2, 0), (3, 0), (3, 1)]                 # (M2S_DEFER, M2S_GATHER_AHEAD): the gather-ahead form exists for DEFER 3 only
GRIDS = [(16, 16, 16), (33, 17, 9)]
TINY = (7, 5, 4)                                                 # fewer than 8 packet bricks: no seed lattice, the greedy-descent seed

# the one-, two- and three-triangle meshes of tests/test_gpu_pair_eval.py
_V = np.array([[0.1, 0.2, 0.3], [1.3, 0.1, 0.5], [0.4, 1.2, 0.2], [1.1, 1.4, 1.0], [0.2, 0.9, 1.3], [1.5, 0.3, 1.4], [0.7, 0.6, 1.6]], np.float32)


def _mixed():
    """The "mixed classes" mesh of tests/test_gpu_pair_eval.py: 40 triangles over 60 random vertices of the unit cube, their classes
    alternating regular, a == b == c, a == b, b == c (every fourth of that kind: a == c) — a seed can be a point or a segment."""
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
          # one triangle under two indices: the same record twice, and with the winding turned (the same distance wherever a vertex is
          # nearest, the opposite normal), each with either copy first
          "twice": lambda: (_V, np.array([0, 1, 2, 0, 1, 2], np.uint32)),
          "twice, turned second": lambda: (_V, np.array([0, 1, 2, 0, 2, 1], np.uint32)),
          "twice, turned first": lambda: (_V, np.array([0, 2, 1, 0, 1, 2], np.uint32)),
          "twice and another": lambda: (_V, np.array([4, 5, 6, 0, 2, 1, 0, 1, 2], np.uint32)),
          "mixed classes": _mixed,
          "mixed classes, NaN and inf": _mixed_nonfinite,
          "blob-6k": lambda: meshes.named("blob-6k")}
SMALL = [n for n in MESHES if n != "blob-6k"]


def bbox(name, v):
    if name.startswith("mixed"): v = _mixed()[0]          # the box of the finite form
    return meshes.extended_bbox(v, 0.1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size}/{want.size} differ, first {bad[:5]}"


def skip_launches():
    fn = _lib.lib().m2s_debug_seed_skip_launches
    fn.restype, fn.argtypes = ctypes.c_uint64, []
    return int(fn())


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


def both(call, knobs, want, what, passes_over=True):
    """call() under `knobs` with M2S_SEED_SKIP 0 and 1: the same bits as each other and as `want`; the knob reaches the launches
    (`passes_over` None: not looked at — the forced split walk, whose plan may still launch a plain form on the smallest trees)."""
    got = {}
    for skip in (0, 1):
        before = skip_launches()
        with _lib.knobs(**knobs, M2S_SEED_SKIP=skip):
            got[skip] = np.asarray(call())
        told = skip_launches() - before
        if passes_over is not None:
            assert (told > 0) == (skip == 1 and passes_over), f"{what} M2S_SEED_SKIP={skip}: {told} launches told to pass over the seed"
    assert_same_bits(got[1], got[0], f"{what}: M2S_SEED_SKIP=1 against 0")
    assert_same_bits(got[1], want, f"{what}: M2S_SEED_SKIP=1 against the oracle")


def check_grid(name, counts, knobs, sign=SignMethod.Raycast, passes_over=True):
    if sign == SignMethod.Normal and "NaN" in name:
        # the reference panics here ("NaN distance": the oracle has no grid to compare with), and what the library reports must not depend
        # on whether the walk meets a non-finite seed again: the prologue's evaluation has recorded its NaN for every lane
        from mesh_to_sdf_amd import M2SPanic

        v, idx = MESHES[name]()
        grid = Grid.from_bounding_box(*bbox(name, v), list(counts))
        seen = {}
        for skip in (0, 1):
            with _lib.knobs(**{**PACKET_WALK, **knobs}, M2S_SEED_SKIP=skip):
                try:
                    seen[skip] = bits(np.asarray(generate_grid_sdf(v, Topology.TriangleList(idx), grid, sign))).tobytes()
                except M2SPanic as e:
                    seen[skip] = str(e)
        assert seen[0] == seen[1], f"{name} {counts} {sign.name} {knobs}: M2S_SEED_SKIP=1 against 0"
        return
    v, idx, grid, want = grid_case(name, counts, sign)
    both(lambda: generate_grid_sdf(v, Topology.TriangleList(idx), grid, sign), {**PACKET_WALK, **knobs}, want,
         f"{name} {counts} {sign.name} {knobs}", passes_over)


@pytest.mark.parametrize("counts", GRIDS, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("name", list(MESHES))
def test_packet_walk_every_form(name, counts):
    for defer, ahead in FORMS:
        for lists in (LISTS_ON, LISTS_OFF):
            check_grid(name, counts, {"M2S_DEFER": defer, "M2S_GATHER_AHEAD": ahead, **lists})


@pytest.mark.parametrize("name", ["twice, turned second", "twice, turned first", "mixed classes", "mixed classes, NaN and inf", "blob-6k"])
def test_packet_walk_normal_sign(name):
    for counts in GRIDS:
        for defer, ahead in FORMS:
            check_grid(name, counts, {"M2S_DEFER": defer, "M2S_GATHER_AHEAD": ahead, **LISTS_ON}, SignMethod.Normal)
        check_grid(name, counts, {"M2S_DEFER": 3, **LISTS_OFF}, SignMethod.Normal)


@pytest.mark.parametrize("name", list(MESHES))
def test_greedy_descent_seed(name):
    # no lattice: the seed is the first triangle of the leaf the descent ends in (k_packet), whatever the leaf size
    for leaf in (1, 2, 16):
        for defer, ahead in FORMS:
            check_grid(name, TINY, {"M2S_DEFER": defer, "M2S_GATHER_AHEAD": ahead, "M2S_LEAF_MAX": leaf})
        check_grid(name, TINY, {"M2S_DEFER": 3, "M2S_LEAF_MAX": leaf}, SignMethod.Normal)


@pytest.mark.parametrize("leaf", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("name", ["mixed classes", "blob-6k"])
def test_every_leaf_size(name, leaf):
    # the seed first, inside and last in a collapsed leaf: the lattice's seeds are spread over the leaves' triangles
    for defer, ahead in FORMS:
        for lists in (LISTS_ON, LISTS_OFF):
            check_grid(name, GRIDS[0], {"M2S_DEFER": defer, "M2S_GATHER_AHEAD": ahead, "M2S_LEAF_MAX": leaf, **lists})
    check_grid(name, GRIDS[1], {"M2S_DEFER": 3, "M2S_GATHER_AHEAD": 1, "M2S_LEAF_MAX": leaf, **LISTS_ON})
    check_grid(name, GRIDS[0], {"M2S_DEFER": 3, "M2S_LEAF_MAX": leaf, **LISTS_ON}, SignMethod.Normal)
    check_grid(name, GRIDS[0], {**GROUP, "M2S_LEAF_MAX": leaf})


@pytest.mark.parametrize("counts", GRIDS, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("name", list(MESHES))
def test_packet_groups(name, counts):
    check_grid(name, counts, GROUP)
    check_grid(name, counts, GROUP, SignMethod.Normal)


@pytest.mark.parametrize("counts", GRIDS, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("name", list(MESHES))
def test_split_walk_keeps_evaluating_the_seed(name, counts):
    # k_packet's split forms and k_split_round start from handed-over minima and pass "none": the knob changes nothing where they run
    check_grid(name, counts, SPLIT, passes_over=None)
    check_grid(name, counts, {**SPLIT, "M2S_DEFER": 1}, passes_over=None)


def test_split_walk_normal_sign():
    for counts in GRIDS:
        check_grid("blob-6k", counts, SPLIT, SignMethod.Normal, passes_over=None)


@pytest.mark.parametrize("name", list(MESHES))
def test_query_forms(name):
    v, idx = MESHES[name]()
    q = meshes.uniform_queries(*bbox(name, v), 5000)           # 78 full packets and one of 8 queries
    for method, accel in ((AccelerationMethod.RtreeBvh, 3), (AccelerationMethod.Rtree, 2)):     # three-ray sign; nearest with normal
        want = orc.generate_sdf(v, idx, q, accel=accel, fast=True)
        for defer, ahead in FORMS:
            if defer == 2: continue                            # a grid form
            for extra in ({}, {"M2S_QUERY_CUT_MIN": 1}):
                both(lambda: generate_sdf(v, Topology.TriangleList(idx), q, method), {**PACKET_WALK, **extra, "M2S_DEFER": defer, "M2S_GATHER_AHEAD": ahead},
                     want, f"5 000 queries against {name}, accel {accel}, M2S_DEFER={defer} M2S_GATHER_AHEAD={ahead} {extra}")


def test_one_x_slab():
    import torch

    for name, sign in (("mixed classes", SignMethod.Raycast), ("blob-6k", SignMethod.Raycast), ("blob-6k", SignMethod.Normal)):
        v, idx, grid, want = grid_case(name, GRIDS[1], sign)
        dv, di = torch.as_tensor(v, device="cuda"), torch.as_tensor(idx.astype(np.int64), device="cuda")
        x0, x1 = 5, 22
        cells = GRIDS[1][1] * GRIDS[1][2]

        def slab():
            out = torch.full((want.size,), float("nan"), device="cuda")
            generate_grid_sdf(dv, Topology.TriangleList(di), grid, sign, x_slab=(x0, x1), out=out)
            return out.cpu().numpy()[x0 * cells:x1 * cells]

        for lists in (LISTS_ON, LISTS_OFF):
            both(slab, {**PACKET_WALK, "M2S_DEFER": 3, **lists}, np.asarray(want).ravel()[x0 * cells:x1 * cells], f"{name} x-slab {sign.name} {lists}")


def test_the_knob():
    v, idx, grid, want = grid_case("blob-6k", GRIDS[0])
    call = lambda: generate_grid_sdf(v, Topology.TriangleList(idx), grid, SignMethod.Raycast)    # noqa: E731
    with _lib.knobs(**PACKET_WALK):
        assert int(_lib.describe_knobs()["M2S_SEED_SKIP"]) == -1
        before = skip_launches()
        assert_same_bits(np.asarray(call()), want, "automatic")
        assert skip_launches() > before                         # the automatic setting passes over the seed in every packet form
    for asked, held in ((7, 1), (-5, -1), (0, 0), (1, 1)):
        with _lib.knobs(M2S_SEED_SKIP=asked):
            assert int(_lib.describe_knobs()["M2S_SEED_SKIP"]) == held     # clamped to the documented values
