"""The random band chains of tests/band_chain_cases.py, model only: conditions on the inputs of tests/test_gpu_band_chain.py.  Over the 12
seeds x 3 grid pairs (288 steps) of the first family and the 16 seeds x 3 pairs (384 steps) of the second, which has advect as a sixth
op, the chains must reach the states in which a handle made by one call can mislead the next: empty bands, but not too many; every op
on a non-empty band; the rare branches of each op's info; results of resample, of select and of advect that are consumed.  The figures
are printed (pytest -s) and quoted in DESIGN.md section 6; the first family's are pinned, so that an edit of the generator cannot shift
it silently."""
import numpy as np

import band_advect_model as am
import band_chain_cases as cc

FAMILIES = {"first": (cc.chain, cc.SEEDS, cc.OPS), "with advect": (cc.chain_b, cc.SEEDS_B, cc.OPS_B)}
# the first family as it has been since it was written: steps, empty inputs, and each op of cc.OPS on a non-empty input
PINNED = {"steps": 288, "empty input": 50, "csg on a non-empty input": 50, "filter on a non-empty input": 43, "redistance on a non-empty input": 57,
          "resample on a non-empty input": 43, "select on a non-empty input": 45}
RARE = ("filter n_nonfinite > 0", "redistance n_open > 0", "redistance n_open == 0, n_frozen > 0", "resample n_partial > 0",
        "resample to the other grid", "select of more than one component", "select drops cells", "select clears sign bits",
        "non-empty input -> empty output")


def _all(family):
    chain, seeds, _ = FAMILIES[family]
    return [(pair, seed, at, r) for pair in range(len(cc.PAIRS)) for seed in seeds for at, r in enumerate(chain(seed, pair)[2])]


def _figures(family):
    chain, seeds, ops = FAMILIES[family]
    steps = _all(family)
    by = lambda op: [r for _, _, _, r in steps if r.step[0] == op]                # noqa: E731
    full = lambda rs: [r for r in rs if r.source.cells.size]                       # noqa: E731
    pairs = [(a, b) for pair in range(len(cc.PAIRS)) for seed in seeds for a, b in zip(chain(seed, pair)[2], chain(seed, pair)[2][1:])]
    after = lambda op: sum(1 for a, _ in pairs if a.step[0] == op)                 # noqa: E731
    fig = {"steps": len(steps),
           "empty input": sum(1 for _, _, _, r in steps if r.source.cells.size == 0),
           "non-empty input -> empty output": sum(1 for _, _, _, r in steps if r.source.cells.size and r.band.cells.size == 0),
           "filter n_nonfinite > 0": sum(1 for r in by("filter") if r.info.n_nonfinite > 0),
           "redistance n_open > 0": sum(1 for r in by("redistance") if r.info.n_open > 0),
           "redistance n_open == 0, n_frozen > 0": sum(1 for r in by("redistance") if r.info.n_open == 0 and r.info.n_frozen > 0),
           "resample n_partial > 0": sum(1 for r in by("resample") if r.info.n_partial > 0),
           "resample to the other grid": sum(1 for r in by("resample") if r.grid != r.source_grid),
           "select of more than one component": sum(1 for r in by("select") if r.components.count > 1),
           "select drops cells": sum(1 for r in by("select") if r.info.n_dropped > 0),
           "select clears sign bits": sum(1 for r in by("select") if r.info.n_sign_cleared > 0),
           "consume a resample result": after("resample"),
           "consume a select result": after("select")}
    for op in ops:
        fig[f"{op} on a non-empty input"] = len(full(by(op)))
    if "advect" in ops:
        adv = full(by("advect"))
        fig.update({"advect by a velocity on a non-empty input": sum(1 for r in adv if cc.args(r.step)["kind"] == am.VELOCITY),
                    "advect by a normal speed on a non-empty input": sum(1 for r in adv if cc.args(r.step)["kind"] == am.NORMAL),
                    "advect n_nonfinite > 0": sum(1 for r in adv if r.info.n_nonfinite > 0),
                    "advect n_sign_flips > 0": sum(1 for r in adv if r.info.n_sign_flips > 0),
                    "advect 0 < n_moving < n": sum(1 for r in adv if 0 < r.info.n_moving < r.source.cells.size),
                    "consume a non-empty advect result": sum(1 for a, _ in pairs if a.step[0] == "advect" and a.band.cells.size),
                    "advect consumes another op's non-empty result": sum(1 for a, b in pairs if b.step[0] == "advect" and a.step[0] != "advect"
                                                                         and a.band.cells.size)})
    return fig


def test_the_plan_is_a_pure_function_of_seed_and_pair():
    for draw, plan, start_of, seeds in ((cc.draw, cc.plan, cc.start_of, cc.SEEDS), (cc.draw_b, cc.plan_b, cc.start_of_b, cc.SEEDS_B)):
        for pair in range(len(cc.PAIRS)):
            for seed in seeds:
                draw.cache_clear()
                first, start = plan(seed, pair), start_of(seed, pair)
                draw.cache_clear()
                assert plan(seed, pair) == first and start_of(seed, pair) == start and len(first) == cc.STEPS
        assert plan(0, 1) != plan(1, 1) and plan(0, 1) != plan(0, 2)
    assert cc.OPS == ("csg", "filter", "redistance", "resample", "select") and cc.OPS_B == cc.OPS + ("advect",)
    assert all(cc.plan(seed, pair) != cc.plan_b(seed, pair) for pair in range(len(cc.PAIRS)) for seed in cc.SEEDS)    # a stream of its own
    for pair, (a, b) in enumerate(cc.PAIRS):                                       # resample really changes grid
        assert all(a[f] != b[f] for f in range(3)) and all(x != y for f in range(2) for x, y in zip(a[f], b[f])), pair


def test_the_field_and_the_time_step_of_an_advect_step():
    """`field_of` and `dt_of` are what both sides of the GPU test call: one entry per cell in [-1, 1], the drawn share at rest in every
    component, nothing but the cells' indices read; dt a binary32 fraction of the smallest cell side."""
    step = next(s for seed in cc.SEEDS_B for s in cc.plan_b(seed, 2) if s[0] == "advect" and cc.args(s)["kind"] == am.VELOCITY)
    spec = cc.PAIRS[2][0]
    band = cc.pool(2, 0)[0]
    u = cc.field_of(step, band, spec)
    assert u.dtype == np.float32 and u.shape == (band.cells.size, 3) and np.abs(u).max() <= 1 and np.array_equal(u, cc.field_of(step, band, spec))
    rest = (u == 0).all(1)
    assert ((u == 0).any(1) == rest).all() and abs(rest.mean() - cc.args(step)["still"]) < 0.05
    part = type(band)(band.shape, band.cells[::3], band.distances[::3], None, 1.0, 1.0)             # the same cells get the same entries
    assert np.array_equal(cc.field_of(step, part, spec), u[::3])
    speed = cc.field_of(("advect",) + tuple((k, am.NORMAL if k == "kind" else v) for k, v in step[1:]), band, spec)
    assert speed.shape == (band.cells.size,) and np.array_equal(speed, u[:, 0])
    dt = cc.dt_of(step, spec)
    assert isinstance(dt, np.float32) and 0.2 * min(spec.cell) < dt < 0.9 * min(spec.cell)
    empty = type(band)(band.shape, [], [], None, 1.0, 1.0)
    assert cc.field_of(step, empty, spec).shape == (0, 3)


def _check(family):
    fig = _figures(family)
    ops = FAMILIES[family][2]
    for name, value in fig.items():
        print(f"{name}: {value}")
    assert fig["steps"] == cc.STEPS * len(cc.PAIRS) * len(FAMILIES[family][1])
    assert fig["empty input"] <= 0.2 * fig["steps"]
    for op in ops:
        assert fig[f"{op} on a non-empty input"] >= 40, op
    for name in RARE:
        assert fig[name] >= 3, name
    assert fig["consume a resample result"] >= 10 and fig["consume a select result"] >= 10
    return fig


def test_the_chains_reach_what_they_are_meant_to_reach():
    fig = _check("first")
    assert fig["steps"] == 288
    assert {name: fig[name] for name in PINNED} == PINNED


def test_the_chains_with_advect_reach_what_they_are_meant_to_reach():
    fig = _check("with advect")
    assert fig["steps"] == 384
    assert fig["advect by a velocity on a non-empty input"] >= 10 and fig["advect by a normal speed on a non-empty input"] >= 10
    for name in ("advect n_nonfinite > 0", "advect n_sign_flips > 0", "advect 0 < n_moving < n"):
        assert fig[name] >= 3, name
    assert fig["consume a non-empty advect result"] >= 10 and fig["advect consumes another op's non-empty result"] >= 10


def test_every_model_output_is_finite():
    for family in FAMILIES:
        for pair, seed, at, r in _all(family):
            assert np.isfinite(r.band.distances).all() and np.isfinite(r.band.bg_out) and np.isfinite(r.band.bg_in), \
                (family, cc.PAIR_IDS[pair], seed, at, cc.describe(r.step))
