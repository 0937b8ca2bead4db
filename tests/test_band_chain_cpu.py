"""The random band chains of tests/band_chain_cases.py, model only: conditions on the inputs of tests/test_gpu_band_chain.py.  Over the 12
seeds x 3 grid pairs (288 steps) the chains must reach the states in which a handle made by one call can mislead the next: empty
bands, but not too many; every op on a non-empty band; the rare branches of each op's info; results of resample and of select that
are consumed.  The figures are printed (pytest -s) and quoted in DESIGN.md section 6."""
import numpy as np

import band_chain_cases as cc


def _all():
    return [(pair, seed, at, r) for pair in range(len(cc.PAIRS)) for seed in cc.SEEDS for at, r in enumerate(cc.chain(seed, pair)[2])]


def _figures():
    steps = _all()
    by = lambda op: [r for _, _, _, r in steps if r.step[0] == op]                # noqa: E731
    full = lambda rs: [r for r in rs if r.source.cells.size]                       # noqa: E731
    after = lambda op: sum(1 for pair in range(len(cc.PAIRS)) for seed in cc.SEEDS                                     # noqa: E731
                           for a, b in zip(cc.chain(seed, pair)[2], cc.chain(seed, pair)[2][1:]) if a.step[0] == op)
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
    for op in cc.OPS:
        fig[f"{op} on a non-empty input"] = len(full(by(op)))
    return fig


def test_the_plan_is_a_pure_function_of_seed_and_pair():
    for pair in range(len(cc.PAIRS)):
        for seed in cc.SEEDS:
            cc.draw.cache_clear()
            first, start = cc.plan(seed, pair), cc.start_of(seed, pair)
            cc.draw.cache_clear()
            assert cc.plan(seed, pair) == first and cc.start_of(seed, pair) == start and len(first) == cc.STEPS
    assert cc.plan(0, 1) != cc.plan(1, 1) and cc.plan(0, 1) != cc.plan(0, 2)
    for pair, (a, b) in enumerate(cc.PAIRS):                                       # resample really changes grid
        assert all(a[f] != b[f] for f in range(3)) and all(x != y for f in range(2) for x, y in zip(a[f], b[f])), pair


def test_the_chains_reach_what_they_are_meant_to_reach():
    fig = _figures()
    for name, value in fig.items():
        print(f"{name}: {value}")
    assert fig["steps"] == 288
    assert fig["empty input"] <= 0.2 * fig["steps"]
    for op in cc.OPS:
        assert fig[f"{op} on a non-empty input"] >= 40, op
    for name in ("filter n_nonfinite > 0", "redistance n_open > 0", "redistance n_open == 0, n_frozen > 0", "resample n_partial > 0",
                 "resample to the other grid", "select of more than one component", "select drops cells", "select clears sign bits",
                 "non-empty input -> empty output"):
        assert fig[name] >= 3, name
    assert fig["consume a resample result"] >= 10 and fig["consume a select result"] >= 10


def test_every_model_output_is_finite():
    for pair, seed, at, r in _all():
        assert np.isfinite(r.band.distances).all() and np.isfinite(r.band.bg_out) and np.isfinite(r.band.bg_in), (cc.PAIR_IDS[pair], seed, at, cc.describe(r.step))
