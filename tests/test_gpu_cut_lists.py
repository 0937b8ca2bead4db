"""k_cut's lists, word for word.  The lists a call leaves (test hook m2s_debug_cut_lists: the call's own steps up to and including k_cut) are
compared with the lists recorded under tests/golden/cut_lists/ by tools/record_cut_lists.py, on the kernel as it was before its node loop
moved its bookkeeping to the scalar unit: small meshes in small grids (tests/cut_list_cases.py), each in five forms — one level, two levels,
a visit cap of 40 so that the cap decides, an x-slab, an interleaved slab — and the lists of a query set with and without non-finite queries.
The recorded set itself must hold a saturated list, a single-range list and a wave that reached the cap.  Three of the cases also go
through generate_grid_sdf against the oracle, bit for bit, with and without lists."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bounds_model as bm  # noqa: E402
import cut_list_cases as cc  # noqa: E402
import oracle as orc  # noqa: E402
from mesh_to_sdf_amd import Mesh, SignMethod, Topology, _lib, generate_grid_sdf, meshes  # noqa: E402

pytestmark = pytest.mark.gpu

_golden = {}


def golden(name):
    if name not in _golden:
        with np.load(os.path.join(cc.GOLDEN, name + ".npz")) as d:
            _golden[name] = {k: d[k] for k in d.files}
    return _golden[name]


def assert_same_words(got, want, what, per):
    assert got.size == want.size, f"{what}: {got.size} words, recorded {want.size}"
    bad = np.flatnonzero((got.reshape(-1, per) != want.reshape(-1, per)).any(1))
    assert bad.size == 0, (f"{what}: {bad.size} of {want.size // per} lists differ; first {bad[0]}: got {got.reshape(-1, per)[bad[0]].tolist()}, "
                           f"recorded {want.reshape(-1, per)[bad[0]].tolist()}")


@pytest.fixture(scope="module")
def case_mesh():
    """name -> (resident mesh, grid) of a grid case, built once and shared by its forms."""
    made = {}

    def get(name):
        if name not in made:
            v, idx = cc.mesh_of(name)
            made[name] = (Mesh(v, Topology.TriangleList(idx)), cc.grid_of(name, v))
        return made[name]

    yield get
    for m, _ in made.values():
        m.close()


@pytest.mark.parametrize("form", cc.FORMS)
@pytest.mark.parametrize("name", list(cc.GRID_CASES))
def test_grid_lists_equal_the_recorded_ones(case_mesh, name, form):
    m, grid = case_mesh(name)
    knobs, kw = cc.form_call(name, form)
    with _lib.knobs(**knobs):
        got = m.debug_cut_lists(grid, **kw)
        coarse = m.debug_cut_lists(grid, coarse=True, **kw) if form == "two-level" else None
    want = golden(name)
    assert want[form].size > 0 and want[form].size % cc.CUT_WORDS == 0
    assert_same_words(got, want[form], f"{name}, {form}", cc.CUT_WORDS)
    if coarse is not None:
        assert want[form + ".coarse"].size > 0
        assert_same_words(coarse, want[form + ".coarse"], f"{name}, {form}, coarse records", 8)


@pytest.mark.parametrize("name", ["queries", "queries-non-finite"])
def test_query_lists_equal_the_recorded_ones(name):
    v, idx = meshes.named("blob-6k")
    q = cc.query_sets()[name]
    with Mesh(v, Topology.TriangleList(idx)) as m, _lib.knobs(**cc.QUERY_KNOBS):
        got = m.debug_cut_lists(queries=q)
    want = golden("queries")[name]
    assert want.size >= (q.shape[0] // 64) * cc.CUT_WORDS
    assert_same_words(got, want, name, cc.CUT_WORDS)


def test_recorded_set_holds_the_edge_cases(case_mesh):
    """A list of 15 ranges, a list of one range, and a wave that reached the visit cap: in the capped form some list differs from the
    uncapped one and ends in a range longer than the subtree at its start (past the cap a wave emits whatever it meets, and what it
    meets next to the last range merges into it)."""
    saturated, single, capped = [], [], []
    for name in cc.GRID_CASES:
        g = golden(name)
        for form in cc.FORMS:
            w = g[form].reshape(-1, cc.CUT_WORDS)
            assert (w[:, 0] >= 1).all() and (w[:, 0] <= cc.CUT_MAX).all(), f"{name}, {form}: a list without ranges or with too many"
            if (w[:, 0] == cc.CUT_MAX).any():
                saturated.append((name, form))
            if (w[:, 0] == 1).any():
                single.append((name, form))
        m, _ = case_mesh(name)
        skip = m.debug_arrays(bm.DTYPES)["nodes"]["skip"].astype(np.int64)
        cnt, start, length, exact_below = cc.list_ranges(g["wave-cap"], skip.size)
        rows = np.arange(cnt.size)
        last_start, last_len = start[rows, cnt - 1], length[rows, cnt - 1]
        differs = (g["wave-cap"].reshape(-1, cc.CUT_WORDS) != g["one-level"].reshape(-1, cc.CUT_WORDS)).any(1)
        # (an unsaturated list — a saturated one grows its last range for another reason — and a length the word holds exactly)
        if (differs & (cnt < cc.CUT_MAX) & (last_len < exact_below) & (last_len > skip[last_start] - last_start)).any():
            capped.append(name)
    print(f"15 ranges: {saturated}\none range: {single}\ncap reached: {capped}")
    assert saturated, "no recorded list has 15 ranges"
    assert single, "no recorded list has a single range"
    assert capped, "no recorded wave reached the visit cap"


_PARITY_KNOBS = [{}, {"M2S_CUT_MIN_PACKETS": 8, "M2S_LANE_WALK": 0, "M2S_BRUTE_MAX": 0, "M2S_GROUP": 0, "M2S_SPLIT": 0},
                 {"M2S_CUT_MIN_PACKETS": 8, "M2S_LANE_WALK": 0, "M2S_BRUTE_MAX": 0, "M2S_GROUP": 0, "M2S_SPLIT": 0, "M2S_CUT_COARSE": 1}]


@pytest.mark.parametrize("name", cc.PARITY_CASES)
def test_grid_results_equal_the_oracle(name):
    """generate_grid_sdf with the default knobs, with cut lists on every grid, and with two-level lists: the oracle's bits each time."""
    v, idx = cc.mesh_of(name)
    grid = cc.grid_of(name, v)
    want = orc.generate_grid_sdf(v, idx, grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count(), sign=int(SignMethod.Raycast),
                                 semantics=orc.EXACT_BVH)
    for knobs in _PARITY_KNOBS:
        with _lib.knobs(**knobs):
            got = np.asarray(generate_grid_sdf(v, Topology.TriangleList(idx), grid, SignMethod.Raycast))
        bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
        assert bad.size == 0, f"{name}, knobs {knobs}: {bad.size} of {want.size} cells differ from the oracle, first {bad[:5]}"
