"""The inputs whose cut lists are recorded under tests/golden/cut_lists/ (tools/record_cut_lists.py writes them, tests/test_gpu_cut_lists.py
compares): small meshes in small grids, each in five forms of the grid call, and one query set with and without non-finite queries.  The
one copy of the case table, so that the recorder and the test cannot disagree about an input."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_model  # noqa: E402
from mesh_to_sdf_amd import Grid, meshes  # noqa: E402

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cut_lists")
CUT_WORDS = 16      # csrc/dist.hip.h: word 0 the number of ranges, then one word per range
CUT_MAX = 15
COARSE_WORDS = 64   # per block of 4 x 4 x 4 bricks: 8 sub-lists of 8 words

# every case walks in packets with cut lists, whatever its size: no tiny path, no lane walk, no groups, no split walk
BASE_KNOBS = {"M2S_CUT_MIN_PACKETS": 8, "M2S_LANE_WALK": 0, "M2S_BRUTE_MAX": 0, "M2S_GROUP": 0, "M2S_SPLIT": 0}
QUERY_KNOBS = {"M2S_QUERY_CUT_MIN": 1, "M2S_LANE_WALK": 0, "M2S_BRUTE_MAX": 0}
WAVE_CAP = 40


def _suzanne():
    d = np.load(os.path.join(os.path.dirname(GOLDEN), "suzanne.npz"))
    return d["vertices"].astype(F), d["indices"].astype(np.uint32)


def _sliver_blob():
    from test_gpu_closest import _sliver_meshes   # "blob with slivers", as tests/test_gpu_bounds.py takes it

    return list(_sliver_meshes())[1][1:]


def _nan_inf_blob():
    v, idx = meshes.blob(24, 13)
    v = v.copy()
    v[17, 1] = np.nan
    v[140, 0] = np.inf
    return v, idx


def _two_triangles():
    return np.random.default_rng(42).uniform(-1, 1, (6, 3)).astype(F), np.arange(6, dtype=np.uint32)


# name -> (mesh maker, cell counts, x-slab, (x_begin, x_end, x_period) of the interleaved slab)
GRID_CASES = {
    "blob-6k-48": (lambda: meshes.named("blob-6k"), (48, 48, 48), (16, 32), (0, 16, 32)),
    "blob-6k-ragged": (lambda: meshes.named("blob-6k"), (40, 52, 36), (8, 24), (8, 24, 16)),
    "suzanne-64": (_suzanne, (64, 64, 64), (16, 48), (0, 16, 32)),
    "sheet-48": (lambda: meshes.sheet(20, 20, rotate=False), (48, 48, 48), (16, 32), (0, 16, 32)),
    "degenerates-32": (lambda: sample_model.with_degenerates(*meshes.blob(12, 9)), (32, 32, 32), (8, 24), (0, 16, 16)),
    "slivers-32": (_sliver_blob, (32, 32, 32), (8, 24), (0, 16, 16)),
    "nan-inf-32": (_nan_inf_blob, (32, 32, 32), (8, 24), (0, 16, 16)),
    "two-triangles-32": (_two_triangles, (32, 32, 32), (8, 24), (0, 16, 16)),
}
FORMS = ("one-level", "two-level", "wave-cap", "x-slab", "interleaved")
PARITY_CASES = ("blob-6k-ragged", "suzanne-64", "sheet-48")   # these also go through generate_grid_sdf against the oracle


def mesh_of(name):
    v, idx = GRID_CASES[name][0]()
    return np.ascontiguousarray(v, F).reshape(-1, 3), np.ascontiguousarray(idx, np.uint32).reshape(-1)


def grid_of(name, v):
    """The grid over the extended box of the mesh's ordinary vertices (planted NaN, inf and overflowing ones left out)."""
    ok = np.isfinite(v).all(1) & (np.abs(v) < 1.0e3).all(1)
    lo, hi = meshes.extended_bbox(v[ok], 0.1)
    return Grid.from_bounding_box(lo, hi, list(GRID_CASES[name][1]))


def form_call(name, form):
    """(knobs, keyword arguments of Mesh.debug_cut_lists) of one form of a case."""
    _, _, slab, inter = GRID_CASES[name]
    knobs = dict(BASE_KNOBS)
    kw = {}
    if form == "two-level":
        knobs["M2S_CUT_COARSE"] = 1
    elif form == "wave-cap":
        knobs["M2S_CUT_WAVE_CAP"] = WAVE_CAP
    elif form == "x-slab":
        kw["x_slab"] = slab
    elif form == "interleaved":
        kw["x_slab"], kw["x_period"] = inter[:2], inter[2]
    else:
        knobs["M2S_CUT_COARSE"] = 0
    return knobs, kw


def query_sets():
    """name -> queries against blob-6k: 20 000 uniform ones, and the same with a few non-finite ones planted."""
    v, _ = meshes.named("blob-6k")
    lo, hi = meshes.extended_bbox(v, 0.1)
    q = meshes.uniform_queries(lo, hi, 20000)
    bad = q.copy()
    bad[5] = np.nan
    bad[4000, 1] = np.inf
    bad[12345, 2] = -np.inf
    bad[19999, 0] = np.nan
    return {"queries": q, "queries-non-finite": bad}


def list_ranges(words, n_nodes):
    """Decodes lists (n x 16 words) as k_packet does: counts (n), starts and lengths (n x 15, records; unused entries 0), and the length
    from which on a word holds a rounded-up value."""
    w = np.asarray(words, np.uint32).reshape(-1, CUT_WORDS).astype(np.int64)
    S = 1
    while S < 27 and (1 << S) < n_nodes:
        S += 1
    cnt = w[:, 0]
    r = w[:, 1:]
    start = r & ((1 << S) - 1)
    length = ((r >> S) & ((1 << (27 - S)) - 1)) << (r >> 27)
    used = np.arange(CUT_MAX)[None, :] < cnt[:, None]
    return cnt, np.where(used, start, 0), np.where(used, length, 0), 1 << (27 - S)
