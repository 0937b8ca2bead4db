#!/usr/bin/env python3
"""Records the cut lists of the cases of tests/cut_list_cases.py under tests/golden/cut_lists/ (needs the GPU): one .npz per grid case with
the lists of every form (and the coarse records of the two-level form), queries.npz with the lists of the two query sets.  Run it on the
commit whose lists are to be the reference; tests/test_gpu_cut_lists.py then compares every later kernel with them word for word.  Prints,
per case and form, how many lists are saturated (15 ranges), single-range, and (wave-cap form) changed by the cap.

usage: tools/record_cut_lists.py [output directory]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cut_list_cases as cc  # noqa: E402
from mesh_to_sdf_amd import Mesh, Topology, _lib, meshes  # noqa: E402


def grid_lists(name):
    """form -> words (and "two-level.coarse") of one grid case, from the library as it is loaded."""
    v, idx = cc.mesh_of(name)
    grid = cc.grid_of(name, v)
    out = {}
    with Mesh(v, Topology.TriangleList(idx)) as m:
        for form in cc.FORMS:
            knobs, kw = cc.form_call(name, form)
            with _lib.knobs(**knobs):
                out[form] = m.debug_cut_lists(grid, **kw)
                if form == "two-level":
                    out[form + ".coarse"] = m.debug_cut_lists(grid, coarse=True, **kw)
    return out


def query_lists():
    v, idx = meshes.named("blob-6k")
    out = {}
    with Mesh(v, Topology.TriangleList(idx)) as m, _lib.knobs(**cc.QUERY_KNOBS):
        for name, q in cc.query_sets().items():
            out[name] = m.debug_cut_lists(queries=q)
    return out


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else cc.GOLDEN
    os.makedirs(dst, exist_ok=True)
    for name in cc.GRID_CASES:
        got = grid_lists(name)
        np.savez_compressed(os.path.join(dst, name + ".npz"), **got)
        for form in cc.FORMS:
            w = got[form].reshape(-1, cc.CUT_WORDS)
            capped = int((w != got["one-level"].reshape(-1, cc.CUT_WORDS)).any(1).sum()) if form == "wave-cap" else 0
            print(f"{name:18s} {form:12s} {len(w):6d} lists: {int((w[:, 0] == cc.CUT_MAX).sum()):5d} of 15 ranges, {int((w[:, 0] == 1).sum()):5d} of one"
                  + (f", {capped} differ from one-level" if form == "wave-cap" else "")
                  + (f", {got[form + '.coarse'].size} coarse words" if form == "two-level" else ""), flush=True)
    got = query_lists()
    np.savez_compressed(os.path.join(dst, "queries.npz"), **got)
    for name, w in got.items():
        w = w.reshape(-1, cc.CUT_WORDS)
        print(f"{name:18s} {len(w):6d} lists: {int((w[:, 0] == cc.CUT_MAX).sum()):5d} of 15 ranges, {int((w[:, 0] == 1).sum()):5d} of one", flush=True)


if __name__ == "__main__":
    main()
