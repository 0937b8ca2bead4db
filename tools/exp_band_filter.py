#!/usr/bin/env python3
"""Cost of filtering a narrow band (include/m2s.h m2s_band_filter) on device-resident data, on the workload of tools/exp_band_csg.py and
tools/exp_band_redistance.py: blob-100k and a copy translated by a quarter of its extent (Raycast), bands three cells wide with the sign
mask of voxelize(solid), their union, at 256^3, 512^3 and 2048^3 (--grids).  The union is filtered everywhere, --iterations iterations
of each kind.
  - table: m2s_timings.seed_ms (per cell its 6 or 18 neighbour places, its region byte and its value);
  - passes: m2s_timings.distance_ms, the number of passes (distance_launches), ms per pass, and beside it the bytes one pass must move —
    per cell its slots (24 bytes; for the mean the two of the pass's axis, 8 bytes), its region byte and its value in and out; the
    neighbour values are taken to come from the cache — with the time those bytes take at the HBM rate --hbm (TB/s; 6.29 is the
    measured copy rate of the MI355X);
  - the total, and the peak of device memory during the call above what was resident before it (torch cannot see the library's
    allocations, so the peak is taken from hipMemGetInfo polled by a thread: a lower bound; it includes the result).
All times best of --reps after one warm-up of the very call.

usage: tools/exp_band_filter.py [--out profiles/band_filter.txt] [--grids 256,512,2048] [--iterations 8] [--reps 5] [--hbm 6.29]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from exp_band_redistance import PeakMemory  # noqa: E402
from mesh_to_sdf_amd import FilterKind, Grid, M2STimings, Mesh, SignMethod, Topology, meshes  # noqa: E402

# per cell and pass: the slots the pass reads, the region byte, the value in and out
PASS_BYTES = {FilterKind.Mean: 2 * 4 + 1 + 8, FilterKind.Laplacian: 6 * 4 + 1 + 8, FilterKind.MeanCurvature: 18 * 4 + 1 + 8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--grids", default="256,512,2048")
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hbm", type=float, default=6.29)
    ap.add_argument("--note", default="")
    a = ap.parse_args()
    v, idx = meshes.named("blob-100k")
    v2 = (v + np.array([0.25 * float(v[:, 0].max() - v[:, 0].min()), 0.0, 0.0], np.float32)).astype(np.float32)
    lo, hi = meshes.extended_bbox(np.concatenate([v, v2]), 0.1)
    ti = Topology.TriangleList(torch.as_tensor(idx.astype(np.int64), device="cuda:0"))
    lines = [f"# blob-100k ({idx.size // 3} triangles) and a copy moved by a quarter of its extent along x, {torch.cuda.get_device_name(0)}; Raycast, "
             f"bands of 3 cells either side, sign masks from voxelize(solid), their union filtered everywhere, {a.iterations} iterations; device "
             f"memory; kernel times from m2s_timings; best of {a.reps} after one warm-up; 'floor' = the bytes a pass must move at {a.hbm} TB/s"
             + (f"; {a.note}" if a.note else "")]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    with Mesh(torch.as_tensor(v, device="cuda:0"), ti) as ma, Mesh(torch.as_tensor(v2, device="cuda:0"), ti) as mb:
        for n in [int(x) for x in a.grids.split(",")]:
            grid = Grid.from_bounding_box(lo, hi, [n, n, n])
            w = 3.0 * float(max(grid.get_cell_size()))
            with ma.narrow_band_field(grid, w, SignMethod.Raycast, True, background=w) as fa, \
                    mb.narrow_band_field(grid, w, SignMethod.Raycast, True, background=w) as fb, fa | fb as fu:
                say(f"grid {n}^3: the union has {fu.count} cells ({fu.count / n ** 3:.2%} of the grid); its handle {fu.device_bytes / 2**20:.1f} MiB "
                    f"(a dense grid: {4 * n ** 3 / 2**20:.0f} MiB)")
                for kind in (FilterKind.Mean, FilterKind.Laplacian, FilterKind.MeanCurvature):
                    best = None
                    with PeakMemory() as mem:
                        for r in range(a.reps + 1):
                            t = M2STimings()
                            with fu.filter(kind, a.iterations, timings=t) as fr:
                                info = fr.filter_info
                            if r and (best is None or t.total_ms < best.total_ms):
                                best = t
                    run = max(1, best.distance_launches)
                    moved = PASS_BYTES[kind] * fu.count
                    floor = moved / (a.hbm * 1e9)
                    say(f"grid {n}^3 {kind.name}: {info.passes} passes, {info.n_changed} cells changed, {info.n_sign_flips} signs, max change "
                        f"{info.max_change / w * 3:.3f} cells, n_nonfinite {info.n_nonfinite} | table {best.seed_ms:.3f} ms | passes "
                        f"{best.distance_ms:.3f} ms, {best.distance_ms / run:.3f} ms per pass; a pass must move {moved / 2**20:.1f} MiB, floor "
                        f"{floor:.3f} ms, {best.distance_ms / run / floor:.2f} x the floor | total {best.total_ms:.3f} ms | peak device memory "
                        f"during the call {(mem.peak - mem.base) / 2**20:.0f} MiB above the resident handles")
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
