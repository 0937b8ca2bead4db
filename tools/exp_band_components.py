#!/usr/bin/env python3
"""Cost of labelling and selecting the connected components of a narrow band (include/m2s.h m2s_band_components / m2s_band_select) on
device-resident data, on the workload of tools/exp_band_csg.py and tools/exp_band_filter.py plus debris: blob-100k and a copy translated
by a quarter of its extent (Raycast), bands three cells wide with the sign mask of voxelize(solid), their union, united with the band of
one small debris blob (a twentieth of the size, clear of the others), at 256^3, 512^3 and 2048^3 (--grids).
  - components: the whole call (m2s_timings.total_ms: init, hook, flatten, scan, number, label with the statistics) for connectivity 6,
    18 and 26, with the count and the first components' cells;
  - select: keep_largest(1)'s m2s_band_select alone (m2s_timings.total_ms: the mask walk with the row search, the scan, the compaction),
    with what it dropped and cleared, and keeping everything (no cell dropped: the row search still runs);
  - the peak of device memory during the calls above what was resident before them (hipMemGetInfo polled by a thread: a lower bound; for
    select it includes the result).
All times best of --reps after one warm-up of the very call.

usage: tools/exp_band_components.py [--out profiles/band_components.txt] [--grids 256,512,2048] [--reps 5]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from exp_band_redistance import PeakMemory  # noqa: E402
from mesh_to_sdf_amd import Grid, M2STimings, Mesh, SignMethod, Topology, meshes  # noqa: E402


def best_of(reps, call):
    """call(timings) -> result, run reps + 1 times; -> (the best m2s_timings by total_ms, the last result)."""
    best, res = None, None
    for r in range(reps + 1):
        t = M2STimings()
        res = call(t)
        if r and (best is None or t.total_ms < best.total_ms):
            best = t
    return best, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--grids", default="256,512,2048")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--note", default="")
    a = ap.parse_args()
    v, idx = meshes.named("blob-100k")
    ext = v.max(0) - v.min(0)
    v2 = (v + np.array([0.25 * float(ext[0]), 0.0, 0.0], np.float32)).astype(np.float32)
    centre = 0.5 * (v.max(0) + v.min(0))
    v3 = ((v - centre) * 0.05 + centre + np.array([0.0, 0.0, 0.62 * float(ext[2])], np.float32)).astype(np.float32)   # the debris, above the blobs
    lo, hi = meshes.extended_bbox(np.concatenate([v, v2, v3]), 0.1)
    ti = Topology.TriangleList(torch.as_tensor(idx.astype(np.int64), device="cuda:0"))
    lines = [f"# blob-100k ({idx.size // 3} triangles), a copy moved by a quarter of its extent along x and a debris copy a twentieth of the size, "
             f"{torch.cuda.get_device_name(0)}; Raycast, bands of 3 cells either side, sign masks from voxelize(solid), the union of all three; "
             f"device memory; times are m2s_timings.total_ms, best of {a.reps} after one warm-up" + (f"; {a.note}" if a.note else "")]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    with Mesh(torch.as_tensor(v, device="cuda:0"), ti) as ma, Mesh(torch.as_tensor(v2, device="cuda:0"), ti) as mb, \
            Mesh(torch.as_tensor(v3, device="cuda:0"), ti) as md:
        for n in [int(x) for x in a.grids.split(",")]:
            grid = Grid.from_bounding_box(lo, hi, [n, n, n])
            w = 3.0 * float(max(grid.get_cell_size()))
            with ma.narrow_band_field(grid, w, SignMethod.Raycast, True, background=w) as fa, \
                    mb.narrow_band_field(grid, w, SignMethod.Raycast, True, background=w) as fb, \
                    md.narrow_band_field(grid, w, SignMethod.Raycast, True, background=w) as fd, fa | fb as fab, fab | fd as fu:
                say(f"grid {n}^3: the union has {fu.count} cells ({fu.count / n ** 3:.2%} of the grid), the debris {fd.count}; its handle "
                    f"{fu.device_bytes / 2**20:.1f} MiB (a dense grid: {4 * n ** 3 / 2**20:.0f} MiB)")
                comps = None
                for conn in (6, 18, 26):
                    with PeakMemory() as mem:
                        t, cc = best_of(a.reps, lambda tm: fu.components(conn, timings=tm))
                    say(f"grid {n}^3 components, connectivity {conn}: {cc.count} components, cells {cc.n_cells.tolist()[:8]}, negative "
                        f"{cc.n_negative.tolist()[:8]} | total {t.total_ms:.3f} ms, {t.total_ms * 1e6 / max(fu.count, 1):.2f} ns per cell | peak device "
                        f"memory during the call {(mem.peak - mem.base) / 2**20:.0f} MiB above the resident handles")
                    comps = comps or cc
                # select: the largest component only, then everything
                for what, keep in (("keep the largest", comps.largest(1)), ("keep all", np.arange(comps.count))):
                    def run(tm, keep=keep):
                        with fu.select(comps, keep, timings=tm) as r:
                            return r.select_info
                    with PeakMemory() as mem:
                        t, info = best_of(a.reps, run)
                    say(f"grid {n}^3 select, {what}: {info.n_cells} cells kept, {info.n_dropped} dropped, {info.n_sign_cleared} inside bits cleared | "
                        f"total {t.total_ms:.3f} ms | peak device memory during the call {(mem.peak - mem.base) / 2**20:.0f} MiB above the resident handles")
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
