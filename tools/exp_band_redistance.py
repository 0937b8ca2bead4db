#!/usr/bin/env python3
"""Cost of redistancing a narrow band (include/m2s.h m2s_band_redistance) on device-resident data, on the workload of tools/exp_band_csg.py:
blob-100k and a copy translated by a quarter of its extent (Raycast), bands three cells wide with the sign mask of voxelize(solid), their
union, at 256^3, 512^3 and 2048^3 (--grids).  The union is redistanced to --widths cells (of the largest cell size) either side.
  - topology: m2s_timings.seed_ms (s, the frozen set, the two box dilations, the candidates' index, the start values);
  - sweeps: m2s_timings.distance_ms, the number of sweeps run (distance_launches: the flags are read every fourth sweep) and the number
    that changed a value, ms per sweep, and beside it the bytes one sweep must move — per candidate its six neighbour slots, its meta
    byte and its value in and out, 33 bytes; the six neighbour values are taken to come from the cache — with the time those bytes
    take at the HBM rate --hbm (TB/s; 6.29 is the measured copy rate of the MI355X);
  - the total, candidates / result cells, and the peak of device memory during the call above what was resident before it
    (torch cannot see the library's allocations, so the peak is taken from hipMemGetInfo polled by a thread: a lower bound);
  - beside them, as information only, the wall time of the exact route on the same machine: isosurface of the union -> Mesh ->
    narrow_band_field of the same widths, where it fits (--exact-max).
All times best of --reps after one warm-up of the very call.

usage: tools/exp_band_redistance.py [--out profiles/band_redistance.txt] [--grids 256,512,2048] [--widths 3,5] [--reps 5] [--hbm 6.29]"""
import argparse
import os
import sys
import threading
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mesh_to_sdf_amd import Grid, M2STimings, Mesh, SignMethod, Topology, meshes  # noqa: E402


class PeakMemory:
    """The largest device memory in use while the block runs, polled every millisecond."""

    def __enter__(self):
        self.base = self.used()
        self.peak = self.base
        self.stop = False
        self.thread = threading.Thread(target=self.poll)
        self.thread.start()
        return self

    @staticmethod
    def used():
        free, total = torch.cuda.mem_get_info()
        return total - free

    def poll(self):
        while not self.stop:
            self.peak = max(self.peak, self.used())
            time.sleep(0.001)

    def __exit__(self, *exc):
        self.stop = True
        self.thread.join()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--grids", default="256,512,2048")
    ap.add_argument("--widths", default="3,5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hbm", type=float, default=6.29)
    ap.add_argument("--exact-max", type=int, default=512, help="largest grid on which the exact route is timed")
    ap.add_argument("--note", default="")
    a = ap.parse_args()
    v, idx = meshes.named("blob-100k")
    v2 = (v + np.array([0.25 * float(v[:, 0].max() - v[:, 0].min()), 0.0, 0.0], np.float32)).astype(np.float32)
    lo, hi = meshes.extended_bbox(np.concatenate([v, v2]), 0.1)
    ti = Topology.TriangleList(torch.as_tensor(idx.astype(np.int64), device="cuda:0"))
    lines = [f"# blob-100k ({idx.size // 3} triangles) and a copy moved by a quarter of its extent along x, {torch.cuda.get_device_name(0)}; Raycast, "
             f"bands of 3 cells either side, sign masks from voxelize(solid), their union redistanced; device memory; kernel times from "
             f"m2s_timings, wall times with a device synchronisation either side; best of {a.reps} after one warm-up; 'floor' = the bytes a "
             f"sweep must move at {a.hbm} TB/s" + (f"; {a.note}" if a.note else "")]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    with Mesh(torch.as_tensor(v, device="cuda:0"), ti) as ma, Mesh(torch.as_tensor(v2, device="cuda:0"), ti) as mb:
        for n in [int(x) for x in a.grids.split(",")]:
            grid = Grid.from_bounding_box(lo, hi, [n, n, n])
            cell = float(max(grid.get_cell_size()))
            w = 3.0 * cell
            with ma.narrow_band_field(grid, w, SignMethod.Raycast, True, background=w) as fa, \
                    mb.narrow_band_field(grid, w, SignMethod.Raycast, True, background=w) as fb, fa | fb as fu:
                say(f"grid {n}^3: the union has {fu.count} cells ({fu.count / n ** 3:.2%} of the grid); its handle {fu.device_bytes / 2**20:.1f} MiB "
                    f"(a dense grid: {4 * n ** 3 / 2**20:.0f} MiB)")
                for cells in [float(x) for x in a.widths.split(",")]:
                    width = cells * cell
                    best = None
                    with PeakMemory() as mem:
                        for r in range(a.reps + 1):
                            t = M2STimings()
                            with fu.redistance(width, timings=t) as fr:
                                info, count = fr.redistance_info, fr.count
                            if r and (best is None or t.total_ms < best.total_ms):
                                best = t
                    run = max(1, best.distance_launches)
                    moved = 33 * info.n_candidates
                    floor = moved / (a.hbm * 1e9)
                    say(f"grid {n}^3 redistance to {cells:g} cells: {count} cells of {info.n_candidates} candidates ({info.n_candidates / max(count, 1):.2f} x), "
                        f"{info.n_frozen} frozen, n_open {info.n_open} | topology {best.seed_ms:.3f} ms | {run} sweeps run ({info.sweeps} changed a value, "
                        f"converged {int(info.converged)}) {best.distance_ms:.3f} ms, {best.distance_ms / run:.3f} ms per sweep; a sweep must move "
                        f"{moved / 2**20:.1f} MiB, floor {floor:.3f} ms, {best.distance_ms / run / floor:.2f} x the floor | total {best.total_ms:.3f} ms | "
                        f"peak device memory during the call {(mem.peak - mem.base) / 2**20:.0f} MiB above the resident handles")
                    if n <= a.exact_max:
                        def exact():
                            ev, ei, _ = fu.isosurface(0.0)
                            ei = ei if ei.dtype in (torch.int32, torch.int64) else ei.view(torch.int32)
                            with Mesh(ev, Topology.TriangleList(ei.reshape(-1).contiguous())) as mu, \
                                    mu.narrow_band_field(grid, width, SignMethod.Raycast, True, background=width) as fe:
                                return fe.count, ev.shape[0]
                        ms = 1e30
                        for r in range(a.reps + 1):
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            n_exact, n_vert = exact()
                            torch.cuda.synchronize()
                            if r:
                                ms = min(ms, (time.perf_counter() - t0) * 1e3)
                        say(f"grid {n}^3 the exact route to {cells:g} cells (isosurface -> Mesh of {n_vert} vertices -> narrow_band_field): {ms:.2f} ms wall, "
                            f"{n_exact} cells")
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
