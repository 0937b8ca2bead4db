#!/usr/bin/env python3
"""Cost of moving a narrow band (include/m2s.h m2s_band_advect) on device-resident data, on the workload of tools/exp_band_filter.py:
blob-100k and a copy translated by a quarter of its extent (Raycast), bands three cells wide with the sign mask of voxelize(solid),
their union, at 256^3, 512^3 and 2048^3 (--grids).  The union takes --steps steps by a velocity that turns about the z axis and by a
normal speed that varies over the surface, both device tensors evaluated on `centers()`; dt gives a CFL number of 0.5.  Beside them,
in the same process and on the same field, --steps iterations of the Laplacian filter, alternating with the advect calls: a velocity
step reads the same six neighbours as a Laplacian pass plus 13 bytes a cell (the velocity and the moving byte for the region byte),
so that pass is the yardstick.
  - table: m2s_timings.seed_ms (per cell its 6 neighbour places, its value, and for advect the moving byte, n_moving and max_cfl);
  - steps: m2s_timings.distance_ms over the launches (distance_launches), and beside it the bytes one step must move — per cell its
    slots (24 bytes), its byte, its value in and out, and its field entry (12 or 4 bytes); the neighbour values are taken to come from
    the cache — with the time those bytes take at the HBM rate --hbm (TB/s; 6.29 is the measured copy rate of the MI355X);
  - one round of the tracker, `flow` over the time in which the fastest cell moves one cell edge (advect, then redistance), as the host
    clock sees it around a synchronise;
  - the peak of device memory during the call above what was resident before it (hipMemGetInfo polled by a thread: a lower bound).
All kernel times best of --reps after one warm-up of the very call.

usage: tools/exp_band_advect.py [--out profiles/band_advect.txt] [--grids 256,512,2048] [--steps 32] [--reps 5] [--hbm 6.29]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from exp_band_redistance import PeakMemory  # noqa: E402
from mesh_to_sdf_amd import AdvectKind, FilterKind, Grid, M2STimings, Mesh, SignMethod, Topology, flow_round, meshes  # noqa: E402

# per cell and step: the six slots, the byte, the value in and out, the field entry
STEP_BYTES = {"velocity": 6 * 4 + 1 + 8 + 12, "speed": 6 * 4 + 1 + 8 + 4, "laplacian": 6 * 4 + 1 + 8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--grids", default="256,512,2048")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hbm", type=float, default=6.29)
    ap.add_argument("--note", default="")
    a = ap.parse_args()
    v, idx = meshes.named("blob-100k")
    v2 = (v + np.array([0.25 * float(v[:, 0].max() - v[:, 0].min()), 0.0, 0.0], np.float32)).astype(np.float32)
    lo, hi = meshes.extended_bbox(np.concatenate([v, v2]), 0.1)
    ti = Topology.TriangleList(torch.as_tensor(idx.astype(np.int64), device="cuda:0"))
    lines = [f"# blob-100k ({idx.size // 3} triangles) and a copy moved by a quarter of its extent along x, {torch.cuda.get_device_name(0)}; Raycast, "
             f"bands of 3 cells either side, sign masks from voxelize(solid), their union moved {a.steps} steps at a CFL number of 0.5 and "
             f"filtered {a.steps} Laplacian iterations, the calls alternating; device memory; kernel times from m2s_timings; best of {a.reps} "
             f"after one warm-up; 'floor' = the bytes a step must move at {a.hbm} TB/s" + (f"; {a.note}" if a.note else "")]

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
                c = fu.centers()
                mid = c.mean(0)
                velocity = torch.stack([-(c[:, 1] - mid[1]), c[:, 0] - mid[0], torch.zeros_like(c[:, 0])], 1).contiguous()
                speed = (0.5 + 0.5 * torch.sin(4.0 * c[:, 2])).contiguous()
                del c
                fields = {"velocity": velocity, "speed": speed}
                dts = {name: flow_round(f, AdvectKind.Velocity if name == "velocity" else AdvectKind.Normal, grid.get_cell_size(), 1e30, 0.5, 1e30)[1]
                       for name, f in fields.items()}
                best, infos = {}, {}
                with PeakMemory() as mem:
                    for r in range(a.reps + 1):
                        for name in ("velocity", "laplacian", "speed"):
                            t = M2STimings()
                            if name == "laplacian":
                                with fu.filter(FilterKind.Laplacian, a.steps, timings=t) as fr:
                                    infos[name] = fr.filter_info
                            else:
                                with fu.advect(dts[name], a.steps, timings=t, **{name: fields[name]}) as fr:
                                    infos[name] = fr.advect_info
                            if r and (name not in best or t.distance_ms < best[name].distance_ms):
                                best[name] = t
                for name in ("velocity", "speed", "laplacian"):
                    t, info = best[name], infos[name]
                    run = max(1, t.distance_launches)
                    moved = STEP_BYTES[name] * fu.count
                    floor = moved / (a.hbm * 1e9)
                    what = (f"max_cfl {info.max_cfl:.3f}, {info.n_moving} cells moving, " if name != "laplacian" else "")
                    say(f"grid {n}^3 {name}: {run} steps, {what}{info.n_changed} cells changed, {info.n_sign_flips} signs, max change "
                        f"{info.max_change / w * 3:.3f} cells, n_nonfinite {info.n_nonfinite} | table {t.seed_ms:.3f} ms | steps {t.distance_ms:.3f} ms, "
                        f"{t.distance_ms / run:.4f} ms per step; a step must move {moved / 2**20:.1f} MiB, floor {floor:.4f} ms, "
                        f"{t.distance_ms / run / floor:.2f} x the floor | total {t.total_ms:.3f} ms")
                lap = best["laplacian"].distance_ms / max(1, best["laplacian"].distance_launches)
                say(f"grid {n}^3: a velocity step takes {best['velocity'].distance_ms / max(1, best['velocity'].distance_launches) / lap:.2f} x, a speed "
                    f"step {best['speed'].distance_ms / max(1, best['speed'].distance_launches) / lap:.2f} x a Laplacian pass; peak device memory "
                    f"during the calls {(mem.peak - mem.base) / 2**20:.0f} MiB above the resident handles")
                # one round of the tracker: the fastest cell moves one smallest cell edge, then the band is re-grown
                took = flow_round(velocity, AdvectKind.Velocity, grid.get_cell_size(), 1e30, 0.5, 1.0)[2]
                walls = []
                for r in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    with fu.flow(took, w, velocity=velocity) as fr:
                        torch.cuda.synchronize()
                        walls.append(time.perf_counter() - t0)
                        fi, ri, cells = fr.flow_info, fr.redistance_info, fr.count
                say(f"grid {n}^3 flow, one round by the velocity: {fi.steps} steps then redistance ({ri.sweeps} sweeps, n_open {ri.n_open}), {cells} cells, "
                    f"{min(walls[1:]) * 1e3:.2f} ms wall (best of 2 after one warm-up)")
                del velocity, speed, fields
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
