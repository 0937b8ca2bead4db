#!/usr/bin/env python3
"""Cost of resampling a narrow band onto another grid (include/m2s.h m2s_band_resample) on device-resident data: blob-100k, Raycast, a
band three cells wide with the sign mask of voxelize(solid).  Rows (--rows):
  turn    the solid turned by 0.7 rad about (1, 2, 3), scaled by 0.75 about the box centre, TRILINEAR, n^3 -> n^3 at 256 and 512;
  refine  the identity, TRILINEAR, 512^3 -> 1024^3 on the same box;
  shift   a shift by (2, -1, 3) whole cells, SNAP, 2048^3 -> 2048^3: the capacity case.
Per row:
  - mask: m2s_timings.seed_ms (the per-point pass over the target and the scan); values: distance_ms; the call's total_ms;
  - the floor: the bytes the call must move — the target's three index arrays out, the source's index words and band values in, the
    result's values out — at the HBM rate --hbm (TB/s; 6.29 is the measured copy rate of the MI355X);
  - the peak of device memory during the call above what was resident before it (hipMemGetInfo polled by a thread: a lower bound; it
    includes the result);
  - at 256^3 and 512^3, the only route without the call, timed by events around it: BandField.sample with support at every target centre
    (12 bytes in and 5 out per point), a torch compaction of the points with full support and a finite value, BandField(...).  That route
    builds no sign mask, which would take a second, SNAP sample of every point.
All times best of --reps after one warm-up of the very call.

usage: tools/exp_band_resample.py [--out profiles/band_resample.txt] [--rows turn256,turn512,refine,shift] [--reps 5] [--hbm 6.29]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from exp_band_redistance import PeakMemory  # noqa: E402
from mesh_to_sdf_amd import BandField, Grid, M2STimings, Mesh, SampleMode, SignMethod, Topology, meshes  # noqa: E402


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def centres(grid):
    """The target's cell centres on the device, float32[total, 3] in the order of L: first + (float)idx * size."""
    f, s, n = grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count()
    ax = [torch.as_tensor(np.float32(f[a]), device="cuda:0") + torch.arange(n[a], dtype=torch.float32, device="cuda:0") * float(s[a]) for a in range(3)]
    return torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def old_route(field, grid, to_source, scale, mode, K):
    """sample at every target centre, a torch compaction, BandField(...) -> (ms, cells)."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    p = centres(grid)
    m = torch.as_tensor(np.asarray(to_source, np.float32).reshape(3, 4), device="cuda:0")
    q = (p @ m[:, :3].T + m[:, 3]).contiguous()
    v, sup = field.sample(q, mode=mode, outside=field.background[1], support=True)
    r = v * float(scale)
    keep = (sup == K) & torch.isfinite(r)
    cells = torch.nonzero(keep).reshape(-1)
    out = BandField(grid, cells, r[cells].contiguous(), background=tuple(float(b) * float(scale) for b in field.background))
    stop.record()
    torch.cuda.synchronize()
    n = out.count
    out.close()
    return start.elapsed_time(stop), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="turn256,turn512,refine,shift")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hbm", type=float, default=6.29)
    ap.add_argument("--note", default="")
    a = ap.parse_args()
    v, idx = meshes.named("blob-100k")
    lo, hi = meshes.extended_bbox(v, 0.1)
    ti = Topology.TriangleList(torch.as_tensor(idx.astype(np.int64), device="cuda:0"))
    lines = [f"# blob-100k ({idx.size // 3} triangles), {torch.cuda.get_device_name(0)}; Raycast, a band of 3 cells either side, sign mask from "
             f"voxelize(solid); device memory; kernel times from m2s_timings; best of {a.reps} after one warm-up; 'floor' = the bytes the call must "
             f"move at {a.hbm} TB/s; 'old route' = sample at every target centre + torch compaction + BandField(...), by events"
             + (f"; {a.note}" if a.note else "")]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    centre = (np.asarray(lo, np.float64) + np.asarray(hi, np.float64)) / 2
    A = 0.75 * rotation((1, 2, 3), 0.7)
    turn = np.concatenate([A, (centre - A @ centre)[:, None]], 1)
    plans = {"turn256": (256, 256, "turn", SampleMode.Trilinear, True), "turn512": (512, 512, "turn", SampleMode.Trilinear, True),
             "refine": (512, 1024, "identity", SampleMode.Trilinear, False), "shift": (2048, 2048, "shift", SampleMode.Snap, False)}
    with Mesh(torch.as_tensor(v, device="cuda:0"), ti) as mesh:
        for row in a.rows.split(","):
            ns, nt, what, mode, compare = plans[row]
            src = Grid.from_bounding_box(lo, hi, [ns, ns, ns])
            w = 3.0 * float(max(src.get_cell_size()))
            if what == "shift":
                f, s = src.get_first_cell(), src.get_cell_size()
                tgt = Grid([float(f[k]) + (2, -1, 3)[k] * float(s[k]) for k in range(3)], list(s), [nt, nt, nt])
            else:
                tgt = Grid.from_bounding_box(lo, hi, [nt, nt, nt])
            fwd = turn if what == "turn" else None
            with mesh.narrow_band_field(src, w, SignMethod.Raycast, True, background=w) as fs:
                best = None
                with PeakMemory() as mem:
                    for r in range(a.reps + 1):
                        t = M2STimings()
                        with fs.resample(tgt, fwd, mode=mode, timings=t) as fr:
                            info, count, rbytes = fr.resample_info, fr.count, fr.device_bytes
                        if r and (best is None or t.total_ms < best.total_ms):
                            best = t
                words_t = (nt ** 3 + 63) // 64
                moved = 24 * words_t + fs.device_bytes + 4 * count
                floor = moved / (a.hbm * 1e9)
                line = (f"{row}: {ns}^3 -> {nt}^3 {what} {mode.name}: source {fs.count} cells ({fs.device_bytes / 2**20:.1f} MiB), result {count} cells "
                        f"({rbytes / 2**20:.1f} MiB; a dense grid: {4 * nt ** 3 / 2**20:.0f} MiB), {info} | mask {best.seed_ms:.3f} ms "
                        f"({nt ** 3 / best.seed_ms / 1e6:.1f} G points/s) | values {best.distance_ms:.3f} ms | total {best.total_ms:.3f} ms | must move "
                        f"{moved / 2**20:.1f} MiB, floor {floor:.3f} ms, {best.total_ms / floor:.1f} x the floor | peak device memory during the call "
                        f"{(mem.peak - mem.base) / 2**20:.0f} MiB above the resident source")
                if compare:
                    from mesh_to_sdf_amd.api import _similarity
                    to_source, scale = _similarity(fwd)
                    old = None
                    for r in range(a.reps + 1):
                        ms, n_old = old_route(fs, tgt, to_source, scale, mode, 8)
                        if r and (old is None or ms < old):
                            old = ms
                    line += f" | old route {old:.3f} ms ({n_old} cells, no sign mask), {old / best.total_ms:.1f} x the call"
                say(line)
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
