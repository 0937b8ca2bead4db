#!/usr/bin/env python3
"""Cost of the winding-number calls (include/m2s.h m2s_grid_winding_numbers / m2s_winding_numbers), timed with the library's HIP events:
seed_ms = the moments (k_moments), distance_ms = the Barnes-Hut walk (w alone) or the unsigned distance pass + the walk (signed
distances), next to the Raycast generate call of the same grid — what the robust sign costs.  Also the exact all-pairs form
(algorithm = 1) at a size where it finishes.  Device-resident data, best of --reps calls after one warm-up.

usage: tools/exp_winding.py [--out profiles/winding.txt] [--grids 128,256,512] [--queries 10000000] [--betas 2,3] [--exact-grid 64]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mesh_to_sdf_amd import (AccelerationMethod, Grid, M2STimings, SignMethod, Topology, generate_grid_sdf, generate_grid_sdf_winding,  # noqa: E402
                             generate_sdf, grid_winding_numbers, meshes, winding_numbers)


def best(fn, reps):
    fn(None)
    runs = []
    for _ in range(reps):
        t = M2STimings()
        fn(t)
        runs.append((t.total_ms, t.accel_build_ms, t.seed_ms, t.distance_ms))
    return min(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/winding.txt")
    ap.add_argument("--grids", default="128,256,512")
    ap.add_argument("--queries", default="10000000")
    ap.add_argument("--betas", default="2,3")
    ap.add_argument("--exact-grid", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    v, idx = meshes.named("blob-100k")
    dv, di = torch.as_tensor(v, device="cuda"), torch.as_tensor(idx.astype(np.int64), device="cuda")
    topo = Topology.TriangleList(di)
    betas = [float(x) for x in a.betas.split(",") if x]
    lines = [f"# blob-100k ({idx.size // 3} triangles), {torch.cuda.get_device_name(0)}; ms, best of {a.reps} by total_ms",
             "# case | beta | w alone: total, build, moments (seed_ms), walk (distance_ms) | signed: total, distance pass + walk (distance_ms)"
             " | generate (Raycast / RtreeBvh): total, distance_ms"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")

    lo, hi = meshes.extended_bbox(v, 0.1)
    for n in [int(x) for x in a.grids.split(",") if x]:
        g = Grid.from_bounding_box(lo, hi, [n, n, n])
        out = torch.empty(n ** 3, dtype=torch.float32, device="cuda")
        gen = best(lambda t: generate_grid_sdf(dv, topo, g, SignMethod.Raycast, timings=t, out=out), a.reps)
        for beta in betas:
            w = best(lambda t: grid_winding_numbers(dv, topo, g, beta=beta, timings=t, out=out), a.reps)
            s = best(lambda t: generate_grid_sdf_winding(dv, topo, g, beta=beta, timings=t, out=out), a.reps)
            emit(f"grid {n}^3 | {beta:g} | {w[0]:.3f}, {w[1]:.3f}, {w[2]:.3f}, {w[3]:.3f} | {s[0]:.3f}, {s[3]:.3f} | {gen[0]:.3f}, {gen[3]:.3f}")
        del out
    for nq in [int(x) for x in a.queries.split(",") if x]:
        lo2, hi2 = meshes.extended_bbox(v, 0.2)
        q = torch.as_tensor(meshes.uniform_queries(lo2, hi2, nq), device="cuda")
        gen = best(lambda t: generate_sdf(dv, topo, q, AccelerationMethod.RtreeBvh, timings=t), a.reps)
        for beta in betas:
            w = best(lambda t: winding_numbers(dv, topo, q, beta=beta, timings=t), a.reps)
            emit(f"queries {nq} | {beta:g} | {w[0]:.3f}, {w[1]:.3f}, {w[2]:.3f}, {w[3]:.3f} | - | {gen[0]:.3f}, {gen[3]:.3f}")
    if a.exact_grid:
        n = a.exact_grid
        g = Grid.from_bounding_box(lo, hi, [n, n, n])
        e = best(lambda t: grid_winding_numbers(dv, topo, g, algorithm=1, timings=t), 1)
        i = best(lambda t: grid_winding_numbers(dv, topo, g, beta=float("inf"), timings=t), 1)
        emit(f"exact, grid {n}^3 ({n ** 3 * (idx.size // 3) / 1e9:.1f} G solid angles) | all pairs (algorithm 1): walk {e[3]:.3f} | beta = inf through the tree: walk {i[3]:.3f}")


if __name__ == "__main__":
    main()
