#!/usr/bin/env python3
"""Cost of the closest-point calls (include/m2s.h m2s_grid_closest_points / m2s_closest_points), both passes timed with the library's HIP
events: seed_ms = the first pass (the unsigned distance walk of the generate call), distance_ms - seed_ms = the second (k_closest), next to
the Raycast / RtreeBvh generate call of the same shape.  Device-resident data, best of five calls after one warm-up.

usage: tools/exp_closest.py [--out profiles/closest_passes.txt] [--grids 128,256,512] [--queries 1000000,10000000]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mesh_to_sdf_amd import (AccelerationMethod, Grid, M2STimings, SignMethod, Topology, closest_points, generate_grid_sdf,  # noqa: E402
                             generate_sdf, grid_closest_points, meshes)


def best(fn, reps=5):
    fn(None)
    runs = []
    for _ in range(reps):
        t = M2STimings()
        fn(t)
        runs.append((t.total_ms, t.seed_ms, t.distance_ms))
    return min(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/closest_passes.txt")
    ap.add_argument("--grids", default="128,256,512")
    ap.add_argument("--queries", default="1000000,10000000")
    a = ap.parse_args()
    v, idx = meshes.named("blob-100k")
    dv, di = torch.as_tensor(v, device="cuda"), torch.as_tensor(idx.astype(np.int64), device="cuda")
    topo = Topology.TriangleList(di)
    lines = [f"# blob-100k ({idx.size // 3} triangles), {torch.cuda.get_device_name(0)}; ms, best of 5 by total_ms",
             "# case | closest: total, first pass (seed_ms), second pass k_closest (distance_ms - seed_ms) | generate: total, distance_ms"]
    for n in [int(x) for x in a.grids.split(",") if x]:
        lo, hi = meshes.extended_bbox(v, 0.1)
        g = Grid.from_bounding_box(lo, hi, [n, n, n])
        out = tuple(torch.empty(s, dtype=dt, device="cuda") for s, dt in [(n ** 3, torch.int32), ((n ** 3, 3), torch.float32), (n ** 3, torch.float32)])
        c = best(lambda t: grid_closest_points(dv, topo, g, timings=t, out=out))
        gen = best(lambda t: generate_grid_sdf(dv, topo, g, SignMethod.Raycast, timings=t))
        lines.append(f"grid {n}^3 | {c[0]:.3f}, {c[1]:.3f}, {c[2] - c[1]:.3f} | {gen[0]:.3f}, {gen[2]:.3f}")
        print(lines[-1], flush=True)
        del out
    for nq in [int(x) for x in a.queries.split(",") if x]:
        lo, hi = meshes.extended_bbox(v, 0.2)
        q = torch.as_tensor(meshes.uniform_queries(lo, hi, nq), device="cuda")
        c = best(lambda t: closest_points(dv, topo, q, timings=t))
        gen = best(lambda t: generate_sdf(dv, topo, q, AccelerationMethod.RtreeBvh, timings=t))
        lines.append(f"queries {nq} | {c[0]:.3f}, {c[1]:.3f}, {c[2] - c[1]:.3f} | {gen[0]:.3f}, {gen[2]:.3f}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
