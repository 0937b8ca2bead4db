#!/usr/bin/env python3
"""Cost of ray casting against the mesh (include/m2s.h m2s_mesh_cast_rays) on device-resident data: the kernel time of the library's HIP
events (m2s_timings.distance_ms), best of five calls after one warm-up, on blob-100k:
  - 1920 x 1080 pinhole camera rays (the camera of tools/exp_grid_query.py) in scanline order and in 8 x 8 pixel tiles;
  - random rays in 1.8 x the mesh's box;
  - each for the three things a call can ask for: every output (the count needs every hit, so nothing is pruned against the best t),
    the first hit alone (pruned), occlusion alone (stops at the first hit met);
  - the random rays once more after the caller sorted them by direction octant and origin cell (16^3 cells of the box, x-major), with
    the cost of that sort beside it: what ray sorting inside the library could gain at best.

usage: tools/exp_rays.py [--out profiles/rays.txt] [--random 10000000]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from exp_grid_query import best, camera_rays  # noqa: E402
from mesh_to_sdf_amd import Mesh, Topology, meshes  # noqa: E402


def sort_rays(o, d, lo, hi):
    """Rays ordered by direction octant, then by the origin's cell in a 16^3 grid over [lo, hi]; and what the ordering costs (ms)."""
    def order():
        cell = ((o - lo) / (hi - lo) * 16).clamp_(0, 15).long()
        octant = ((d > 0).long() * torch.tensor([1, 2, 4], device=d.device)).sum(1)
        perm = torch.argsort((octant << 12) | (cell[:, 0] << 8) | (cell[:, 1] << 4) | cell[:, 2])
        return o[perm].contiguous(), d[perm].contiguous()
    order()
    ms = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = order()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return out[0], out[1], min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/rays.txt")
    ap.add_argument("--random", type=int, default=10_000_000)
    a = ap.parse_args()
    v, idx = meshes.named("blob-100k")
    dv, di = torch.as_tensor(v, device="cuda"), torch.as_tensor(idx.astype(np.int64), device="cuda")
    lo, hi = meshes.extended_bbox(v, 0.1)
    rng = np.random.default_rng(1)
    mid, half = (v.max(0) + v.min(0)) / 2, (v.max(0) - v.min(0)) / 2
    sets = [("camera 1920x1080 scanline", *camera_rays(lo, hi, tiles=False)), ("camera 1920x1080 8x8 tiles", *camera_rays(lo, hi, tiles=True)),
            (f"random {a.random}", (mid + 1.8 * half * rng.uniform(-1, 1, (a.random, 3))).astype(np.float32),
             rng.normal(size=(a.random, 3)).astype(np.float32))]
    lines = [f"# blob-100k ({idx.size // 3} triangles), {torch.cuda.get_device_name(0)}; kernel ms (m2s_timings.distance_ms), best of 5",
             "# walk: one ray per lane, stackless pre-order walk in storage order"]
    with Mesh(dv, Topology.TriangleList(di)) as m:
        for label, o_h, d_h in sets:
            o, d = torch.as_tensor(o_h, device="cuda"), torch.as_tensor(d_h, device="cuda")
            n = o.shape[0]
            hit = float(m.test_occlusions(o, d).float().mean())
            for what, fn in (("first hit (t, triangle, uv)", m.cast_rays), ("count", m.count_intersections), ("occluded only", m.test_occlusions)):
                ms = best(lambda t: fn(o, d, timings=t))
                lines.append(f"{label:<28} {what:<28} {ms:9.3f} ms  {n / ms / 1e3:9.1f} Mrays/s  (hit rate {hit:.3f})")
                print(lines[-1], flush=True)
            if label.startswith("random"):
                t_lo, t_hi = (torch.as_tensor(x, device="cuda") for x in ((mid - 1.8 * half).astype(np.float32), (mid + 1.8 * half).astype(np.float32)))
                o, d, sort_ms = sort_rays(o, d, t_lo, t_hi)
                for what, fn in (("first hit (t, triangle, uv)", m.cast_rays), ("count", m.count_intersections), ("occluded only", m.test_occlusions)):
                    ms = best(lambda t: fn(o, d, timings=t))
                    lines.append(f"{label + ' sorted':<28} {what:<28} {ms:9.3f} ms  {n / ms / 1e3:9.1f} Mrays/s  (+ {sort_ms:.3f} ms to sort and gather)")
                    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
