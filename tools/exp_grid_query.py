#!/usr/bin/env python3
"""Cost of the grid queries (include/m2s.h m2s_sample_grid / m2s_raymarch_grid) on device-resident data: the kernel time of the library's
HIP events (m2s_timings.distance_ms), best of five calls after one warm-up.
  - trilinear sampling of 10 M uniformly random points over the blob-100k grid at 256^3 (64 MiB: fits the Infinity Cache) and 512^3
    (512 MiB: does not), values alone and with normals, and the same points sorted by cell (what locality buys);
  - the exact query path, generate_sdf(RtreeBvh), on the same points;
  - 1920 x 1080 pinhole camera rays against the 256^3 grid in scanline order and in 8 x 8 pixel tiles: Mrays/s and mean steps.

usage: tools/exp_grid_query.py [--out profiles/grid_query.txt] [--grids 256,512] [--points 10000000]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mesh_to_sdf_amd import (AccelerationMethod, Grid, M2STimings, SampleMode, SignMethod, Topology, generate_grid_sdf,  # noqa: E402
                             generate_sdf, meshes, raymarch_grid, sample_grid)


def best(fn, reps=5):
    fn(None)
    runs = []
    for _ in range(reps):
        t = M2STimings()
        fn(t)
        runs.append(t.distance_ms)
    return min(runs)


def camera_rays(lo, hi, w=1920, h=1080, tiles=False):
    c, ext = (lo + hi) / 2, float((hi - lo).max())
    eye = c + np.array([0.3, 0.4, -1.6]) * ext
    fwd = (c - eye) / np.linalg.norm(c - eye)
    right = np.cross(fwd, [0, 1, 0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    px, py = np.meshgrid(np.arange(w), np.arange(h))                 # scanline order: row after row
    if tiles:                                                        # 8 x 8 pixel tiles, tile after tile
        key = ((py // 8) * ((w + 7) // 8) + px // 8) * 64 + (py % 8) * 8 + px % 8
        order = np.argsort(key.reshape(-1), kind="stable")
        px, py = px.reshape(-1)[order], py.reshape(-1)[order]
    u = ((px.reshape(-1) + 0.5) / w * 2 - 1) * (w / h)
    v = 1 - (py.reshape(-1) + 0.5) / h * 2
    r = fwd + 0.35 * (u[:, None] * right + v[:, None] * up)
    r = (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(np.float32)
    return np.tile(eye.astype(np.float32), (r.shape[0], 1)), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/grid_query.txt")
    ap.add_argument("--grids", default="256,512")
    ap.add_argument("--points", type=int, default=10_000_000)
    a = ap.parse_args()
    v, idx = meshes.named("blob-100k")
    dv, di = torch.as_tensor(v, device="cuda"), torch.as_tensor(idx.astype(np.int64), device="cuda")
    topo = Topology.TriangleList(di)
    lo, hi = meshes.extended_bbox(v, 0.1)
    n_pts = a.points
    rng = np.random.default_rng(1)
    pts_h = rng.uniform(lo, hi, (n_pts, 3)).astype(np.float32)
    pts = torch.as_tensor(pts_h, device="cuda")
    lines = [f"# blob-100k ({idx.size // 3} triangles), {torch.cuda.get_device_name(0)}; kernel ms (m2s_timings.distance_ms), best of 5",
             f"# {n_pts} points uniform in the grid box"]
    exact = best(lambda t: generate_sdf(dv, topo, pts, AccelerationMethod.RtreeBvh, timings=t))
    lines.append(f"exact generate_sdf(RtreeBvh) distance_ms {exact:.3f}")
    print(lines[-1], flush=True)
    for n in [int(x) for x in a.grids.split(",") if x]:
        g = Grid.from_bounding_box(lo, hi, [n, n, n])
        d = generate_grid_sdf(dv, topo, g, SignMethod.Raycast)
        cs = g.get_cell_size()
        cell = np.floor((pts_h - g.get_first_cell()) / cs).astype(np.int64).clip(0, n - 1)
        sorted_pts = torch.as_tensor(pts_h[np.argsort((cell[:, 0] * n + cell[:, 1]) * n + cell[:, 2], kind="stable")], device="cuda")
        for mode in (SampleMode.Trilinear, SampleMode.Tetrahedral, SampleMode.Snap):
            for label, p in (("random", pts), ("sorted by cell", sorted_pts)):
                t_v = best(lambda t: sample_grid(g, d, p, mode=mode, timings=t))
                t_n = best(lambda t: sample_grid(g, d, p, mode=mode, normals=True, timings=t))
                lines.append(f"grid {n}^3 {mode.name:<11} {label:<14} values {t_v:.3f} ms ({n_pts / t_v / 1e6:.2f} Gpts/s)"
                             f" | values + normals {t_n:.3f} ms")
                print(lines[-1], flush=True)
        for tiles in (False, True):
            o_h, r_h = camera_rays(lo, hi, tiles=tiles)
            o, r = torch.as_tensor(o_h, device="cuda"), torch.as_tensor(r_h, device="cuda")
            for mode in (SampleMode.Trilinear, SampleMode.Tetrahedral):
                tr = best(lambda t: raymarch_grid(g, d, o, r, mode=mode, timings=t))
                tn = best(lambda t: raymarch_grid(g, d, o, r, mode=mode, normals=True, timings=t))
                _, _, steps, hit = raymarch_grid(g, d, o, r, mode=mode)
                st = steps.view(torch.int32) if steps.dtype != torch.int32 else steps
                lines.append(f"grid {n}^3 rays 1920x1080 {'8x8 tiles' if tiles else 'scanline '} {mode.name:<11} {tr:.3f} ms"
                             f" ({o.shape[0] / tr / 1e3:.0f} Mrays/s), with normals {tn:.3f} ms; mean steps {st.float().mean().item():.2f},"
                             f" max {st.max().item()}, hits {hit.float().mean().item():.3f}")
                print(lines[-1], flush=True)
        del d
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
