#!/usr/bin/env python3
"""Cost of making a band field from spheres and capsules (include/m2s.h m2s_band_from_capsules) on device-resident shapes, on a grid of
--grid^3 cells over the unit cube, with a band of 3 cells either side:
  - spheres:    --spheres balls of radius 2.5 cells, centres uniform in the cube;
  - lattice:    the edges of a cubic lattice of 33^3 nodes (104 544 capsules of radius 2 cells);
  - one ball:   a single ball of radius 400 / 1024 of the cube (its rows are shared among the waves);
  - contention: the same --spheres balls with their centres jittered into a cube of 64 cells' side (hundreds of them on every cell);
  - the route without this call: --mesh-spheres of the balls as icospheres of 80 triangles merged into one mesh, Mesh.narrow_band_field
    (Raycast, sign mask from voxelize(solid)), beside from_spheres of the same balls.
Times are m2s_timings of the call (seed_ms = boxes, bit planes, mask and offsets; distance_ms = the values; total_ms) and the wall clock
of the Python call up to a device synchronisation; best of --reps after one warm-up of the very call.

usage: tools/exp_band_shapes.py [--out profiles/band_shapes.txt] [--grid 1024] [--spheres 1000000] [--mesh-spheres 100000] [--reps 3]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mesh_to_sdf_amd import BandField, Grid, M2STimings, Mesh, SignMethod, Topology  # noqa: E402

DEV = "cuda:0"


def icosphere():
    """An icosahedron subdivided once, on the unit sphere: 42 vertices, 80 triangles."""
    p = (1 + 5 ** 0.5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    mid, out = {}, []

    def m(a, b):
        key = (min(a, b), max(a, b))
        if key not in mid:
            x = v[a] + v[b]
            v.append(x / np.linalg.norm(x))
            mid[key] = len(v) - 1
        return mid[key]

    for a, b, c in f:
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    return np.asarray(v, np.float32), np.asarray(out, np.int64)


def timed(reps, make):
    """make(timings) -> BandField, run reps + 1 times -> (best m2s_timings by total_ms, best wall ms, count, shapes_info)."""
    best, wall, count, info = None, None, 0, None
    for r in range(reps + 1):
        t = M2STimings()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = make(t)
        torch.cuda.synchronize()
        w = (time.perf_counter() - t0) * 1e3
        count, info = f.count, getattr(f, "shapes_info", None)
        f.close()
        if r and (best is None or t.total_ms < best.total_ms):
            best = t
        if r and (wall is None or w < wall):
            wall = w
    return best, wall, count, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--spheres", type=int, default=1000000)
    ap.add_argument("--mesh-spheres", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--note", default="")
    a = ap.parse_args()
    n = a.grid
    h = 1.0 / n
    grid = Grid([0.5 * h] * 3, [h] * 3, [n] * 3)
    w = 3.0 * h
    rng = np.random.default_rng(1)
    lines = [f"# {n}^3 cells over the unit cube, bands of 3 cells either side, {torch.cuda.get_device_name(0)}; device memory; planes / values / total are "
             f"m2s_timings seed_ms / distance_ms / total_ms, wall is the Python call up to a synchronisation; best of {a.reps} after one warm-up"
             + (f"; {a.note}" if a.note else "")]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    def report(what, t, wall, count, info):
        say(f"{what}: {count} cells ({count / n ** 3:.2%} of the grid), n_inside {info.n_inside}, n_off_grid {info.n_off_grid} | planes {t.seed_ms:.3f} ms, "
            f"values {t.distance_ms:.3f} ms, total {t.total_ms:.3f} ms, wall {wall:.3f} ms")

    centres = torch.as_tensor(rng.uniform(0.02, 0.98, (a.spheres, 3)).astype(np.float32), device=DEV)
    report(f"{a.spheres} spheres of 2.5 cells", *timed(a.reps, lambda tm: BandField.from_spheres(grid, centres, 2.5 * h, w, timings=tm)))

    k = 33
    node = np.stack(np.meshgrid(*(np.linspace(0.03, 0.97, k),) * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    idx = np.arange(k ** 3).reshape(k, k, k)
    edges = np.concatenate([np.stack([idx[:-1].ravel(), idx[1:].ravel()], 1), np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], 1),
                            np.stack([idx[:, :, :-1].ravel(), idx[:, :, 1:].ravel()], 1)])
    tn, te = torch.as_tensor(node, device=DEV), torch.as_tensor(edges, device=DEV)
    ea, eb = tn[te[:, 0]].contiguous(), tn[te[:, 1]].contiguous()
    report(f"{edges.shape[0]} capsules of 2 cells (the edges of a lattice of {k}^3 nodes)",
           *timed(a.reps, lambda tm: BandField.from_capsules(grid, ea, eb, 2.0 * h, w, timings=tm)))

    one = torch.as_tensor(np.asarray([[0.5, 0.5, 0.5]], np.float32), device=DEV)
    report("one ball of 400 / 1024 of the cube", *timed(a.reps, lambda tm: BandField.from_spheres(grid, one, 400.0 / 1024.0, w, timings=tm)))

    packed = torch.as_tensor((0.5 + rng.uniform(-32, 32, (a.spheres, 3)) * h).astype(np.float32), device=DEV)
    report(f"{a.spheres} spheres of 2.5 cells jittered into 64^3 cells", *timed(a.reps, lambda tm: BandField.from_spheres(grid, packed, 2.5 * h, w, timings=tm)))

    # the route without this call: icospheres merged into one mesh
    m = a.mesh_spheres
    if m:
        sub = centres[:m].contiguous()
        report(f"{m} spheres of 2.5 cells", *timed(a.reps, lambda tm: BandField.from_spheres(grid, sub, 2.5 * h, w, timings=tm)))
        iv, it = icosphere()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        verts = (sub[:, None, :] + torch.as_tensor(iv * np.float32(2.5 * h), device=DEV)[None]).reshape(-1, 3).contiguous()
        tris = (torch.as_tensor(it, device=DEV)[None] + (torch.arange(m, device=DEV) * iv.shape[0])[:, None, None]).reshape(-1)
        torch.cuda.synchronize()
        merge_ms = (time.perf_counter() - t0) * 1e3
        best = None
        for r in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with Mesh(verts, Topology.TriangleList(tris)) as mesh, mesh.narrow_band_field(grid, w, SignMethod.Raycast, True, background=w) as f:
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                count = f.count
            if r and (best is None or wall < best):
                best = wall
        say(f"{m} icospheres of {it.shape[0]} triangles ({tris.numel() // 3} triangles) through Mesh.narrow_band_field: {count} cells | merging the meshes "
            f"{merge_ms:.3f} ms, mesh + band field {best:.3f} ms wall")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
