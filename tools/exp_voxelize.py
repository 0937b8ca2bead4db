#!/usr/bin/env python3
"""Cost of voxelization (include/m2s.h m2s_mesh_voxelize) on device-resident data, from the library's HIP events, best of five calls after
one warm-up, per shape:
  - SURFACE and SOLID, mask only (bits_out) and mask + occupancy bytes: m2s_timings.distance_ms (the voxelization kernels), seed_ms (the
    sign planes, SOLID) and total_ms;
  - the candidate count: the sum over triangles of the cells in their exact candidate boxes (what the raster kernel walks), and the
    columns among them, computed here in numpy with the contract's own box clause;
  - the set count;
  - the complete generate_grid_sdf call of the same mesh and grid in the same run (total_ms, Raycast sign): the route to occupancy
    without this call.
Shapes: blob-100k at 128^3, 256^3, 512^3 and 1024^3, blob-1M at 512^3.

usage: tools/exp_voxelize.py [--out profiles/voxelize.txt] [--shapes blob-100k:128,...] [--once]
(--once: one SURFACE and one SOLID call per shape and nothing else — for a kernel trace)"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mesh_to_sdf_amd import Grid, M2STimings, Mesh, SignMethod, Topology, meshes  # noqa: E402

F = np.float32


def best_of(call, reps=5):
    call(None)
    best = None
    for _ in range(reps):
        t = M2STimings()
        call(t)
        if best is None or t.total_ms < best.total_ms:
            best = t
    return best


def candidates(v, idx, grid):
    """(columns, cells) summed over the triangles' candidate boxes: per axis, the indices that pass the box clause (every index tried)."""
    tri = v[idx.reshape(-1, 3).astype(np.int64)]                                  # [T, 3, 3]
    first, size, count = np.array(grid.get_first_cell(), F), np.array(grid.get_cell_size(), F), grid.get_cell_count()
    ext = []
    fin = np.isfinite(tri).all((1, 2))
    for m in range(3):
        q = (first[m] + (np.arange(count[m]).astype(F) * size[m]).astype(F)).astype(F)
        h = F(size[m] * F(0.5))
        n = np.zeros(tri.shape[0], np.int64)
        for s in range(0, tri.shape[0], 20000):                                   # chunks: T x n booleans
            p = tri[s:s + 20000, :, m]
            va, vb, vc = (p[:, k, None] - q[None, :] for k in range(3))
            below = (va > h) & (vb > h) & (vc > h)
            above = (va < -h) & (vb < -h) & (vc < -h)
            n[s:s + 20000] = (~(below | above)).sum(1)
        ext.append(n)
    live = fin & (ext[0] > 0) & (ext[1] > 0) & (ext[2] > 0)
    cols = (ext[0] * ext[1])[live]
    return int(cols.sum()), int((cols * ext[2][live]).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/voxelize.txt")
    ap.add_argument("--shapes", default="blob-100k:128,blob-100k:256,blob-100k:512,blob-100k:1024,blob-1M:512")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    lines = [f"# {torch.cuda.get_device_name(0)}; ms from the library's HIP events, best of 5 (by total_ms) after a warm-up; device memory",
             "# kernels = distance_ms, planes = seed_ms, call = total_ms; sdf = total_ms of generate_grid_sdf (Raycast) on the same mesh and grid"]
    loaded = {}
    for shape in a.shapes.split(","):
        name, n = shape.split(":")
        n = int(n)
        if name not in loaded:
            loaded.clear()
            v, idx = meshes.named(name)
            loaded[name] = (v, idx, torch.as_tensor(v, device="cuda"), torch.as_tensor(idx.astype(np.int64), device="cuda"))
        v, idx, dv, di = loaded[name]
        lo, hi = meshes.extended_bbox(v, 0.1)
        grid = Grid.from_bounding_box(lo, hi, [n, n, n])
        with Mesh(dv, Topology.TriangleList(di)) as m:
            if a.once:
                m.voxelize(grid, False, bits=True, occupancy=False)
                m.voxelize(grid, True, bits=True, occupancy=False)
                torch.cuda.synchronize()
                continue
            cols, cand = candidates(v, idx, grid)
            out = torch.empty(grid.get_total_cell_count(), dtype=torch.float32, device="cuda")
            sdf = best_of(lambda t: m.generate_grid_sdf(grid, SignMethod.Raycast, timings=t, out=out))
            del out
            row = [f"{name} ({idx.size // 3} triangles) in {n}^3: candidate columns {cols}, candidate cells {cand} ({cand / (idx.size // 3):.1f} per triangle); "
                   f"generate_grid_sdf call {sdf.total_ms:.3f} ms"]
            for solid in (False, True):
                for label, kw in (("mask", dict(bits=True, occupancy=False)), ("mask + bytes", dict(bits=True, occupancy=True))):
                    res = {}

                    def call(t, kw=kw, solid=solid, res=res):
                        res["r"] = m.voxelize(grid, solid, timings=t, count=t is None, **kw)   # (the count's trip to the host stays out of the timed calls)
                    t = best_of(call)
                    row.append(f"  {'SOLID  ' if solid else 'SURFACE'} {label:<12}: kernels {t.distance_ms:.4f} ms, planes {t.seed_ms:.4f} ms, call {t.total_ms:.4f} ms; "
                               f"set {m.voxelize(grid, solid, occupancy=False).count}; sdf / call = {sdf.total_ms / t.total_ms:.1f}")
                    del res
            lines += row
            torch.cuda.empty_cache()
    if a.once:
        return
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
