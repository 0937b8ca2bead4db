#!/usr/bin/env python3
"""Cost of CSG on narrow bands (include/m2s.h m2s_band_csg / m2s_band_export) and of the mesh boolean built on it, on device-resident
data.  blob-100k and a copy translated by a quarter of its extent (Raycast), bands three cells wide with the sign mask of voxelize(solid),
at 256^3, 512^3 and 2048^3 (--grids).
  - csg: m2s_timings.seed_ms of m2s_band_csg per op, best of --reps after one warm-up of that very call;
  - export: m2s_timings.distance_ms of m2s_band_export of the union (cells, distances, sign mask);
  - beside each, the bytes the call must move — every index word of both operands once (mask, sign mask), the result's three index arrays
    once, the band values in and out (export: mask and offsets in, the three lists out) — and the time those bytes take at the HBM rate
    --hbm (TB/s; 6.29 is the measured copy rate of the MI355X);
  - boolean: the whole mesh -> band fields -> csg -> export -> band isosurface pipeline on two resident meshes, wall time, best of --reps;
  - at 256^3 and 512^3 the dense alternative: torch.minimum of the two dense grids and grid_isosurface of it, wall time, with and without
    the two generate_grid_sdf calls that make the grids; it is compared with the union's mesh.  At 2048^3 a dense grid is 32 GiB and
    the three the alternative needs have nothing to run on.

usage: tools/exp_band_csg.py [--out profiles/band_csg.txt] [--grids 256,512,2048] [--reps 5] [--hbm 6.29]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mesh_to_sdf_amd import CsgOp, Grid, M2STimings, Mesh, SignMethod, Topology, grid_isosurface, meshes  # noqa: E402

DENSE_MAX = 512
OPS = [CsgOp.Union, CsgOp.Intersection, CsgOp.Difference]


def best_ms(reps, fn, field):
    """Best `field` of m2s_timings over `reps` runs of fn(timings) after one warm-up; fn's result is closed if it can be."""
    out = 1e30
    for r in range(reps + 1):
        t = M2STimings()
        res = fn(t)
        if hasattr(res, "close"):
            res.close()
        if r:
            out = min(out, getattr(t, field))
    return out


def best_wall(reps, fn):
    out = 1e30
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r:
            out = min(out, (time.perf_counter() - t0) * 1e3)
    return out


def same(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--grids", default="256,512,2048")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hbm", type=float, default=6.29)
    a = ap.parse_args()
    v, idx = meshes.named("blob-100k")
    v2 = (v + np.array([0.25 * float(v[:, 0].max() - v[:, 0].min()), 0.0, 0.0], np.float32)).astype(np.float32)
    lo, hi = meshes.extended_bbox(np.concatenate([v, v2]), 0.1)
    ti = Topology.TriangleList(torch.as_tensor(idx.astype(np.int64), device="cuda:0"))
    lines = [f"# blob-100k ({idx.size // 3} triangles) and a copy moved by a quarter of its extent along x, {torch.cuda.get_device_name(0)}; Raycast, "
             f"bands of 3 cells either side, sign masks from voxelize(solid); device memory; kernel times from m2s_timings, wall times with a "
             f"device synchronisation either side; best of {a.reps} after one warm-up; 'floor' = the bytes a call must move at {a.hbm} TB/s"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    with Mesh(torch.as_tensor(v, device="cuda:0"), ti) as ma, Mesh(torch.as_tensor(v2, device="cuda:0"), ti) as mb:
        for n in [int(x) for x in a.grids.split(",")]:
            grid = Grid.from_bounding_box(lo, hi, [n, n, n])
            w = 3.0 * float(max(grid.get_cell_size()))
            words = (n ** 3 + 63) // 64
            with ma.narrow_band_field(grid, w, SignMethod.Raycast, True, background=w) as fa, \
                    mb.narrow_band_field(grid, w, SignMethod.Raycast, True, background=w) as fb:
                say(f"grid {n}^3: A {fa.count} cells, B {fb.count} cells ({fa.count / n ** 3:.2%} of the grid each); a handle "
                    f"{fa.device_bytes / 2**20:.1f} MiB (a dense grid: {4 * n ** 3 / 2**20:.0f} MiB)")
                for op in OPS:
                    with fa.csg(fb, op) as fr:
                        n_r = fr.count
                    ms = best_ms(a.reps, lambda t: fa.csg(fb, op, timings=t), "seed_ms")
                    moved = 8 * words * (4 + 3) + 4 * (fa.count + fb.count + n_r)
                    floor = moved / (a.hbm * 1e9)
                    say(f"grid {n}^3 csg {op.name}: {n_r} cells | {ms:.3f} ms | must move {moved / 2**20:.1f} MiB, floor {floor:.3f} ms, "
                        f"{ms / floor:.2f} x the floor")
                with fa | fb as fu:
                    ms = best_ms(a.reps, lambda t: fu.to_band(timings=t), "distance_ms")
                    moved = 8 * words * 3 + fu.count * (8 + 4 + 4) + 4 * n * n * ((n + 31) // 32)
                    floor = moved / (a.hbm * 1e9)
                    say(f"grid {n}^3 export of the union: {fu.count} cells | {ms:.3f} ms | must move {moved / 2**20:.1f} MiB, floor {floor:.3f} ms, "
                        f"{ms / floor:.2f} x the floor")
                    uv, ui, n_open = fu.isosurface(0.0)
            for op in OPS:
                ms = best_wall(a.reps, lambda: ma.boolean(mb, op, grid))
                bv, bi = ma.boolean(mb, op, grid)
                say(f"grid {n}^3 boolean {op.name} (two resident meshes -> mesh): {ms:.2f} ms wall | {bv.shape[0]} vertices, {bi.shape[0]} triangles")
            if n <= DENSE_MAX:
                da, db = ma.generate_grid_sdf(grid, SignMethod.Raycast), mb.generate_grid_sdf(grid, SignMethod.Raycast)
                ms_op = best_wall(a.reps, lambda: grid_isosurface(grid, torch.minimum(da, db)))
                ms_all = best_wall(a.reps, lambda: grid_isosurface(grid, torch.minimum(ma.generate_grid_sdf(grid, SignMethod.Raycast),
                                                                                       mb.generate_grid_sdf(grid, SignMethod.Raycast))))
                dv, di = grid_isosurface(grid, torch.minimum(da, db))
                bv, bi = ma.boolean(mb, CsgOp.Union, grid)
                say(f"grid {n}^3 dense union: torch.minimum + grid_isosurface {ms_op:.2f} ms wall, with the two generate_grid_sdf {ms_all:.2f} ms wall "
                    f"(three dense grids: {3 * 4 * n ** 3 / 2**20:.0f} MiB) | the boolean's mesh: "
                    f"{'the same bits' if same(dv, bv) and same(di, bi) else f'differs ({dv.shape[0]} / {bv.shape[0]} vertices)'}")
                del da, db, dv, di
            else:
                say(f"grid {n}^3 dense union: nothing to run on: three dense grids are {3 * 4 * n ** 3 / 2**30:.0f} GiB")
            del uv, ui
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
