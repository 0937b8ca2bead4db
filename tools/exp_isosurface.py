#!/usr/bin/env python3
"""Cost of m2s_grid_isosurface (include/m2s.h) on device-resident grids: the blob-100k Raycast grid at 256^3, 512^3 (the headline's
output) and 1024^3, iso 0.
  - call: the whole C call (count-only and fill), timed by HIP events around it on the call's stream, best of 5 after one warm-up;
  - kernels: m2s_timings.distance_ms of the fill call (its kernels, first to last, host waits included), best of 5;
  - vertex and triangle counts, active points;
  - the bytes the full-grid passes must move, counted from shapes (k_iso_classify reads the grid once and writes the 1-bit mask;
    k_iso_compact reads the mask), as a fraction of 8 TB/s over the kernels' time.  Take the passes' own time from a
    `rocprofv3 --kernel-trace --stats` run of this tool (profiles/isosurface.txt).

usage: tools/exp_isosurface.py [--out profiles/isosurface.txt] [--grids 256,512,1024]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mesh_to_sdf_amd import Grid, M2STimings, SignMethod, Topology, _lib, generate_grid_sdf, meshes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--grids", default="256,512,1024")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    v, idx = meshes.named("blob-100k")
    lo, hi = meshes.extended_bbox(v, 0.1)
    tv = torch.as_tensor(v, device="cuda:0")
    ti = Topology.TriangleList(torch.as_tensor(idx.astype(np.int64), device="cuda:0"))
    L = _lib.lib()
    s = torch.cuda.current_stream()
    lines = [f"# blob-100k ({idx.size // 3} triangles), {torch.cuda.get_device_name(0)}; Raycast grids, iso 0, device memory; best of {a.reps}"]
    for n in [int(x) for x in a.grids.split(",")]:
        grid = Grid.from_bounding_box(lo, hi, [n, n, n])
        d = generate_grid_sdf(tv, ti, grid, SignMethod.Raycast)
        cnt = (C.c_uint64 * 2)()

        def call(vo, to, cv, ct, t=None):
            o = _lib.M2SOpts()
            o.struct_size = C.sizeof(o)
            o.device = 0
            o.mem_kind = _lib.MEM_DEVICE
            o.stream = s.cuda_stream
            o.stream_mode = 1
            o.synchronous = 1
            if t is not None:
                o.timings = C.pointer(t)
            rc = L.m2s_grid_isosurface(C.byref(grid._g), d.data_ptr(), 0.0, vo, cv, to, ct, cnt, C.byref(o))
            assert rc == 0, _lib.last_error()

        call(None, None, 0, 0)
        nv, nt = int(cnt[0]), int(cnt[1])
        vb = torch.empty((nv, 3), dtype=torch.float32, device="cuda:0")
        tb = torch.empty((nt, 3), dtype=torch.int32, device="cuda:0")

        def timed(fill):
            best = kern = 1e30
            for r in range(a.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t = M2STimings()
                torch.cuda.synchronize()
                e0.record(s)
                if fill:
                    call(vb.data_ptr(), tb.data_ptr(), nv, nt, t)
                else:
                    call(None, None, 0, 0, t)
                e1.record(s)
                torch.cuda.synchronize()
                if r:
                    best = min(best, e0.elapsed_time(e1))
                    kern = min(kern, t.distance_ms)
            return best, kern

        c_count, k_count = timed(False)
        c_fill, k_fill = timed(True)
        pts = n ** 3
        grid_bytes = 4 * pts + 2 * (pts / 8)   # the grid once, the mask written and read once
        frac = grid_bytes / (k_count * 1e-3) / 8e12
        lines.append(f"grid {n}^3 ({4 * pts / 2**20:.0f} MiB): {nv} vertices, {nt} triangles | call count-only {c_count:.3f} ms, fill "
                     f"{c_fill:.3f} ms | kernels (m2s_timings) count-only {k_count:.3f} ms, fill {k_fill:.3f} ms | full-grid bytes "
                     f"{grid_bytes / 2**20:.0f} MiB = {grid_bytes / (k_count * 1e-3) / 1e12:.2f} TB/s over the count-only kernels "
                     f"({frac:.1%} of 8 TB/s)")
        print(lines[-1], flush=True)
        del d, vb, tb
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
