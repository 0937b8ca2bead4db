#!/usr/bin/env python3
"""Cost of m2s_band_isosurface (include/m2s.h) on device-resident narrow bands of blob-100k (Raycast), iso 0: the band of
isosurface_band(grid, 0) (1.001 cell diagonals either side, the one whose mesh is the dense mesh) and a band of 3 cells either side, at
256^3, 512^3 and 1024^3; at 2048^3, which no dense grid call can hold beside its output, the first band only.
  - call: the whole C call (count-only and fill), timed by HIP events around it on the call's stream, best of 5 after one warm-up;
  - kernels: m2s_timings.distance_ms of the same calls, best of 5;
  - dense: m2s_grid_isosurface on the dense grid of the same shape, in the same process (up to 1024^3), and whether the two meshes are
    the same bits;
  - pipelines: narrow_band_sdf + band_isosurface against generate_grid_sdf + grid_isosurface through the Python API (which counts, then
    fills), by HIP events, best of 3;
  - device memory in use (hipMemGetInfo) once the last band call has returned, the library's workspace included: the high-water mark
    of the sparse pipeline, since the workspace only grows.
The per-kernel split comes from a `rocprofv3 --kernel-trace --stats` run of this tool with --extract-only, a run of its own
(profiles/band_isosurface.txt).

usage: tools/exp_band_isosurface.py [--out profiles/band_isosurface.txt] [--grids 256,512,1024,2048] [--extract-only]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mesh_to_sdf_amd import (Grid, M2STimings, SignMethod, Topology, _lib, generate_grid_sdf, grid_isosurface, isosurface_band, meshes,  # noqa: E402
                             narrow_band_sdf)

DENSE_MAX = 1024


def _opts(stream, t=None):
    o = _lib.M2SOpts()
    o.struct_size = C.sizeof(o)
    o.device = 0
    o.mem_kind = _lib.MEM_DEVICE
    o.stream = stream.cuda_stream
    o.stream_mode = 1
    o.synchronous = 1
    if t is not None:
        o.timings = C.pointer(t)
    return o


def _timed(s, reps, fn):
    """(best ms by HIP events, best m2s_timings.distance_ms) of fn(timings) over `reps` runs after one warm-up."""
    best = kern = 1e30
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = M2STimings()
        torch.cuda.synchronize()
        e0.record(s)
        fn(t)
        e1.record(s)
        torch.cuda.synchronize()
        if r:
            best = min(best, e0.elapsed_time(e1))
            kern = min(kern, t.distance_ms)
    return best, kern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--grids", default="256,512,1024,2048")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--extract-only", action="store_true", help="the isosurface_band band's calls alone (for a kernel trace): no dense call, no pipelines")
    a = ap.parse_args()
    v, idx = meshes.named("blob-100k")
    lo, hi = meshes.extended_bbox(v, 0.1)
    tv = torch.as_tensor(v, device="cuda:0")
    ti = Topology.TriangleList(torch.as_tensor(idx.astype(np.int64), device="cuda:0"))
    L = _lib.lib()
    s = torch.cuda.current_stream()
    lines = [f"# blob-100k ({idx.size // 3} triangles), {torch.cuda.get_device_name(0)}; Raycast, iso 0, device memory; best of {a.reps} "
             f"(pipelines: best of 3)"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    for n in [int(x) for x in a.grids.split(",")]:
        grid = Grid.from_bounding_box(lo, hi, [n, n, n])
        G = C.byref(grid._g)
        h = float(min(grid.get_cell_size()))
        dense = n <= DENSE_MAX and not a.extract_only
        d = dense_mesh = None
        if dense:
            d = generate_grid_sdf(tv, ti, grid, SignMethod.Raycast)
            cnt2 = (C.c_uint64 * 2)()

            def dense_call(vo, to, cv, ct, t=None):
                rc = L.m2s_grid_isosurface(G, d.data_ptr(), 0.0, vo, cv, to, ct, cnt2, C.byref(_opts(s, t)))
                assert rc == 0, _lib.last_error()

            dense_call(None, None, 0, 0)
            dnv, dnt = int(cnt2[0]), int(cnt2[1])
            dvb = torch.empty((dnv, 3), dtype=torch.float32, device="cuda:0")
            dtb = torch.empty((dnt, 3), dtype=torch.int32, device="cuda:0")
            dc_count, dk_count = _timed(s, a.reps, lambda t: dense_call(None, None, 0, 0, t))
            dc_fill, dk_fill = _timed(s, a.reps, lambda t: dense_call(dvb.data_ptr(), dtb.data_ptr(), dnv, dnt, t))
            dense_mesh = (dvb, dtb)
            say(f"grid {n}^3 dense ({4 * n ** 3 / 2**20:.0f} MiB): {dnv} vertices, {dnt} triangles | grid_isosurface call count-only {dc_count:.3f} ms, "
                f"fill {dc_fill:.3f} ms | kernels count-only {dk_count:.3f} ms, fill {dk_fill:.3f} ms")
        bands = [("isosurface_band", isosurface_band(grid, 0.0))]
        if n <= DENSE_MAX and not a.extract_only:
            bands.append(("3 cells", (3.0 * h, 3.0 * h)))
        for name, widths in bands:
            band = narrow_band_sdf(tv, ti, grid, widths, SignMethod.Raycast)
            cells, dist, nb = band.cells, band.distances, band.count
            cnt = (C.c_uint64 * 3)()

            def call(vo, to, cv, ct, t=None):
                rc = L.m2s_band_isosurface(G, cells.data_ptr(), dist.data_ptr(), nb, 0.0, vo, cv, to, ct, cnt, C.byref(_opts(s, t)))
                assert rc == 0, _lib.last_error()

            call(None, None, 0, 0)
            nv, nt, n_open = int(cnt[0]), int(cnt[1]), int(cnt[2])
            vb = torch.empty((nv, 3), dtype=torch.float32, device="cuda:0")
            tb = torch.empty((nt, 3), dtype=torch.int32, device="cuda:0")
            c_count, k_count = _timed(s, a.reps, lambda t: call(None, None, 0, 0, t))
            c_fill, k_fill = _timed(s, a.reps, lambda t: call(vb.data_ptr(), tb.data_ptr(), nv, nt, t))
            same = ""
            if dense_mesh is not None:
                eq = vb.shape == dense_mesh[0].shape and tb.shape == dense_mesh[1].shape and bool((vb.view(torch.int32) == dense_mesh[0].view(torch.int32)).all()) \
                    and bool((tb == dense_mesh[1]).all())
                same = f" | the dense mesh bit for bit: {'yes' if eq else 'NO'}"
            free, total = torch.cuda.mem_get_info()
            say(f"grid {n}^3 band {name} ({widths[0] / h:.2f} + {widths[1] / h:.2f} cells): {nb} cells ({12 * nb / 2**20:.0f} MiB, {nb / n ** 3:.2%} of the grid), "
                f"{nv} vertices, {nt} triangles, n_open {n_open} | band_isosurface call count-only {c_count:.3f} ms, fill {c_fill:.3f} ms | kernels count-only "
                f"{k_count:.3f} ms, fill {k_fill:.3f} ms{same} | device memory in use {(total - free) / 2**30:.2f} GiB")
            if not a.extract_only:
                p_sparse, _ = _timed(s, 3, lambda t: narrow_band_sdf(tv, ti, grid, widths, SignMethod.Raycast).isosurface(0.0))
                line = f"grid {n}^3 band {name}: pipeline narrow_band_sdf + band_isosurface {p_sparse:.2f} ms"
                if dense and name == "isosurface_band":
                    p_dense, _ = _timed(s, 3, lambda t: grid_isosurface(grid, generate_grid_sdf(tv, ti, grid, SignMethod.Raycast)))
                    line += f" | generate_grid_sdf + grid_isosurface {p_dense:.2f} ms"
                say(line)
            del band, cells, dist, vb, tb
            torch.cuda.empty_cache()
        del d, dense_mesh
        if dense:
            del dvb, dtb
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
