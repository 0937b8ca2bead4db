#!/usr/bin/env python3
"""Cost of measuring a narrow band (include/m2s.h m2s_band_measure) on device-resident data, beside the route it replaces, on the
workload of tools/exp_band_components.py: blob-100k and a copy translated by a quarter of its extent (Raycast), bands three cells wide
with the sign mask of voxelize(solid), their union, united with the band of one small debris blob, at 256^3, 512^3 and 2048^3 (--grids).
  - measure: the whole call (m2s_timings.total_ms: clearing the records and the one kernel), without labels and with the labels of
    m2s_band_components at connectivity 26 (one record per component), with what it measured;
  - the route it replaces, in the same run on the same handle: m2s_band_export (m2s_timings.total_ms) and m2s_band_isosurface of the
    exported lists (m2s_timings.total_ms of its filling call; the Python call runs it twice, count then fill), and the wall-clock time of
    the two together up to a device synchronisation, which is what a caller waits for before the mesh can be summed up on the host;
  - the float64 area and volume of that mesh summed on the host, to show what the two routes agree on.
All times best of --reps after one warm-up of the very call.

usage: tools/exp_band_measure.py [--out profiles/band_measure.txt] [--grids 256,512,2048] [--reps 5]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from exp_band_components import best_of  # noqa: E402
from mesh_to_sdf_amd import Grid, M2STimings, Mesh, SignMethod, Topology, meshes  # noqa: E402


def mesh_measures(v, t):
    """Float64 area and volume of a mesh on the device, summed in chunks."""
    area = vol = 0.0
    for a in range(0, t.shape[0], 1 << 22):
        tri = t[a:a + (1 << 22)].long()
        p0, p1, p2 = (v[tri[:, k]].double() for k in range(3))
        area += 0.5 * float(torch.linalg.norm(torch.linalg.cross(p1 - p0, p2 - p0), dim=1).sum())
        vol += float((p0 * torch.linalg.cross(p1, p2)).sum()) / 6.0
    return area, vol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--grids", default="256,512,2048")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--note", default="")
    a = ap.parse_args()
    v, idx = meshes.named("blob-100k")
    ext = v.max(0) - v.min(0)
    v2 = (v + np.array([0.25 * float(ext[0]), 0.0, 0.0], np.float32)).astype(np.float32)
    centre = 0.5 * (v.max(0) + v.min(0))
    v3 = ((v - centre) * 0.05 + centre + np.array([0.0, 0.0, 0.62 * float(ext[2])], np.float32)).astype(np.float32)   # the debris, above the blobs
    lo, hi = meshes.extended_bbox(np.concatenate([v, v2, v3]), 0.1)
    ti = Topology.TriangleList(torch.as_tensor(idx.astype(np.int64), device="cuda:0"))
    lines = [f"# blob-100k ({idx.size // 3} triangles), a copy moved by a quarter of its extent along x and a debris copy a twentieth of the size, "
             f"{torch.cuda.get_device_name(0)}; Raycast, bands of 3 cells either side, sign masks from voxelize(solid), the union of all three; "
             f"device memory; times are m2s_timings.total_ms unless they say wall, best of {a.reps} after one warm-up" + (f"; {a.note}" if a.note else "")]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    with Mesh(torch.as_tensor(v, device="cuda:0"), ti) as ma, Mesh(torch.as_tensor(v2, device="cuda:0"), ti) as mb, \
            Mesh(torch.as_tensor(v3, device="cuda:0"), ti) as md:
        for n in [int(x) for x in a.grids.split(",")]:
            grid = Grid.from_bounding_box(lo, hi, [n, n, n])
            w = 3.0 * float(max(grid.get_cell_size()))
            with ma.narrow_band_field(grid, w, SignMethod.Raycast, True, background=w) as fa, \
                    mb.narrow_band_field(grid, w, SignMethod.Raycast, True, background=w) as fb, \
                    md.narrow_band_field(grid, w, SignMethod.Raycast, True, background=w) as fd, fa | fb as fab, fab | fd as fu:
                say(f"grid {n}^3: the union has {fu.count} cells ({fu.count / n ** 3:.2%} of the grid)")
                t, m = best_of(a.reps, lambda tm: fu.measure(timings=tm))
                say(f"grid {n}^3 measure, no labels: {m.n_triangles} triangles, {m.n_vertices} vertices, n_open {m.n_open}, n_border {m.n_border}, euler {m.euler}, "
                    f"area {m.area:.9g}, volume {m.volume:.9g} | total {t.total_ms:.3f} ms, {t.total_ms * 1e6 / max(fu.count, 1):.2f} ns per cell")
                comps = fu.components(26)
                t, parts = best_of(a.reps, lambda tm: fu.measure(0.0, comps, timings=tm))
                say(f"grid {n}^3 measure, {comps.count} components (connectivity 26): volumes {[float(f'{p.volume:.6g}') for p in parts[:6]]}, euler "
                    f"{[p.euler for p in parts[:6]]}, closed {[p.closed for p in parts[:6]]} | total {t.total_ms:.3f} ms")
                # the route it replaces: export the lists, extract the mesh
                best_wall, te, ti_ = None, None, None
                for r in range(a.reps + 1):
                    t1, t2 = M2STimings(), M2STimings()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    nb = fu.to_band(timings=t1)
                    vv, tt, n_open = nb.isosurface(timings=t2)
                    torch.cuda.synchronize()
                    wall = (time.perf_counter() - t0) * 1e3
                    if r and (best_wall is None or wall < best_wall):
                        best_wall, te, ti_ = wall, t1.total_ms, t2.total_ms
                    if r < a.reps:
                        del nb, vv, tt
                area, vol = mesh_measures(vv, tt)
                say(f"grid {n}^3 export + isosurface: {tt.shape[0]} triangles, {vv.shape[0]} vertices, n_open {n_open} | export {te:.3f} ms, isosurface (the "
                    f"filling call) {ti_:.3f} ms, both with the counting call up to a synchronisation {best_wall:.3f} ms wall | the mesh summed in "
                    f"float64: area {area:.9g}, volume {vol:.9g} (relative to the measure {area / m.area - 1:+.2e}, {vol / m.volume - 1:+.2e})")
                del nb, vv, tt
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
