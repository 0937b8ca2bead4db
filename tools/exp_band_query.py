#!/usr/bin/env python3
"""Cost of the band queries (include/m2s.h m2s_band_create / m2s_band_sample / m2s_band_raymarch) on device-resident data, beside the
dense m2s_sample_grid / m2s_raymarch_grid on the dense grid D' the band stands for (the same bits, checked here).  blob-100k (Raycast),
a band three cells wide with the sign mask of voxelize(solid), at 256^3 and 512^3; at 2048^3, where D' would take 32 GiB, the band calls
alone (--grids).
  - index: m2s_timings.seed_ms of m2s_band_create (mask + offsets + sign mask), best of --reps after one warm-up;
  - points: --points points drawn within the band (band cell centres displaced by up to half a cell), every mode, values alone and
    values + normals: m2s_timings.distance_ms (the kernel), best of --reps after one warm-up of that very call;
  - rays: a res x res pinhole camera outside the box looking at the mesh, every mode, hit + steps and + normals, the same way;
  - the three fetch forms of the band kernels (M2S_BAND_FETCH): 0 "rounds", three rounds of independent loads with a normal's samples in
    groups of 24 corners; 1 "chain", corner after corner; 2 "rounds-small", the three rounds with groups of 16 / 12 corners; alternating
    within one process.  The library's own choice (M2S_BAND_FETCH=-1) is "rounds" in m2s_band_sample and "rounds-small" in m2s_band_raymarch.

usage: tools/exp_band_query.py [--out profiles/band_query.txt] [--grids 256,512,2048] [--points 4000000] [--res 1024] [--reps 5]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mesh_to_sdf_amd import BandField, Grid, M2STimings, Mesh, SampleMode, SignMethod, Topology, _lib, meshes, raymarch_grid, sample_grid  # noqa: E402

DENSE_MAX = 512
MODES = [SampleMode.Snap, SampleMode.Trilinear, SampleMode.Tetrahedral]


def best(reps, fn):
    """Best m2s_timings.distance_ms of fn(timings) over `reps` runs after one warm-up."""
    out = 1e30
    for r in range(reps + 1):
        t = M2STimings()
        fn(t)
        if r:
            out = min(out, t.distance_ms)
    return out


def camera(lo, hi, res):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    centre, size = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    eye = centre + np.array([0.9, 0.55, 1.3]) * size
    fwd = (centre - eye) / np.linalg.norm(centre - eye)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    u = (np.arange(res) + 0.5) / res * 2 - 1
    uu, vv = np.meshgrid(u, u)
    r = fwd + 0.3 * (uu[..., None] * right + vv[..., None] * up)
    r = (r / np.linalg.norm(r, axis=-1, keepdims=True)).reshape(-1, 3).astype(np.float32)
    return np.repeat(eye[None].astype(np.float32), r.shape[0], 0), r


def same(a, b):
    return bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--grids", default="256,512,2048")
    ap.add_argument("--points", type=int, default=4000000)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    v, idx = meshes.named("blob-100k")
    lo, hi = meshes.extended_bbox(v, 0.1)
    tv = torch.as_tensor(v, device="cuda:0")
    ti = Topology.TriangleList(torch.as_tensor(idx.astype(np.int64), device="cuda:0"))
    o_h, r_h = camera(lo, hi, a.res)
    org, ray = torch.as_tensor(o_h, device="cuda:0"), torch.as_tensor(r_h, device="cuda:0")
    lines = [f"# blob-100k ({idx.size // 3} triangles), {torch.cuda.get_device_name(0)}; Raycast, band of 3 cells either side, sign mask from "
             f"voxelize(solid); device memory; kernel times (m2s_timings), best of {a.reps} after one warm-up; {a.points} points within the band, "
             f"{a.res} x {a.res} rays; M/s = million points or rays per second"]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(1)
    with Mesh(tv, ti) as mesh:
        for n in [int(x) for x in a.grids.split(",")]:
            grid = Grid.from_bounding_box(lo, hi, [n, n, n])
            cs = torch.as_tensor(np.asarray(grid.get_cell_size(), np.float32), device="cuda:0")
            first = torch.as_tensor(np.asarray(grid.get_first_cell(), np.float32), device="cuda:0")
            h = float(max(grid.get_cell_size()))
            nb = mesh.narrow_band_sdf(grid, 3.0 * h, SignMethod.Raycast)
            vox = mesh.voxelize(grid, solid=True, bits=True, occupancy=False, count=False)
            build = 1e30
            for r in range(a.reps + 1):
                t = M2STimings()
                f = BandField(grid, nb.cells, nb.distances, inside=vox, timings=t)
                if r:
                    build = min(build, t.seed_ms)
                if r < a.reps:
                    f.close()
            field = f
            say(f"grid {n}^3: band {nb.count} cells ({nb.count / n ** 3:.2%} of the grid), handle {field.device_bytes / 2**20:.1f} MiB "
                f"(a dense grid: {4 * n ** 3 / 2**20:.0f} MiB) | index build {build:.3f} ms")
            # points within the band: the centres of random band cells displaced by up to half a cell
            pick = nb.cells[torch.randint(0, nb.count, (a.points,), generator=gen, device="cuda:0")]
            ijk = torch.stack([pick // (n * n), (pick // n) % n, pick % n], 1).to(torch.float32)
            pts = (first + (ijk + torch.rand((a.points, 3), generator=gen, device="cuda:0") - 0.5) * cs).contiguous()
            dense = None
            if n <= DENSE_MAX:
                bg_in, bg_out = field.background
                k = torch.arange(n, device="cuda:0")
                inside = ((vox.bits.view(torch.int32)[:, :, k >> 5] >> (k & 31)) & 1).bool()
                dense = torch.where(inside, torch.tensor(-bg_in, device="cuda:0"), torch.tensor(bg_out, device="cuda:0")).reshape(-1)
                dense[nb.cells] = nb.distances
                del inside
            for mode in MODES:
                row = {}
                for form in (0, 1, 2, 0, 1, 2):                            # the fetch forms, alternating
                    with _lib.knobs(M2S_BAND_FETCH=form):
                        tag = ("rounds", "chain", "rounds-small")[form]
                        for what, fn in (("sample", lambda t: field.sample(pts, mode=mode, timings=t)),
                                         ("sample+normals", lambda t: field.sample(pts, mode=mode, normals=True, timings=t)),
                                         ("march", lambda t: field.raymarch(org, ray, mode=mode, timings=t)),
                                         ("march+normals", lambda t: field.raymarch(org, ray, mode=mode, normals=True, timings=t))):
                            row[(tag, what)] = min(row.get((tag, what), 1e30), best(a.reps, fn))
                if dense is not None:
                    row[("dense", "sample")] = best(a.reps, lambda t: sample_grid(grid, dense, pts, mode=mode, timings=t))
                    row[("dense", "sample+normals")] = best(a.reps, lambda t: sample_grid(grid, dense, pts, mode=mode, normals=True, timings=t))
                    row[("dense", "march")] = best(a.reps, lambda t: raymarch_grid(grid, dense, org, ray, mode=mode, timings=t))
                    row[("dense", "march+normals")] = best(a.reps, lambda t: raymarch_grid(grid, dense, org, ray, mode=mode, normals=True, timings=t))
                    gv, gn = field.sample(pts, mode=mode, normals=True)
                    dv, dn = sample_grid(grid, dense, pts, mode=mode, normals=True)
                    gp, gd, gs, gh, gm = field.raymarch(org, ray, mode=mode, normals=True)
                    dp, dd, ds, dh, dm = raymarch_grid(grid, dense, org, ray, mode=mode, normals=True)
                    eq = same(gv, dv) and same(gn, dn) and same(gp, dp) and same(gd, dd) and bool((gs.view(torch.int32) == ds.view(torch.int32)).all()) and same(gm, dm)
                    check = f" | the dense call's bits: {'yes' if eq else 'NO'}"
                else:
                    check = ""
                _, _, steps, hit, sup = field.raymarch(org, ray, mode=mode, support=True)
                vals, s8 = field.sample(pts, mode=mode, support=True)
                kk = {SampleMode.Snap: 1, SampleMode.Trilinear: 8, SampleMode.Tetrahedral: 4}[mode]
                say(f"grid {n}^3 {mode.name}: {float((s8 == kk).float().mean()):.1%} of the points read band cells only; {float(hit.float().mean()):.1%} "
                    f"of the rays hit, {float(steps.view(torch.int32).float().mean()):.1f} steps per ray{check}")
                for what, units in (("sample", a.points), ("sample+normals", a.points), ("march", a.res * a.res), ("march+normals", a.res * a.res)):
                    parts = []
                    for tag in ("rounds", "chain", "rounds-small", "dense"):
                        if (tag, what) in row:
                            ms = row[(tag, what)]
                            parts.append(f"{tag} {ms:.3f} ms ({units / ms / 1e3:.0f} M/s)")
                    say(f"grid {n}^3 {mode.name} {what}: " + " | ".join(parts))
            field.close()
            del nb, vox, pts, dense, pick, ijk
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
