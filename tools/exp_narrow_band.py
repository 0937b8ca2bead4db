#!/usr/bin/env python3
"""Cost of narrow-band grid SDFs (include/m2s.h m2s_mesh_narrow_band_sdf) on a persistent mesh and device-resident data, from the library's
HIP events, best of five calls after a warm-up, per shape, sign method and band width:
  - candidates evaluated (m2s_timings.n_units), active cells, their ratio, and the share of the grid that is active;
  - the split: seed_ms (sign planes + candidate pass), distance_ms (query walks + filter + compaction), total_ms.  The timed calls pass the
    exact count as capacity, so each is one call;
  - the dense generate_grid_sdf call of the same mesh, grid and sign method, timed in the same run (total_ms), unless the grid has more
    cells than --dense-max: there only the band is run, and the device memory the call took is printed.
--chunks runs every band under each value of M2S_BAND_CHUNK (the default's justification).

usage: tools/exp_narrow_band.py [--out profiles/narrow_band.txt] [--shapes blob-100k:256,...] [--widths 1,3,8] [--signs raycast,normal]
                                [--chunks 262144,1048576,4194304] [--dense-max 1100000000] [--once]
(--once: one call per shape, sign and width and nothing else — for a kernel trace)"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mesh_to_sdf_amd import Grid, M2STimings, Mesh, SignMethod, Topology, _lib, meshes  # noqa: E402

F = np.float32
SIGN = {"raycast": SignMethod.Raycast, "normal": SignMethod.Normal}


def best_of(call, reps=5):
    call(None)
    best = None
    for _ in range(reps):
        t = M2STimings()
        call(t)
        if best is None or t.total_ms < best.total_ms:
            best = t
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/narrow_band.txt")
    ap.add_argument("--shapes", default="blob-100k:256,blob-100k:512,blob-100k:1024,blob-1M:512,blob-100k:2048")
    ap.add_argument("--widths", default="1,3,8")
    ap.add_argument("--signs", default="raycast,normal")
    ap.add_argument("--chunks", default="")
    ap.add_argument("--dense-max", type=int, default=1100000000)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    widths = [float(w) for w in a.widths.split(",")]
    chunks = [int(c) for c in a.chunks.split(",")] if a.chunks else [None]
    lines = [f"# {torch.cuda.get_device_name(0)}; ms from the library's HIP events, best of 5 (by total_ms) after a warm-up; device memory, persistent mesh",
             "# band = +- width cells; cand = candidates evaluated, active = cells in the band; seed = sign planes + candidate pass, walk = query walks + filter +",
             "# compaction, call = total_ms of the narrow-band call; dense = total_ms of generate_grid_sdf on the same mesh, grid and sign method in this run"]
    loaded = {}

    def flush():
        text = "\n".join(lines) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)

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
        cells = grid.get_total_cell_count()
        h = float(min(grid.get_cell_size()))
        free0 = torch.cuda.mem_get_info()[0]
        with Mesh(dv, Topology.TriangleList(di)) as m:
            for sname in a.signs.split(","):
                sign = SIGN[sname]
                if a.once:
                    for w in widths:
                        m.narrow_band_sdf(grid, w * h, sign)
                    torch.cuda.synchronize()
                    continue
                dense = None
                if cells <= a.dense_max:
                    out = torch.empty(cells, dtype=torch.float32, device="cuda")
                    dense = best_of(lambda t: m.generate_grid_sdf(grid, sign, timings=t, out=out))
                    del out
                    torch.cuda.empty_cache()
                lines.append(f"{name} ({idx.size // 3} triangles) in {n}^3, {sname}: dense " + (f"{dense.total_ms:.3f} ms" if dense else "not run"))
                for w in widths:
                    for chunk in chunks:
                        with _lib.knobs(**({} if chunk is None else {"M2S_BAND_CHUNK": chunk})):
                            count = m.narrow_band_sdf(grid, w * h, sign).count
                            t = best_of(lambda t: m.narrow_band_sdf(grid, w * h, sign, timings=t, capacity=count))
                        used = free0 - torch.cuda.mem_get_info()[0]
                        lines.append(f"  band {w:g} cells" + (f", chunk {chunk}" if chunk else "") + f": cand {t.n_units}, active {count} ({100.0 * count / cells:.2f} % of the grid), "
                                     f"cand / active {t.n_units / max(1, count):.2f}; seed {t.seed_ms:.3f} ms, walk {t.distance_ms:.3f} ms, call {t.total_ms:.3f} ms"
                                     + (f"; dense / call = {dense.total_ms / t.total_ms:.2f}" if dense else f"; device memory taken {used / 2 ** 30:.2f} GiB"))
                        print(lines[-1], flush=True)
                        flush()
                torch.cuda.empty_cache()
    if a.once:
        return
    print("\n".join(lines))
    flush()


if __name__ == "__main__":
    main()
