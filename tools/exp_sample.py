#!/usr/bin/env python3
"""Cost of area-weighted surface sampling (include/m2s.h m2s_mesh_sample_surface) on device-resident data, from the library's HIP events:
  - the weight table (m2s_timings.seed_ms of the first sampling call on a fresh Mesh: k_tri_area, the scan, its header's trip to the
    host), best of five fresh meshes after one warm-up;
  - the sampling kernel (m2s_timings.distance_ms), best of five calls after one warm-up, for 1 M and 10 M samples, all outputs (point,
    triangle, uv, normal: 36 B per sample) and points only (12 B per sample);
on blob-100k and blob-1M.  Beside every kernel time: the time its output bytes alone would take at the HBM write rate of plain dword
stores (6.0 TB/s), the ratio of the two, and the existing 10 M-query RtreeBvh distance call on the same mesh (distance_ms), the scale
a sampler should sit well below.

usage: tools/exp_sample.py [--out profiles/sample.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mesh_to_sdf_amd import AccelerationMethod, M2STimings, Mesh, Topology, meshes  # noqa: E402

HBM_WRITE_TBS = 6.0   # plain dword stores, 256 B per wave instruction


def best_of(call, field, reps=5):
    call()
    out = []
    for _ in range(reps):
        t = M2STimings()
        call(t)
        out.append(getattr(t, field))
    return min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/sample.txt")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    lines = [f"# {torch.cuda.get_device_name(0)}; ms from the library's HIP events, best of 5 after a warm-up; device memory",
             f"# floor = output bytes / {HBM_WRITE_TBS} TB/s (HBM write rate of plain dword stores)"]
    for name in ("blob-100k", "blob-1M"):
        v, idx = meshes.named(name)
        dv, di = torch.as_tensor(v, device="cuda"), torch.as_tensor(idx.astype(np.int64), device="cuda")
        topo = Topology.TriangleList(di)

        def table(t=None):
            with Mesh(dv, topo) as fresh:
                fresh.sample_surface(64, timings=t)
        lines.append(f"{name} ({idx.size // 3} triangles): weight table {best_of(table, 'seed_ms'):.4f} ms (first sampling call of a fresh Mesh, seed_ms)")
        with Mesh(dv, topo) as m:
            lo, hi = meshes.extended_bbox(v, 0.1)
            q = torch.as_tensor(meshes.uniform_queries(lo, hi, 10_000_000), device="cuda")
            dist = best_of(lambda t=None: m.generate_sdf(q, AccelerationMethod.RtreeBvh, timings=t), "distance_ms")
            del q
            lines.append(f"  for scale: 10 M-query RtreeBvh distance call {dist:.3f} ms (distance_ms)")
            for n in (1_000_000, 10_000_000):
                for label, kw, bytes_per in (("all outputs", dict(normals=True), 36), ("points only", dict(points_only=True), 12)):
                    ms = best_of(lambda t=None: m.sample_surface(n, seed=1, timings=t, **kw), "distance_ms")
                    floor = n * bytes_per / (HBM_WRITE_TBS * 1e12) * 1e3
                    lines.append(f"  {n // 1_000_000:>2} M samples, {label}: kernel {ms:.4f} ms = {n / ms / 1e6:.2f} G samples/s, "
                                 f"{n * bytes_per / ms / 1e9:.3f} TB/s written; floor {floor:.4f} ms, kernel / floor = {ms / floor:.2f}; "
                                 f"distance call / kernel = {dist / ms:.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
