// sign.hip.h — the index arithmetic of sign.hip: which grid lines a triangle's padded box can meet (axis_range, make_window), which of them
// an x-slab owns (SlabX, x_in_slab), the bucket of a hit along its line (ray_bucket), and the constants and the rule that choose the path a
// call takes through sign.hip (sign_path).  Host-compilable like voxel.hip.h (geo_probe.hip builds it for tests/test_sign_planes_cpu.py).
#pragma once
#include "common.h"
#include "geo.hip.h"

namespace m2s {

constexpr uint32_t SMALL_WINDOW = 64;  // lines a lane handles alone; larger windows are spread over the wave
#ifndef M2S_RAY_SHARED_BELOW
#define M2S_RAY_SHARED_BELOW 16384
#endif
constexpr uint32_t RAY_MARK_SHARED_BELOW = M2S_RAY_SHARED_BELOW;   // meshes of up to this many triangles: sixteen lanes per triangle (k_ray_mark<16>)
constexpr uint32_t BIG_CHUNK = 2048;   // lines of a big window one workgroup pass handles (256 threads x 8)
// Grids whose largest possible window (a whole face of the grid) exceeds this use the work list for big windows.
constexpr uint64_t LIST_ABOVE_LINES = 4096;

struct Window {
  uint32_t ulo, uhi, wlo, whi;  // inclusive index ranges on the two free axes; empty if ulo > uhi
};

M2S_HD void axis_range(float bmn, float bmx, float first, float cs, uint32_t n, uint32_t* lo, uint32_t* hi) {
  // conservative index range of cells whose centre first + i*cs can lie in [bmn, bmx]
  float i0 = (bmn - first) / cs, i1 = (bmx - first) / cs;
  if (i0 > i1) { float t = i0; i0 = i1; i1 = t; }
  const bool bad = !(i0 == i0) || !(i1 == i1) || !(fabsf(i0) < 3.0e38f) || !(fabsf(i1) < 3.0e38f);
  if (bad) { *lo = 0; *hi = n - 1; return; }
  // cells whose centre index lies in [i0, i1], widened by a tolerance that covers the f32 rounding of
  // the index computation (the exact closed-interval test on the true centres decides membership)
  const float tol = 1.0e-3f + 4.0e-6f * fmaxf(fabsf(i0), fabsf(i1)) + 1.0e-6f * (fabsf(bmn) + fabsf(bmx) + fabsf(first)) / fabsf(cs);
  const float l = ceilf(i0 - tol), h = floorf(i1 + tol);
  if (h < 0.0f || l > (float)(n - 1) || h < l) { *lo = 1; *hi = 0; return; }
  *lo = l < 0.0f ? 0u : (uint32_t)l;
  *hi = h >= (float)(n - 1) ? n - 1 : (uint32_t)h;
}

template <int AXIS>
struct FreeAxes {
  static constexpr int U = AXIS == 0 ? 1 : 0;
  static constexpr int W = AXIS == 2 ? 1 : 2;
};

// A call that computes an x-slab only needs the planes of the slab's layers: Y- and Z-lines lie inside one x-layer,
// so a line outside the slab is never looked at (its markers would only be read by cells the call does not compute); X-lines cross
// all layers and are all traced — their hits are slab-independent, t is measured from cell 0 — but the suffix scan along x stops
// at the slab's first layer.  SlabX: the real x-layers of the slab ([lo, hi) is their hull; an interleaved slab owns the chunks
// [lo + j * period, + 2^chunk_log) inside it); all == true: the whole grid (persistent meshes keep their planes per grid, not per slab).
struct SlabX {
  uint32_t lo, hi, chunk_log, period;
  bool all;
};
M2S_HD bool x_in_slab(const SlabX& sx, uint32_t x) {
  if (sx.all) return true;
  if (x < sx.lo || x >= sx.hi) return false;
  return sx.chunk_log >= 31u || ((x - sx.lo) % sx.period) < (1u << sx.chunk_log);
}
template <int AXIS>
M2S_HD Window make_window(f3 mn, f3 mx, const GridParams& g, const SlabX& sx) {
  constexpr int U = FreeAxes<AXIS>::U, W = FreeAxes<AXIS>::W;
  const float bmn[3] = {mn.x, mn.y, mn.z}, bmx[3] = {mx.x, mx.y, mx.z};
  Window w;
  axis_range(bmn[U], bmx[U], g.first[U], g.size[U], g.n[U], &w.ulo, &w.uhi);
  axis_range(bmn[W], bmx[W], g.first[W], g.size[W], g.n[W], &w.wlo, &w.whi);
  if (AXIS != 0 && !sx.all && w.ulo <= w.uhi) {      // U is x for the Y- and Z-lines: only the slab's layers
    w.ulo = w.ulo > sx.lo ? w.ulo : sx.lo;           // (no min / max here: the host's overloads are the signed ones)
    w.uhi = w.uhi < sx.hi - 1u ? w.uhi : sx.hi - 1u;
  }
  if (w.wlo > w.whi) { w.ulo = 1; w.uhi = 0; }
  return w;
}
M2S_HD uint32_t window_count(const Window& w) {
  return w.ulo > w.uhi ? 0u : (w.uhi - w.ulo + 1u) * (w.whi - w.wlo + 1u);
}

// Bucket of a hit at parameter t along a line of n cells of size cell_size: min(floor(t / cell_size) as usize, n - 1), grid.rs:605-607.
// The cast is guarded by 2^32, not by (float)n: above 2^24 cells (float)n can round below n, and a hit at f == (float)n <= n - 1 belongs
// into cell f, not into the last one (tests/test_sign_planes_cpu.py::test_bucket_against_the_numpy_f32_model, n = 2^31 + 5).
M2S_HD uint32_t ray_bucket(float t, float cell_size, uint32_t n) {
  const float f = floorf(t / cell_size);                                         // grid.rs:605-606
  uint32_t k = 0;                                                                // `as usize` saturates, NaN -> 0
  if (f == f && f > 0.0f) {
    const uint32_t last = n - 1, c = f >= 4294967296.0f ? last : (uint32_t)f;
    k = c < last ? c : last;                                                     // .min(n - 1), grid.rs:607
  }
  return k;
}

M2S_HD bool use_big_list(const GridParams& g) {
  const uint64_t a = (uint64_t)g.n[1] * g.n[2], b = (uint64_t)g.n[0] * g.n[2], c = (uint64_t)g.n[0] * g.n[1];
  const uint64_t ab = a > b ? a : b;
  return (ab > c ? ab : c) > LIST_ABOVE_LINES;
}

// The path a call takes through sign.hip, from the mesh's triangle count and the grid's counts alone.
struct SignPath {
  uint32_t lanes;   // lanes per triangle of k_ray_mark: 16 or 1
  bool list;        // big windows go onto the work list of k_ray_mark_big; else the owner's wave walks them
  bool rows;        // k_scan_z_combine_rows (a lane per word, segmented shuffles); else k_scan_z_combine (a thread per row, serial carry)
};
M2S_HD SignPath sign_path(uint32_t n_tris, const GridParams& g) {
  return {n_tris <= RAY_MARK_SHARED_BELOW ? 16u : 1u, use_big_list(g), g.nzw <= 64 && (g.nzw & (g.nzw - 1)) == 0};
}

}  // namespace m2s
