// grid_query.hip.h — the sampling arithmetic of the grid queries, shared by grid_query.hip (a dense grid) and band_query.hip (a narrow
// band behind an index): a sample prepared (the clamped cell offsets it reads and its weights) and the shader's arithmetic after the
// reads.  Moved here from grid_query.hip unchanged.  What differs between the two files is only how the K cell values are fetched.
// Include it under `#pragma clang fp contract(off)`: IEEE binary32 in the shader's operation order, no FMA.
// Everything is in an unnamed namespace: each translation unit that includes this has its own copy.
#pragma once
#include "../../include/m2s.h"
#include "common.h"

#pragma clang fp contract(off)

namespace m2s {
namespace {

constexpr uint32_t kQNaN = 0x7fc00000u;   // the NaN every NaN input produces (the model uses the same bits)

__device__ __forceinline__ float qnan() { return __uint_as_float(kQNaN); }

template <int MODE>
struct Corners { static constexpr int K = MODE == M2S_SAMPLE_SNAP ? 1 : MODE == M2S_SAMPLE_TRILINEAR ? 8 : 4; };

// One sample prepared: the clamped cell offsets it reads and its interpolation weights.
// state: 0 inside the box, 1 outside (the result is `outside`), 2 a NaN coordinate (the result is NaN).
template <int MODE>
struct Prep {
  uint64_t off[Corners<MODE>::K];
  float w[4];   // trilinear: fx, fy, fz; tetrahedral: bary
  int state;
};

__device__ __forceinline__ int64_t clamp_cell(int64_t i, int64_t n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// get_distance (:92-99) without the load: each index clamped to [0, count - 1], offset z + y*nz + x*ny*nz in 64 bits.
__device__ __forceinline__ uint64_t cell_off(const GridQuery& q, int64_t x, int64_t y, int64_t z) {
  return (uint64_t)clamp_cell(z, q.n[2]) + (uint64_t)clamp_cell(y, q.n[1]) * (uint64_t)q.n[2] +
         (uint64_t)clamp_cell(x, q.n[0]) * q.nyz;
}

template <int MODE>
__device__ __forceinline__ Prep<MODE> prepare(const GridQuery& q, float px, float py, float pz) {
  Prep<MODE> r;
  const bool nan = px != px || py != py || pz != pz;
  // :121 any(position < start) || any(position > end); a NaN coordinate fails every comparison and is caught above
  const bool out = px < q.start[0] || py < q.start[1] || pz < q.start[2] || px > q.end[0] || py > q.end[1] || pz > q.end[2];
  r.state = nan ? 2 : (out ? 1 : 0);
  if (r.state) { px = q.start[0]; py = q.start[1]; pz = q.start[2]; }   // keeps the conversions below defined and the reads in the grid
  if (MODE == M2S_SAMPLE_SNAP) {
    // :129-134 start_grid = start - cell_size * 0.5; cell_index = floor((position - start_grid) / cell_size)
    const float gx = q.start[0] - q.cs[0] * 0.5f, gy = q.start[1] - q.cs[1] * 0.5f, gz = q.start[2] - q.cs[2] * 0.5f;
    const int64_t ix = (int64_t)floorf((px - gx) / q.cs[0]);
    const int64_t iy = (int64_t)floorf((py - gy) / q.cs[1]);
    const int64_t iz = (int64_t)floorf((pz - gz) / q.cs[2]);
    r.off[0] = cell_off(q, ix, iy, iz);
  } else {
    // :159-161 / :181-183 cell_index = (position - start) / cell_size; fract = c - floor(c); idx = floor(c)
    const float cx = (px - q.start[0]) / q.cs[0], cy = (py - q.start[1]) / q.cs[1], cz = (pz - q.start[2]) / q.cs[2];
    const float flx = floorf(cx), fly = floorf(cy), flz = floorf(cz);
    const float fx = cx - flx, fy = cy - fly, fz = cz - flz;
    const int64_t ix = (int64_t)flx, iy = (int64_t)fly, iz = (int64_t)flz;
    if (MODE == M2S_SAMPLE_TRILINEAR) {
      r.w[0] = fx; r.w[1] = fy; r.w[2] = fz; r.w[3] = 0.0f;
#pragma unroll
      for (int k = 0; k < 8; ++k) r.off[k] = cell_off(q, ix + (k & 1), iy + ((k >> 1) & 1), iz + (k >> 2));
    } else {
      // compute_tetrahedral_barycenter (:585-640): the six cases in the shader's order, the LAST matching one wins
      // (r, g, b) = (x, y, z); vert2 / vert3 are the two middle vertices of the tetrahedron
      float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, b3 = 0.0f;
      int v2 = 0, v3 = 0;   // bits: x = 1, y = 2, z = 4
      if (fy >= fz && fz >= fx) { b0 = 1.0f - fy; b1 = fy - fz; b2 = fz - fx; b3 = fx; v2 = 2; v3 = 6; }
      if (fz > fx && fx > fy)   { b0 = 1.0f - fz; b1 = fz - fx; b2 = fx - fy; b3 = fy; v2 = 4; v3 = 5; }
      if (fz > fy && fy >= fx)  { b0 = 1.0f - fz; b1 = fz - fy; b2 = fy - fx; b3 = fx; v2 = 4; v3 = 6; }
      if (fx >= fy && fy > fz)  { b0 = 1.0f - fx; b1 = fx - fy; b2 = fy - fz; b3 = fz; v2 = 1; v3 = 3; }
      if (fy > fx && fx >= fz)  { b0 = 1.0f - fy; b1 = fy - fx; b2 = fx - fz; b3 = fz; v2 = 2; v3 = 3; }
      if (fx >= fz && fz >= fy) { b0 = 1.0f - fx; b1 = fx - fz; b2 = fz - fy; b3 = fy; v2 = 1; v3 = 5; }
      r.w[0] = b0; r.w[1] = b1; r.w[2] = b2; r.w[3] = b3;
      r.off[0] = cell_off(q, ix, iy, iz);
      r.off[1] = cell_off(q, ix + (v2 & 1), iy + ((v2 >> 1) & 1), iz + (v2 >> 2));
      r.off[2] = cell_off(q, ix + (v3 & 1), iy + ((v3 >> 1) & 1), iz + (v3 >> 2));
      r.off[3] = cell_off(q, ix + 1, iy + 1, iz + 1);
    }
  }
  return r;
}

// The arithmetic of sdf_grid after the reads; v[k] are the raw cell values (get_distance subtracts iso from each).
template <int MODE>
__device__ __forceinline__ float combine(const GridQuery& q, const Prep<MODE>& p, const float* v) {
  const float iso = q.iso;
  float val;
  if (MODE == M2S_SAMPLE_SNAP) {
    val = v[0] - iso;
  } else if (MODE == M2S_SAMPLE_TRILINEAR) {
    // :164-172; v[dx + 2 dy + 4 dz]
    const float fx = p.w[0], fy = p.w[1], fz = p.w[2];
    const float gx = 1.0f - fx, gy = 1.0f - fy, gz = 1.0f - fz;
    const float c_x00 = (v[0] - iso) * gx + (v[1] - iso) * fx;
    const float c_x01 = (v[4] - iso) * gx + (v[5] - iso) * fx;
    const float c_x10 = (v[2] - iso) * gx + (v[3] - iso) * fx;
    const float c_x11 = (v[6] - iso) * gx + (v[7] - iso) * fx;
    const float c_xy0 = c_x00 * gy + c_x10 * fy;
    const float c_xy1 = c_x01 * gy + c_x11 * fy;
    val = c_xy0 * gz + c_xy1 * fz;
  } else {
    // :187-196 dot(bary, samples), left to right
    val = p.w[0] * (v[0] - iso) + p.w[1] * (v[1] - iso) + p.w[2] * (v[2] - iso) + p.w[3] * (v[3] - iso);
  }
  // selected at the end, not branched on: a branch lets the compiler sink the reads into it and wait on them one pair at a time
  return p.state == 2 ? qnan() : (p.state == 1 ? q.outside : val);
}

}  // namespace
}  // namespace m2s
