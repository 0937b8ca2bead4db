// voxel.hip.h — the triangle / cell overlap predicate of m2s_voxelize as include/m2s.h states it: the separating-axis test of
// Akenine-Möller (2001) with its operations fixed.  IEEE binary32, no FMA, sums left to right.  `min(x, y, z) > r` is evaluated as
// "x > r and y > r and z > r" (and `max < -r` likewise), so a NaN in any term never misses.  Also the per-axis interval searches that
// turn a box clause into a range of cell indices.  Host-compilable like ray.hip.h (geo_probe.hip builds it for the CPU tests);
// tests/voxel_model.py is its numpy twin.
#pragma once
#include "geo.hip.h"

#pragma clang fp contract(off)

namespace m2s {

// What a triangle contributes to every cell test.  finite == false: some coordinate is not finite — the triangle overlaps nothing.
struct VoxTri {
  float a[3], b[3], c[3];
  float e[3][3];   // e[0] = b - a, e[1] = c - b, e[2] = a - c
  float n[3];      // e[0] x e[1]
  bool finite;
};

M2S_HD bool vox_finite(float x) { return x - x == 0.0f; }

M2S_HD VoxTri vox_tri(f3 a, f3 b, f3 c) {
  VoxTri t;
  t.a[0] = a.x; t.a[1] = a.y; t.a[2] = a.z;
  t.b[0] = b.x; t.b[1] = b.y; t.b[2] = b.z;
  t.c[0] = c.x; t.c[1] = c.y; t.c[2] = c.z;
  bool fin = true;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    t.e[0][m] = t.b[m] - t.a[m];
    t.e[1][m] = t.c[m] - t.b[m];
    t.e[2][m] = t.a[m] - t.c[m];
    fin = fin && vox_finite(t.a[m]) && vox_finite(t.b[m]) && vox_finite(t.c[m]);
  }
  t.n[0] = t.e[0][1] * t.e[1][2] - t.e[0][2] * t.e[1][1];
  t.n[1] = t.e[0][2] * t.e[1][0] - t.e[0][0] * t.e[1][2];
  t.n[2] = t.e[0][0] * t.e[1][1] - t.e[0][1] * t.e[1][0];
  t.finite = fin;
  return t;
}

// Centre of cell `idx` along one axis: m2s_grid_cell_center's arithmetic.  Non-decreasing in idx (f32 rounding is monotone).
M2S_HD float vox_centre(float first, float size, uint32_t idx) {
  const float prod = (float)idx * size;
  return first + prod;
}

M2S_HD bool vox_all_gt(float x, float y, float z, float r) { return x > r && y > r && z > r; }
M2S_HD bool vox_all_lt(float x, float y, float z, float r) { return x < r && y < r && z < r; }

// The two halves of a box clause for a cell centre q along one axis.  `below` (min(v) > h) holds on a prefix of the cell indices,
// `above` (max(v) < -h) on a suffix: q does not decrease with the index, so v = p - q does not increase.
M2S_HD bool vox_box_below(float pa, float pb, float pc, float q, float h) { return vox_all_gt(pa - q, pb - q, pc - q, h); }
M2S_HD bool vox_box_above(float pa, float pb, float pc, float q, float h) { return vox_all_lt(pa - q, pb - q, pc - q, -h); }

// [lo, hi): the cells of one axis that pass its box clause, found with the clause's own operations: lo = the first index where `below`
// fails, hi = the first index where `above` holds (n when none).  At most 31 steps each for n < 2^31.  Empty when lo >= hi.
M2S_HD void vox_interval(float pa, float pb, float pc, float first, float size, uint32_t n, uint32_t* lo_out, uint32_t* hi_out) {
  const float h = size * 0.5f;
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (vox_box_below(pa, pb, pc, vox_centre(first, size, mid), h)) lo = mid + 1;
    else hi = mid;
  }
  *lo_out = lo;
  hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (vox_box_above(pa, pb, pc, vox_centre(first, size, mid), h)) hi = mid;
    else lo = mid + 1;
  }
  *hi_out = lo;
}

// Plane clause.  v0 = a - q.
M2S_HD bool vox_plane_miss(const VoxTri& t, const float (&v0)[3], const float (&h)[3]) {
  const float d = (t.n[0] * v0[0] + t.n[1] * v0[1]) + t.n[2] * v0[2];
  const float r = (h[0] * fabsf(t.n[0]) + h[1] * fabsf(t.n[1])) + h[2] * fabsf(t.n[2]);
  return d > r || d < -r;
}

// Cross axis (edge e, axis M).  All three projections are computed; none is reused.
template <int M>
M2S_HD bool vox_cross_miss(const float (&e)[3], const float (&v0)[3], const float (&v1)[3], const float (&v2)[3], const float (&h)[3]) {
  constexpr int m1 = (M + 1) % 3, m2 = (M + 2) % 3;
  const float p0 = e[m1] * v0[m2] - e[m2] * v0[m1];
  const float p1 = e[m1] * v1[m2] - e[m2] * v1[m1];
  const float p2 = e[m1] * v2[m2] - e[m2] * v2[m1];
  const float r = h[m1] * fabsf(e[m2]) + h[m2] * fabsf(e[m1]);
  return vox_all_gt(p0, p1, p2, r) || vox_all_lt(p0, p1, p2, -r);
}

// The clauses that do not depend on the cell's z beyond the box clauses of x and y: the three cross axes with m = z.
M2S_HD bool vox_column_miss(const VoxTri& t, const float (&v0)[3], const float (&v1)[3], const float (&v2)[3], const float (&h)[3]) {
  return vox_cross_miss<2>(t.e[0], v0, v1, v2, h) || vox_cross_miss<2>(t.e[1], v0, v1, v2, h) || vox_cross_miss<2>(t.e[2], v0, v1, v2, h);
}
// The plane and the six cross axes with m = x, y.
M2S_HD bool vox_cell_miss(const VoxTri& t, const float (&v0)[3], const float (&v1)[3], const float (&v2)[3], const float (&h)[3]) {
  if (vox_plane_miss(t, v0, h)) return true;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (vox_cross_miss<0>(t.e[j], v0, v1, v2, h) || vox_cross_miss<1>(t.e[j], v0, v1, v2, h)) return true;
  return false;
}

// overlap(t, cell): all 13 clauses, for the cell of centre q and half extent h.
M2S_HD bool vox_overlap(const VoxTri& t, const float (&q)[3], const float (&h)[3]) {
  if (!t.finite) return false;
  float v0[3], v1[3], v2[3];
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    v0[m] = t.a[m] - q[m];
    v1[m] = t.b[m] - q[m];
    v2[m] = t.c[m] - q[m];
    if (vox_all_gt(v0[m], v1[m], v2[m], h[m]) || vox_all_lt(v0[m], v1[m], v2[m], -h[m])) return false;
  }
  return !vox_column_miss(t, v0, v1, v2, h) && !vox_cell_miss(t, v0, v1, v2, h);
}

}  // namespace m2s
