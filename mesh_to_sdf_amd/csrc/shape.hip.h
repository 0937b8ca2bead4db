// shape.hip.h — the distance to a capsule (a segment a-b with a radius r; a sphere is the capsule with a == b) and the index box of the grid
// points it can reach: the definition behind m2s_band_from_capsules (include/m2s.h).  IEEE binary32, no FMA, sums left to
// right, so the host build (geo_probe.hip), tests/band_shapes_model.py and the kernels of band_shapes.hip give the same bits.
//
// THE DEFINITION.  For a point c and a sound shape s (every coordinate finite, r >= 0 and finite):
//   ab = b - a;  ap = c - a;  den = (ab.x ab.x + ab.y ab.y) + ab.z ab.z
//   t  = den > 0 ? clamp(((ap.x ab.x + ap.y ab.y) + ap.z ab.z) / den, 0, 1) : 0         clamp(x) = x < 0 ? 0 : (x > 1 ? 1 : x)
//   e  = ap - t ab                                                                      per component: one product, one subtraction
//   d_s = sqrtf((e.x e.x + e.y e.y) + e.z e.z) - r
// and D(c) = the minimum of d_s over the sound shapes, +inf when there is none.  A d_s that is NaN (the differences of coordinates beyond
// 1.7e38 overflow) passes no comparison below: the shape adds nothing at that point.
// Rounding.  The division and sqrtf are the correctly rounded IEEE operations: hipcc emits them for `/` and sqrtf in device code unless
// -ffast-math or -fhip-fp32-correctly-rounded-divide-sqrt=off is given, and the Makefile gives neither (tests/test_band_shapes_cpu.py
// checks the host build against numpy, the GPU tests check the kernels against the same numpy model).
// d_s is never -0: a difference of equal finite numbers is +0 in round-to-nearest.
//
// WHAT THE VALUES MEAN.  Outside the union D is the Euclidean distance to it up to the rounding below.  Inside, the minimum over the shapes
// is the depth below the nearest shape's own surface: a LOWER BOUND of the depth below the union's surface, as after every level-set CSG
// (m2s_band_csg says the same of its results).  m2s_band_redistance turns it into distances again.
//
// ERROR BOUND, in units of u = 2^-24 times scale, scale >= every |coordinate| of a, b and c and >= r.  Write delta for the true distance
// from c to the segment and p^ = a + t^ ab^ for the foot the computed t^ and ab^ = fl(b - a) name; t^ is in [0, 1] exactly (the clamp does
// not round).
//   The differences: a component of ab^ or ap^ is off by at most u times itself, at most 2 u scale.  p^ lies within 2 sqrt(3) u scale of the
//   point a + t^ (b - a) of the true segment.
//   e: a component is fl(ap^ - fl(t^ ab^)): 2 u scale from ap^, 2 u scale from the product, 4 u scale from the subtraction (|e| <= 4 scale
//   per component): 8 u scale per component, 8 sqrt(3) u scale < 14 u scale for the vector.
//   The norm: three squares, two sums and a correctly rounded root are within a relative 2.5 u of |e| <= 4 sqrt(3) scale: < 18 u scale.
//   So sqrtf(..) >= delta - (3.5 + 14 + 18) u scale = delta - 35.5 u scale: THE LOWER SIDE, which the box below rests on.
//   The upper side adds how far p^ is from the true foot along the segment, |t^ - t*| |ab|.  The dot product is within 3 u |ap| |ab| of the
//   exact one of ap^ and ab^, those within 2 u |ap| |ab| of the true one; den is a sum of squares, relative 5 u with ab^'s own error; the
//   division adds u.  Where the clamp does not decide, |t*| <= 1 + 7 u, so |t^ - t*| |ab| <= 5 u |ap| + 7 u |ab| <= 24 sqrt(3) u scale
//   < 42 u scale.  (A foot that moves along the segment changes the distance in the second order only; the bound takes the first.)
//   A den that underflows (|ab| below 1e-19) loses relative accuracy in t^, but the whole segment is then shorter than 1e-19.
//   The last subtraction rounds by u |d_s| <= u (4 sqrt(3) + 1) scale < 8 u scale.
//   Together  |d_s - (delta - r)| <= (35.5 + 42 + 8) u scale < SHAPE_ERR_U u scale = 96 u scale,  and the same holds for D, a minimum of
//   such values, against the minimum of the true ones.  tests/golden/shapes_error.json records what the tests measured beside it.
//
// THE BOX is a superset of the points with a COMPUTED d_s <= exterior.  fl(s - r) <= exterior gives s <= (r + exterior)(1 + 2 u), and the
// lower side gives delta <= s + 35.5 u scale (scale here: the coordinates only; r is covered by the relative term).  Along one axis the gap
// G from c to the interval [min(a, b), max(a, b)] is at most delta, and band_gap computes it with one subtraction: G_computed <= G (1 + u).
// So a point in reach passes  G_computed <= (r + exterior)(1 + SHAPE_REL) + SHAPE_REL scale  with SHAPE_REL = 8e-6 = 134 u, a reserve of 3.7
// over the 35.5 u and of 40 over the 3 u.  The comparison is band.hip.h's band_near (squares; rounding and underflow are monotone, so
// G <= reach implies fl(G G) <= fl(reach reach)) and the interval is band.hip.h's band_interval: found with the predicate's own operations
// on the walk's own cell_center, not with a division that would have to be trusted.  The kernels evaluate every point of the box with
// the exact d_s, so the box only has to contain what can pass.
#pragma once
#include "band.hip.h"

#pragma clang fp contract(off)

namespace m2s {

constexpr float SHAPE_REL = 8.0e-6f;
constexpr float SHAPE_ERR_U = 96.0f;

struct Capsule {
  float a[3], b[3];
  float r;
};

M2S_HD bool shape_sound(const Capsule& s) {
  bool ok = band_finite(s.r) && s.r >= 0.0f;
#pragma unroll
  for (int m = 0; m < 3; ++m) ok = ok && band_finite(s.a[m]) && band_finite(s.b[m]);
  return ok;
}

M2S_HD float shape_dist(const Capsule& s, float cx, float cy, float cz) {
  const float abx = s.b[0] - s.a[0], aby = s.b[1] - s.a[1], abz = s.b[2] - s.a[2];
  const float apx = cx - s.a[0], apy = cy - s.a[1], apz = cz - s.a[2];
  const float den = (abx * abx + aby * aby) + abz * abz;
  float t = 0.0f;
  if (den > 0.0f) {
    t = ((apx * abx + apy * aby) + apz * abz) / den;
    t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
  }
  const float ex = apx - t * abx, ey = apy - t * aby, ez = apz - t * abz;
  return sqrtf((ex * ex + ey * ey) + ez * ez) - s.r;
}

// The largest |centre| a grid has: the scale of every c.
M2S_HD float shape_grid_scale(const float (&first)[3], const float (&size)[3], const uint32_t (&cnt)[3]) {
  float g = 0.0f;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const float c0 = fabsf(cell_center(first[m], size[m], 0u)), c1 = fabsf(cell_center(first[m], size[m], cnt[m] - 1u));
    g = c0 > g ? c0 : g;
    g = c1 > g ? c1 : g;
  }
  return g;
}

// (r + exterior)(1 + SHAPE_REL) + SHAPE_REL x scale, scale = the largest |coordinate| of the shape and of any cell centre.  +inf for huge
// widths: every point then passes.
M2S_HD float shape_reach(const Capsule& s, float exterior, float grid_scale) {
  float scale = grid_scale;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    scale = fabsf(s.a[m]) > scale ? fabsf(s.a[m]) : scale;
    scale = fabsf(s.b[m]) > scale ? fabsf(s.b[m]) : scale;
  }
  const float grown = (s.r + exterior) * (1.0f + SHAPE_REL);
  const float slack = SHAPE_REL * scale;
  return grown + slack;
}

// [lo, hi) per axis: the index box of a sound shape.  Empty on one axis: the shape reaches no grid point.
M2S_HD void shape_box(const Capsule& s, const float (&first)[3], const float (&size)[3], const uint32_t (&cnt)[3], float exterior, float grid_scale,
                      uint32_t (&lo)[3], uint32_t (&hi)[3]) {
  const float reach = shape_reach(s, exterior, grid_scale), reach2 = reach * reach;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const float blo = s.a[m] < s.b[m] ? s.a[m] : s.b[m], bhi = s.a[m] < s.b[m] ? s.b[m] : s.a[m];
    band_interval(blo, bhi, first[m], size[m], 0u, cnt[m], 0.0f, 0.0f, reach2, &lo[m], &hi[m]);
  }
}

// The order-preserving 32-bit key of a float that is not NaN: x < y iff key(x) < key(y) as unsigned integers (-0 below +0).
M2S_HD uint32_t shape_key(float x) {
  uint32_t u;
  __builtin_memcpy(&u, &x, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
M2S_HD float shape_unkey(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float x;
  __builtin_memcpy(&x, &u, 4);
  return x;
}
constexpr uint32_t SHAPE_KEY_INF = 0xff800000u;   // shape_key(+inf)

}  // namespace m2s
