// band.hip.h — the candidate predicate of m2s_narrow_band_sdf (include/m2s.h): which cells of a grid can have a dense
// distance of magnitude <= r, decided per triangle from its axis-aligned box alone.  IEEE binary32, no FMA, sums left to right, so the host
// build (geo_probe.hip) and tests/band_model.py give the same set as the kernels of band.hip.
//
// Why the set is a superset of the active cells.  A cell is active only if |D| <= r, and |D| is sqrt(min d2) of the dense walk or, in the
// Normal fold, a dpos >= that minimum: some triangle T has a COMPUTED distance d_T <= r to the cell's centre q (q is the walk's own
// cell_center, so it carries no error here).  With delta the true distance from q to T, the walks' margin argument (walk.hip.h "Pruning
// threshold") gives d_T >= delta (1 - e_T) - a_T with e_T <= 4 u and a_T <= 16 u x scale, u = 2^-24, scale >= every coordinate involved.
// The gap G from q to T's box is a true lower bound of delta computed with three subtractions, three products and two sums:
// G_computed <= delta (1 + 4 u).  So G_computed <= (r + a_T) (1 + 9 u), and the test below — G^2 <= (r (1 + 4e-6) + 4e-6 x scale)^2, the
// walks' prune_bound with its square root taken out, scale = the largest |coordinate| of the triangle and of any cell centre — keeps the
// same 4.8-fold reserve over those 14 u that PRUNE_REL keeps.  The plane test at the end of this file tightens the set without giving that up.
// A triangle with a non-finite coordinate can only yield a finite distance through a vertex-region select of geo.hip.h (every other closest
// point multiplies an edge vector that is not finite), so its box is the box of its finite vertices: still a lower bound of whatever finite
// distance the dense walk can compute for it.  A zero-area triangle lies in its box like any other.
#pragma once
#include "geo.hip.h"

#pragma clang fp contract(off)

namespace m2s {

constexpr float BAND_REL = 4.0e-6f;   // walk.hip.h PRUNE_REL, and the factor of the walks' absolute slack

// The box of a triangle's finite vertices.  any == false: no vertex is finite — the triangle is nobody's candidate.
struct BandBox {
  float lo[3], hi[3];
  float amax;   // largest |coordinate| of those vertices
  bool any;
};

M2S_HD bool band_finite(float x) { return x - x == 0.0f; }

M2S_HD BandBox band_box(f3 a, f3 b, f3 c) {
  const float p[3][3] = {{a.x, a.y, a.z}, {b.x, b.y, b.z}, {c.x, c.y, c.z}};
  BandBox bx;
  bx.any = false;
  bx.amax = 0.0f;
#pragma unroll
  for (int m = 0; m < 3; ++m) bx.lo[m] = bx.hi[m] = 0.0f;
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    if (!(band_finite(p[v][0]) && band_finite(p[v][1]) && band_finite(p[v][2]))) continue;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const float x = p[v][m];
      bx.lo[m] = (!bx.any || x < bx.lo[m]) ? x : bx.lo[m];
      bx.hi[m] = (!bx.any || x > bx.hi[m]) ? x : bx.hi[m];
      bx.amax = fabsf(x) > bx.amax ? fabsf(x) : bx.amax;
    }
    bx.any = true;
  }
  return bx;
}

// r (1 + BAND_REL) + BAND_REL x scale: the walks' prune_bound with its square root taken out.  The tests compare squares with reach * reach,
// +inf for a large r: every cell then passes.
M2S_HD float band_reach(float r, float scale) {
  const float grown = r * (1.0f + BAND_REL);
  const float slack = BAND_REL * scale;
  return grown + slack;
}

// Distance from q to the interval [lo, hi] along one axis.
M2S_HD float band_gap(float lo, float hi, float q) {
  const float below = lo - q, above = q - hi;
  float g = 0.0f;
  g = below > g ? below : g;
  g = above > g ? above : g;
  return g;
}

// The predicate: the squared gap to the box is within reach.  Adding a non-negative term never lowers the sum in binary32, so a cell that
// passes also passes with any of its gaps replaced by 0: the per-axis and per-column forms below are necessary conditions of this one.
M2S_HD bool band_near(float gx, float gy, float gz, float reach2) { return (gx * gx + gy * gy) + gz * gz <= reach2; }

// [lo, hi): the indices of [begin, end) along one axis whose centre passes band_near with the other two gaps fixed at (g1, g2), found with
// the predicate's own operations as vox_interval does.  Centres do not decrease with the index, so "below the box and out of reach" holds
// on a prefix and "above the box and out of reach" on a suffix.  (0, 0) for the other gaps gives the axis's own interval: the sum is then
// the axis's g * g exactly, whichever slot it stands in.
M2S_HD void band_interval(float blo, float bhi, float first, float size, uint32_t begin, uint32_t end, float g1, float g2, float reach2,
                          uint32_t* lo_out, uint32_t* hi_out) {
  uint32_t lo = begin, hi = end;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const float q = cell_center(first, size, mid);
    if (blo - q > 0.0f && !band_near(g1, g2, band_gap(blo, bhi, q), reach2)) lo = mid + 1;
    else hi = mid;
  }
  *lo_out = lo;
  hi = end;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const float q = cell_center(first, size, mid);
    if (q - bhi > 0.0f && !band_near(g1, g2, band_gap(blo, bhi, q), reach2)) hi = mid;
    else lo = mid + 1;
  }
  *hi_out = lo;
}

// ---- the plane test: tighter than the box for a triangle that lies askew in it ------------------------------------------------------------------
// The distance from q to the triangle is at least its distance to the triangle's plane, |n . (q - a)| / |n| with n = (b - a) x (c - a).  A cell
// is dropped for a triangle only if  |t| > reach (|n| + 16 u E) + 32 u E W  with everything computed in binary32 (u = 2^-24):
//   t = (n.x w.x + n.y w.y) + n.z w.z,  w = q - a;   E = |b - a| |c - a| >= |n|;   W >= |w|: the sum over the axes of the larger distance from a
//   to the grid's first and last centre, one number per triangle, so that the right-hand side is the same for every cell.
// Margin.  Rounding the edges moves b and c by at most u x scale, which reach's slack holds many times over.  A component x y - z w of n is
// off by at most 2 u (|x y| + |z w|) <= 2 u E, the vector by 3.5 u E, the computed |n| by 5.5 u E with its own rounding; the computed t differs
// from n . w by at most 3 u |n| |w| for the dot product, u |n| |w| for w and 3.5 u E |w| for n: 7.5 u E W together.  The right-hand side itself is
// four operations, 4 u of it.  16 u and 32 u leave those sums a reserve of 1.7 and 4.  So a dropped cell has a true plane distance above
// reach, and reach already exceeds what any triangle with a computed distance <= r can have (top of this file).
// t does not decrease along z when n.z >= 0 and does not increase otherwise (w.z is monotone in the index and so is every rounding), so the
// cells a column keeps form one interval: the searches below find it with the clause's own operations.
// A triangle with a non-finite coordinate takes no plane test (use == false); a zero-area one has n = 0, takes none and drops nothing.
// The margins above are relative: they hold while no product underflows.  Below |n|^2 = 1e-30 (edges of some 1e-8) the squares of n's
// components leave the normal range and the computed |n| falls short, so such a triangle takes no plane test either; above it a product of t
// that underflows loses at most 2^-149, far inside 16 u E reach.
constexpr float BAND_PLANE_MIN_N2 = 1.0e-30f;
struct BandPlane {
  float a[3], n[3];
  float rhs;
  bool use;
};

M2S_HD BandPlane band_plane(f3 a, f3 b, f3 c, float reach, const float (&first)[3], const float (&size)[3], const uint32_t (&cnt)[3]) {
  BandPlane pl;
  pl.a[0] = a.x; pl.a[1] = a.y; pl.a[2] = a.z;
  const f3 e0 = sub3(b, a), e1 = sub3(c, a), n = cross3(e0, e1);
  pl.n[0] = n.x; pl.n[1] = n.y; pl.n[2] = n.z;
  const float n2 = dot3(n, n), nlen = sqrtf(n2), E = sqrtf(dot3(e0, e0)) * sqrtf(dot3(e1, e1));
  float W = 0.0f;
  bool fin = band_finite(b.x) && band_finite(b.y) && band_finite(b.z) && band_finite(c.x) && band_finite(c.y) && band_finite(c.z);
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const float d0 = fabsf(cell_center(first[m], size[m], 0u) - pl.a[m]), d1 = fabsf(cell_center(first[m], size[m], cnt[m] - 1u) - pl.a[m]);
    W = W + (d0 > d1 ? d0 : d1);
    fin = fin && band_finite(pl.a[m]);
  }
  const float lhs = reach * (nlen + 9.5367431640625e-07f * E);   // 16 u
  const float err = 1.9073486328125e-06f * (E * W);              // 32 u
  pl.rhs = lhs + err;
  pl.use = fin && n2 >= BAND_PLANE_MIN_N2;
  return pl;
}

// The x and y terms of t: the same for a whole column.
M2S_HD float band_plane_xy(const BandPlane& pl, float qx, float qy) { return pl.n[0] * (qx - pl.a[0]) + pl.n[1] * (qy - pl.a[1]); }
M2S_HD float band_plane_t(const BandPlane& pl, float sxy, float qz) { return sxy + pl.n[2] * (qz - pl.a[2]); }
// A NaN on either side drops nothing.
M2S_HD bool band_plane_far(const BandPlane& pl, float t) { return pl.use && (t > pl.rhs || t < -pl.rhs); }

// [lo, hi): the indices of [begin, end) along z that the plane test keeps in the column of sxy.
M2S_HD void band_plane_interval(const BandPlane& pl, float sxy, float first, float size, uint32_t begin, uint32_t end, uint32_t* lo_out, uint32_t* hi_out) {
  *lo_out = begin;
  *hi_out = end;
  if (!pl.use) return;
  const bool up = pl.n[2] >= 0.0f;   // t does not decrease with the index
  uint32_t lo = begin, hi = end;
  while (lo < hi) {   // the prefix on the far side the column starts on
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const float t = band_plane_t(pl, sxy, cell_center(first, size, mid));
    if (up ? t < -pl.rhs : t > pl.rhs) lo = mid + 1;
    else hi = mid;
  }
  *lo_out = lo;
  hi = end;
  while (lo < hi) {   // the suffix on the far side it ends on
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const float t = band_plane_t(pl, sxy, cell_center(first, size, mid));
    if (up ? t > pl.rhs : t < -pl.rhs) hi = mid;
    else lo = mid + 1;
  }
  *hi_out = lo;
}

}  // namespace m2s
