// ray.hip.h — the watertight ray / triangle test of Woop, Benthin and Wald (2013) as include/m2s.h states it for m2s_cast_rays:
// IEEE binary32, no FMA, sums left to right, correctly rounded divisions, zeros of the edge functions inside, no culling and no
// f64 fallback — and, beyond the paper, two bounding clauses (RAY_XY_REL, RAY_Z_REL below) that make the test one a tree can prune for
// exactly.  Host-compilable like geo.hip.h (geo_probe.hip builds it for the CPU tests); tests/ray_model.py is its numpy twin.
#pragma once
#include "geo.hip.h"

#pragma clang fp contract(off)

namespace m2s {

// The two bounding clauses of the definition.  Without an f64 fallback, the edge functions of a triangle seen edge-on (the ray in its
// plane, or a sliver below the resolution of its coordinates) are rounding noise, and the bare test reports hits although the ray's axis
// passes far outside the triangle's three sheared points; with underflowing products t can likewise leave the points' depth range.  No
// box can bound such a hit, so the definition itself excludes it, in f32 operations a box test can mirror (rays.hip ray_box_accept):
//   XY  miss unless the axis (0, 0) lies in the rectangle of (Ax, Ay), (Bx, By), (Cx, Cy) widened by fl(2^-20 * the largest |coordinate|);
//   Z   miss unless fl(zmin - mz) <= t <= fl(zmax + mz), zmin / zmax over Az, Bz, Cz and mz = fl(2^-21 * the largest |Az|, |Bz|, |Cz|).
// Neither fires on a triangle whose image is not degenerate and whose products do not underflow (the bounds are derived in rays.hip):
// there the clauses change no bit.
constexpr float RAY_XY_REL = 9.5367431640625e-07f;    // 2^-20
constexpr float RAY_Z_REL = 4.76837158203125e-07f;    // 2^-21

// What a ray contributes to every triangle test: the dominant axis kz of d, the other two in an order that keeps the winding
// (swapped when d[kz] < 0), and the shear that maps d onto (0, 0, 1).  |Sx|, |Sy| <= 1.
struct RaySetup {
  int kx, ky, kz;
  float Sx, Sy, Sz;
  bool valid;   // false: a non-finite component in o or d, or d == (0, 0, 0) — such a ray hits nothing
};

M2S_HD float axis3(f3 v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

M2S_HD RaySetup ray_setup(f3 o, f3 d) {
  RaySetup r;
  const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
  int kz = 0;
  float am = ax;
  if (ay > am) { kz = 1; am = ay; }   // the lowest index on ties
  if (az > am) { kz = 2; am = az; }
  int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
  const float dz = axis3(d, kz);
  if (dz < 0.0f) { const int s = kx; kx = ky; ky = s; }
  r.kx = kx; r.ky = ky; r.kz = kz;
  r.Sx = axis3(d, kx) / dz;
  r.Sy = axis3(d, ky) / dz;
  r.Sz = 1.0f / dz;
  const float inf = __builtin_inff();
  // (a NaN fails every comparison, am == 0 is the zero direction; am is the largest |d_k|, so it alone bounds d)
  r.valid = fabsf(o.x) < inf && fabsf(o.y) < inf && fabsf(o.z) < inf && ax < inf && ay < inf && az < inf && am > 0.0f;
  return r;
}

// One triangle (a, b, c): true iff the ray's line meets it (edge functions of one sign or zero, det != 0, both bounding clauses); then
// (and only then) *t is the ray parameter and (*u, *v) the barycentric weights of b and c.  The caller applies the range
// t_min <= t <= t_max.
M2S_HD bool ray_triangle(const RaySetup& r, f3 o, f3 a, f3 b, f3 c, float* t, float* u, float* v) {
  const f3 A = sub3(a, o), B = sub3(b, o), C = sub3(c, o);
  const float Akz = axis3(A, r.kz), Bkz = axis3(B, r.kz), Ckz = axis3(C, r.kz);
  const float Ax = axis3(A, r.kx) - r.Sx * Akz, Ay = axis3(A, r.ky) - r.Sy * Akz;
  const float Bx = axis3(B, r.kx) - r.Sx * Bkz, By = axis3(B, r.ky) - r.Sy * Bkz;
  const float Cx = axis3(C, r.kx) - r.Sx * Ckz, Cy = axis3(C, r.ky) - r.Sy * Ckz;
  const float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
  const bool neg = U < 0.0f || V < 0.0f || W < 0.0f, pos = U > 0.0f || V > 0.0f || W > 0.0f;
  const float det = U + V + W;
  if ((neg && pos) || !(det < 0.0f || det > 0.0f)) return false;   // det == 0 or NaN: a miss
  // (the clauses come after the edge test, which few triangles pass; every comparison is written so that a NaN excludes nothing)
  const float xl = fminf(fminf(Ax, Bx), Cx), xh = fmaxf(fmaxf(Ax, Bx), Cx), yl = fminf(fminf(Ay, By), Cy), yh = fmaxf(fmaxf(Ay, By), Cy);
  const float mxy = RAY_XY_REL * fmaxf(fmaxf(fabsf(xl), fabsf(xh)), fmaxf(fabsf(yl), fabsf(yh)));
  if (xl > mxy || xh < -mxy || yl > mxy || yh < -mxy) return false;
  const float Az = r.Sz * Akz, Bz = r.Sz * Bkz, Cz = r.Sz * Ckz;
  const float zl = fminf(fminf(Az, Bz), Cz), zh = fmaxf(fmaxf(Az, Bz), Cz), mz = RAY_Z_REL * fmaxf(fabsf(zl), fabsf(zh));
  *t = (U * Az + V * Bz + W * Cz) / det;
  if (*t < zl - mz || *t > zh + mz) return false;
  *u = V / det;
  *v = W / det;
  return true;
}

M2S_HD bool ray_triangle_in_range(const RaySetup& r, f3 o, f3 a, f3 b, f3 c, float t_min, float t_max, float* t, float* u, float* v) {
  return ray_triangle(r, o, a, b, c, t, u, v) && *t >= t_min && *t <= t_max;   // a NaN t (0 * inf in the numerator) is no hit
}

}  // namespace m2s
