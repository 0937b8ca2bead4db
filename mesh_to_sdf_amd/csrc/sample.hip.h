// sample.hip.h — the arithmetic of area-weighted surface sampling as include/m2s.h states it for m2s_sample_surface: a counter-based
// generator (Philox4x32-10), triangle weights that are INTEGERS (so their running sums do not depend on the order a scan adds them in),
// the pick by the high half of a 64 x 64-bit product, and the point, its barycentric weights and the unit normal in IEEE binary32, no
// FMA, sums left to right.  Host-compilable like geo.hip.h and ray.hip.h (geo_probe.hip builds it for the CPU tests);
// tests/sample_model.py is its numpy twin.
#pragma once
#include <string.h>

#include "geo.hip.h"

#pragma clang fp contract(off)

namespace m2s {

M2S_HD uint32_t sample_f32_bits(float f) {
#ifdef __HIP_DEVICE_COMPILE__
  return __float_as_uint(f);
#else
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
#endif
}
M2S_HD double sample_f64_from_bits(uint64_t b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __longlong_as_double((long long)b);
#else
  double d;
  memcpy(&d, &b, 8);
  return d;
#endif
}
M2S_HD uint64_t sample_mulhi64(uint64_t a, uint64_t b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011): ten rounds of two 32 x 32 -> 64-bit products, the key bumped between rounds.
struct Philox4 {
  uint32_t r[4];
};
M2S_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return {{c0, c1, c2, c3}};
}
// The four words of global sample g under `seed`: counter (g lo, g hi, 0, 0), key (seed lo, seed hi).
M2S_HD Philox4 sample_random(uint64_t seed, uint64_t g) {
  return philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// Raw normal n = (b - a) x (c - a) and A_t = |n| = twice the triangle's area; a non-finite A_t (NaN or overflow) counts as 0.
M2S_HD float tri_weight_area(f3 a, f3 b, f3 c, f3* n) {
  *n = cross3(sub3(b, a), sub3(c, a));
  const float A = sqrtf((n->x * n->x + n->y * n->y) + n->z * n->z);
  return A < __builtin_inff() ? A : 0.0f;   // (a NaN fails the comparison)
}

// e = floor(log2(Amax)) of a positive finite f32, subnormals included.
M2S_HD int sample_exponent(float amax) {
  const uint32_t b = sample_f32_bits(amax), E = (b >> 23) & 0xffu, m = b & 0x7fffffu;
  if (E) return (int)E - 127;
  int top = 22;
  while (top > 0 && !((m >> top) & 1u)) --top;
  return top - 149;
}

// w_t = floor((double)A_t * 2^(37 - e)) < 2^38: the product with a power of two is exact, so the only rounding is the floor.
M2S_HD uint64_t sample_weight(float A, int e) {
  const double scale = sample_f64_from_bits((uint64_t)(37 - e + 1023) << 52);   // 37 - e in [-90, 186]: a normal double
  return (uint64_t)((double)A * scale);
}

// T = floor(x * W / 2^64) with x = r0 | r1 << 32: uniform over [0, W) up to 2^-64 W.
M2S_HD uint64_t sample_target(uint32_t r0, uint32_t r1, uint64_t W) { return sample_mulhi64((uint64_t)r0 | ((uint64_t)r1 << 32), W); }

// The smallest index in [lo, hi) whose C exceeds T (hi when none does): upper_bound, so a triangle of weight 0 is never the answer.
M2S_HD uint64_t sample_upper_bound(const uint64_t* C, uint64_t lo, uint64_t hi, uint64_t T) {
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (C[mid] > T) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// u' = (r >> 9) 2^-23 + 2^-24: exact in f32, strictly inside (0, 1), and so is 1 - u'.
M2S_HD float sample_unit(uint32_t r) { return (float)(r >> 9) * 1.1920928955078125e-07f + 5.9604644775390625e-08f; }

// The fold of the unit square onto the triangle u + v <= 1: the weights of b and c.
M2S_HD void sample_fold(uint32_t r2, uint32_t r3, float* u, float* v) {
  const float up = sample_unit(r2), vp = sample_unit(r3);
  const bool flip = up + vp > 1.0f;
  *u = flip ? 1.0f - up : up;
  *v = flip ? 1.0f - vp : vp;
}

M2S_HD f3 sample_point(f3 a, f3 b, f3 c, float u, float v) {
  return mk3((a.x + u * (b.x - a.x)) + v * (c.x - a.x), (a.y + u * (b.y - a.y)) + v * (c.y - a.y), (a.z + u * (b.z - a.z)) + v * (c.z - a.z));
}

// The unit right-hand normal of a triangle the sampler can reach (A > 0 and finite).
M2S_HD f3 sample_normal(f3 n, float A) { return mk3(n.x / A, n.y / A, n.z / A); }

}  // namespace m2s
