// cut_size.hip.h — the size test of k_cut's emit decision (cut.hip): a node is small enough for a brick's list when
// fmaxf(R, half) <= emit_radius.  R and half come from the node record and are the same in every lane, so their maximum is formed once
// per visit on the scalar unit and the lanes pay one compare.  (Written as fmaxf the two wave-uniform operands cost three v_max_f32 per
// visit: one to quiet each operand, one for the maximum.)  Host and device: tests/test_cut_size_cpu.py checks the decision against
// fmaxf(R, half) <= e for every class of bit pattern through the CPU probe library.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace m2s {

// A value m with  (m <= e) == (fmaxf(R, half) <= e)  for every e.  Two floats that are neither negative nor NaN — sign bit clear, bits
// <= +inf's — order as their bit patterns do (+0, denormals and +inf included), and that is every radius and half width a finite mesh
// produces.  Anything else (a negative value, -0, a NaN of either sign) takes fmaxf itself: it drops a NaN operand and returns NaN only for
// two, and NaN <= e is false.
__host__ __device__ __forceinline__ float cut_extent(float R, float half) {
  const uint32_t a = __builtin_bit_cast(uint32_t, R), b = __builtin_bit_cast(uint32_t, half);
  uint32_t m = a > b ? a : b;
  if (__builtin_expect(m > 0x7f800000u, 0)) {
#if defined(__HIP_DEVICE_COMPILE__)
    // (the kernel's operands are wave-uniform: the result stays in a scalar register on this path too)
    m = (uint32_t)__builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, fmaxf(R, half)));
#else
    m = __builtin_bit_cast(uint32_t, fmaxf(R, half));
#endif
  }
  return __builtin_bit_cast(float, m);
}
__host__ __device__ __forceinline__ bool cut_small_enough(float R, float half, float emit_radius) { return cut_extent(R, half) <= emit_radius; }

}  // namespace m2s
