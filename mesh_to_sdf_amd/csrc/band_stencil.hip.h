// band_stencil.hip.h — what the calls that step the values of a resident band between two value buffers share (band_filter.hip,
// band_advect.hip), gfx950: the table of each active cell's clamped neighbour places, and the kernel that turns the last buffer into the
// result.  Both walk the mask words with band_walk.hip.h's walk, units of 256 words.
//   bf_slot      the place of a grid point in the value buffers: its rank in the list, or one of the two background places behind it.
//   k_bf_table   per active cell, once: its 6 or 18 neighbour places as 32-bit slots, a byte, its value into the first value buffer.
//   k_bf_final   the result's sign words (a ballot per mask word), its values, n_changed, n_sign_flips and max_change.
// The kernels are in an unnamed namespace, as band_handle.h's helpers are: each translation unit that includes this has its own copy.
// It holds floating-point arithmetic whose bits are part of the contract: the including unit sets `#pragma clang fp contract(off)` first.
#pragma once
#include "band_handle.h"
#include "band_walk.hip.h"

#pragma clang fp contract(off)

namespace m2s {
namespace {

constexpr int kBfAxisSlots = 6, kBfAllSlots = 18;

// The place in the value buffers of the grid point M (inside the grid): its rank in X's list if it is active, else n (outside) or n + 1
// (its inside bit is set).  Always below n + 2.
__device__ __forceinline__ uint32_t bf_slot(const BandDev& X, uint64_t M) {
  const uint64_t w = M >> 6;
  const int b = (int)(M & 63);
  const uint64_t m = X.mask[w];
  if ((m >> b) & 1ull) {
    const uint64_t r = X.word_off[w] + (uint64_t)__popcll(m & walk_below(b));
    return (uint32_t)(r < X.n ? r : X.n);   // r < n whenever the index is sound
  }
  const uint64_t in = X.inside ? (X.inside[w] >> b) & 1ull : 0ull;
  return (uint32_t)(X.n + in);
}

// Per active cell r, once: slots[s * n + r], s = 0 .. NSLOT - 1 in the order i+, i-, j+, j-, k+, k-, then for ab = ij, ik, jk the four
// diagonals +a+b, +a-b, -a+b, -a-b; in_region[r]; v0[r] = x.  A clamped step is a step of 0, so a clamped neighbour is the clamped point.
// The first lane of the grid also fills the two background places of both value buffers.
template <int NSLOT>
__global__ void __launch_bounds__(kWalkThreads) k_bf_table(BandDev X, BandDev Wh, int has_where, WalkGrid g, uint32_t* __restrict__ slots,
                                                         uint8_t* __restrict__ in_region, float* __restrict__ v0, float* __restrict__ v1) {
  WALK_UNIT_HEAD(kWalkSteps, g.n_words)
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    v0[X.n] = X.bg_out;
    v0[X.n + 1] = X.bg_in_neg;
    v1[X.n] = X.bg_out;
    v1[X.n + 1] = X.bg_in_neg;
  }
  for (int step = 0; step < kWalkSteps; ++step) {
    WALK_STEP_HEAD(g.n_words)
    const uint64_t m = in_range ? X.mask[w] : 0;
    const uint64_t wo = m ? X.word_off[w] : 0;
    const uint64_t wm = (m && has_where) ? Wh.mask[w] : 0;
    const uint64_t win = (m && has_where && Wh.inside) ? Wh.inside[w] : 0;
    const uint64_t wwo = wm ? Wh.word_off[w] : 0;
    WalkIjk base{0, 0, 0};
    if (m) base = walk_base(w << 6, g);
    uint64_t todo = __ballot(m != 0);
    while (todo) {   // wave-uniform
      const int j = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const uint64_t mj = walk_lane(m, j), woj = walk_lane(wo, j), wmj = walk_lane(wm, j), winj = walk_lane(win, j), wwoj = walk_lane(wwo, j);
      const WalkIjk p = walk_step(walk_bcast(base, j), (uint32_t)lane, g);
      const uint64_t L = ((wb + (uint64_t)j) << 6) + (uint64_t)lane;
      const uint64_t r = woj + (uint64_t)__popcll(mj & walk_below(lane));
      if (((mj >> lane) & 1ull) && r < X.n) {   // an active point is inside the grid
        const int64_t d[3][2] = {{p.i + 1 < g.nx ? (int64_t)g.si : 0, p.i > 0 ? -(int64_t)g.si : 0},
                                 {p.j + 1 < g.ny ? (int64_t)g.sj : 0, p.j > 0 ? -(int64_t)g.sj : 0},
                                 {p.k + 1 < g.nz ? (int64_t)1 : 0, p.k > 0 ? (int64_t)-1 : 0}};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          slots[(uint64_t)(2 * a) * X.n + r] = bf_slot(X, (uint64_t)((int64_t)L + d[a][0]));
          slots[(uint64_t)(2 * a + 1) * X.n + r] = bf_slot(X, (uint64_t)((int64_t)L + d[a][1]));
        }
        if (NSLOT == kBfAllSlots) {
          int s = kBfAxisSlots;
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = a + 1; b < 3; ++b)
#pragma unroll
              for (int sa = 0; sa < 2; ++sa)
#pragma unroll
                for (int sb = 0; sb < 2; ++sb) slots[(uint64_t)(s++) * X.n + r] = bf_slot(X, (uint64_t)((int64_t)L + d[a][sa] + d[b][sb]));
        }
        bool in = true;
        if (has_where) {
          in = (winj >> lane) & 1ull;
          if ((wmj >> lane) & 1ull) {
            in = Wh.dist[walk_rank(wmj, wwoj, lane, Wh.n)] < 0.0f;
          }
        }
        in_region[r] = in ? 1 : 0;
        v0[r] = X.dist[r];
      }
    }
  }
}

__device__ __forceinline__ bool bf_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// The result: S = act ? (r < 0) : inside bit on every grid point (bits past the grid zero), out[r] = the last pass's values, and
// counters[1] += n_changed, counters[2] += n_sign_flips, counters[3] = max(the bits of fabsf(r - x)): non-negative floats order as their bits.
__global__ void __launch_bounds__(kWalkThreads) k_bf_final(BandDev X, WalkGrid g, const float* __restrict__ v, uint64_t* __restrict__ S, float* __restrict__ out,
                                                         uint64_t* __restrict__ counters) {
  WALK_UNIT_HEAD(kWalkSteps, g.n_words)
  uint32_t n_changed = 0, n_flips = 0, top = 0;
  for (int step = 0; step < kWalkSteps; ++step) {
    WALK_STEP_HEAD(g.n_words)
    const uint64_t m = in_range ? X.mask[w] : 0;
    const uint64_t in = in_range && X.inside ? X.inside[w] : 0;
    const uint64_t wo = m ? X.word_off[w] : 0;
    const uint64_t valid = walk_valid(w, in_range, g.total);
    uint64_t s = in & valid;
    uint64_t todo = __ballot(m != 0);
    while (todo) {   // wave-uniform
      const int j = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const uint64_t mj = walk_lane(m, j), inj = walk_lane(in, j), woj = walk_lane(wo, j);
      const uint64_t r = woj + (uint64_t)__popcll(mj & walk_below(lane));
      bool sb = (inj >> lane) & 1ull;
      if (((mj >> lane) & 1ull) && r < X.n) {
        const float x = X.dist[r], y = v[r];
        out[r] = y;
        sb = y < 0.0f;
        n_changed += __float_as_uint(x) != __float_as_uint(y) ? 1u : 0u;
        n_flips += sb != (x < 0.0f) ? 1u : 0u;
        const uint32_t ch = __float_as_uint(fabsf(y - x));   // finite operands: a number or +inf, never a NaN
        top = ch > top ? ch : top;
      }
      const uint64_t sm = __ballot(sb);
      if (lane == j) s = sm & valid;
    }
    if (in_range) S[w] = s;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n_changed += __shfl_xor(n_changed, o, 64);
    n_flips += __shfl_xor(n_flips, o, 64);
    const uint32_t other = __shfl_xor(top, o, 64);
    top = other > top ? other : top;
  }
  if (lane == 0) {
    if (n_changed) atomicAdd((unsigned long long*)(counters + 1), (unsigned long long)n_changed);
    if (n_flips) atomicAdd((unsigned long long*)(counters + 2), (unsigned long long)n_flips);
    if (top) atomicMax((unsigned int*)(counters + 3), top);
  }
}

}  // namespace
}  // namespace m2s
