// band_walk.hip.h — the walk over a band's mask words that band_redistance.hip and band_filter.hip share: a wave
// owns a UNIT of 256 words and takes it in 4 steps of 64, lane l loading word 64 * step + l; a word with nothing to do is settled by its own
// lane, the others are taken one at a time by the whole wave (a ballot finds them, v_readlane broadcasts the word's values) and lane t owns
// bit t, the point L = 64 w + t.  A word's base L is decomposed into (i, j, k) once, by the lane that loaded it, and stepped per bit.
// Moved here from band_redistance.hip unchanged but for the names.  In an unnamed namespace, as band_handle.h's helpers are.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace m2s {
namespace {

constexpr int kWalkThreads = 256;
constexpr int kWalkWaves = kWalkThreads / 64;
constexpr int kWalkSteps = 4;                              // steps of 64 words per wave
constexpr uint64_t kWalkUnit = 64 * kWalkSteps;            // 256 words per wave

struct WalkGrid {
  uint64_t total, n_words;
  uint64_t nx, ny, nz;
  uint64_t sj, si;   // the strides of j and i in L: nz, ny * nz
};

struct WalkIjk {
  uint64_t i, j, k;
};

__device__ __forceinline__ uint64_t walk_lane(uint64_t v, int j) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, j), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), j);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t walk_below(int t) { return (1ull << t) - 1ull; }
__device__ __forceinline__ uint64_t walk_valid(uint64_t w, bool in_range, uint64_t total) {
  const uint64_t left = in_range ? total - (w << 6) : 0;
  return left >= 64 ? ~0ull : ((1ull << left) - 1ull);
}
// (i, j, k) of a word's first point: the two 64-bit divisions of a word, taken only by lanes whose word has work.
__device__ __forceinline__ WalkIjk walk_base(uint64_t L0, const WalkGrid& g) {
  WalkIjk b;
  const uint64_t row = L0 / g.nz;
  b.k = L0 - row * g.nz;
  b.i = row / g.ny;
  b.j = row - b.i * g.ny;
  return b;
}
__device__ __forceinline__ WalkIjk walk_bcast(const WalkIjk& b, int j) { return WalkIjk{walk_lane(b.i, j), walk_lane(b.j, j), walk_lane(b.k, j)}; }
// The base stepped by t < 64 points.  The branches are wave-uniform: with 64 or more points per row a step crosses one row end at most.
__device__ __forceinline__ WalkIjk walk_step(const WalkIjk& b, uint32_t t, const WalkGrid& g) {
  WalkIjk p;
  uint64_t kk = b.k + t, q;
  if (g.nz >= 64) {
    q = kk >= g.nz ? 1 : 0;
    kk -= q ? g.nz : 0;
  } else {
    const uint32_t q32 = (uint32_t)kk / (uint32_t)g.nz;   // kk < nz + 64 < 128
    q = q32;
    kk -= (uint64_t)q32 * g.nz;
  }
  uint64_t jj = b.j + q, q2;   // q <= 63
  if (g.ny >= 64) {
    q2 = jj >= g.ny ? 1 : 0;
    jj -= q2 ? g.ny : 0;
  } else {
    const uint32_t q32 = (uint32_t)jj / (uint32_t)g.ny;   // jj < ny + 64 < 128
    q2 = q32;
    jj -= (uint64_t)q32 * g.ny;
  }
  p.k = kk;
  p.j = jj;
  p.i = b.i + q2;
  return p;
}
#define WALK_UNIT_HEAD                                                                                                              \
  const int lane = threadIdx.x & 63;                                                                                              \
  const uint64_t unit = (uint64_t)blockIdx.x * kWalkWaves + (uint64_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);             \
  const uint64_t w0 = unit * kWalkUnit;                                                                                             \
  if (w0 >= g.n_words) return; /* the whole wave: the last workgroup's spare units */
#define WALK_STEP_HEAD                                                                                                              \
  const uint64_t wb = w0 + (uint64_t)step * 64; /* wave-uniform */                                                                \
  if (wb >= g.n_words) break;                                                                                                     \
  const uint64_t w = wb + lane;                                                                                                   \
  const bool in_range = w < g.n_words;

}  // namespace
}  // namespace m2s
