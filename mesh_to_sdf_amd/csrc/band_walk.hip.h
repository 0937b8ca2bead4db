// band_walk.hip.h — the walk over mask words that every band call shares: band_csg.hip, band_redistance.hip,
// band_filter.hip and band_advect.hip (through band_stencil.hip.h), band_resample.hip and band_components.hip.  A wave owns a UNIT of STEPS * 64 words and takes it in steps of 64, lane l loading word
// 64 * step + l; a word with nothing to do is settled by its own lane, the others are taken one at a time by the whole wave (a ballot finds
// them, v_readlane broadcasts the word's values) and lane t owns bit t, the point L = 64 w + t.  A word's base L is decomposed into (i, j, k)
// once, by the lane that loaded it, and stepped per bit.  A mask's word_off comes from three pieces: walk_publish (a unit's count, and by one
// atomic add the sum of its GROUP of units), a scan of the group sums (scan.hip.h's k_scan_tiles, one workgroup), then walk_unit_base and
// walk_word_off.  In an unnamed namespace, as band_handle.h's helpers are.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace m2s {
namespace {

constexpr int kWalkThreads = 256;
constexpr int kWalkWaves = kWalkThreads / 64;
constexpr int kWalkSteps = 4;                              // steps of 64 words per wave, unless a kernel names its own
constexpr uint64_t kWalkUnit = 64 * kWalkSteps;            // 256 words per wave

struct WalkGrid {
  uint64_t total, n_words;
  uint64_t nx, ny, nz;
  uint64_t sj, si;   // the strides of j and i in L: nz, ny * nz
};

// The grid of a handle or of an m2s_grid: cell_count, its product and the mask words that hold it.
WalkGrid walk_grid_of(const uint64_t cell_count[3], uint64_t total, uint64_t n_words) {
  WalkGrid g;
  g.total = total;
  g.n_words = n_words;
  g.nx = cell_count[0];
  g.ny = cell_count[1];
  g.nz = cell_count[2];
  g.sj = g.nz;
  g.si = g.ny * g.nz;
  return g;
}

struct WalkIjk {
  uint64_t i, j, k;
};

// Lane j's value in every lane, j wave-uniform (it comes out of a ballot): two v_readlane into scalar registers, no trip through the LDS
// crossbar as a shuffle would take.
__device__ __forceinline__ uint64_t walk_lane(uint64_t v, int j) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, j), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), j);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t walk_below(int t) { return (1ull << t) - 1ull; }
// The points of word w that the grid has: all 64 but in the last word.
__device__ __forceinline__ uint64_t walk_valid(uint64_t w, bool in_range, uint64_t total) {
  const uint64_t left = in_range ? total - (w << 6) : 0;
  return left >= 64 ? ~0ull : ((1ull << left) - 1ull);
}
// The list place of the active bit t of a word with mask m and offset wo, in a list of n.  It is below n whenever the index is sound; the
// guard keeps a broken invariant in bounds.
__device__ __forceinline__ uint64_t walk_rank(uint64_t m, uint64_t wo, int t, uint64_t n) {
  const uint64_t at = wo + (uint64_t)__popcll(m & walk_below(t));
  return at < n ? at : 0;
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
// The head of a kernel: this wave's unit of STEPS * 64 words of the N_WORDS there are, and of each of its steps (inside
// `for (int step = 0; step < STEPS; ++step)`): the step's first word wb, this lane's word w and whether it exists.
#define WALK_UNIT_HEAD(STEPS, N_WORDS)                                                                                              \
  const int lane = threadIdx.x & 63;                                                                                              \
  const uint64_t unit = (uint64_t)blockIdx.x * kWalkWaves + (uint64_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);             \
  const uint64_t w0 = unit * (uint64_t)(64 * (STEPS));                                                                            \
  if (w0 >= (N_WORDS)) return; /* the whole wave: the last workgroup's spare units */
#define WALK_STEP_HEAD(N_WORDS)                                                                                                     \
  const uint64_t wb = w0 + (uint64_t)step * 64; /* wave-uniform */                                                                \
  if (wb >= (N_WORDS)) break;                                                                                                     \
  const uint64_t w = wb + lane;                                                                                                   \
  const bool in_range = w < (N_WORDS);

// A unit's count of active points: the wave sum of cnt to unit_cnt[unit] (at most 64 * 64 * STEPS), and by one atomic add to the sum of its
// group of GROUP units, which the launcher zeroed.
template <int GROUP>
__device__ __forceinline__ void walk_publish(uint64_t cnt, int lane, uint64_t unit, uint32_t* unit_cnt, uint64_t* group_sum) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) {
    unit_cnt[unit] = (uint32_t)cnt;
    if (cnt) atomicAdd((unsigned long long*)(group_sum + unit / GROUP), (unsigned long long)cnt);
  }
}
// The list place of a unit's first active point: the scanned sum of its group plus the counts of the units before it in the group, one
// lane each.
template <int GROUP>
__device__ __forceinline__ uint64_t walk_unit_base(int lane, uint64_t unit, const uint32_t* unit_cnt, const uint64_t* group_base) {
  static_assert(GROUP >= 1 && GROUP <= 64, "a group's units are summed by one lane each");
  const uint64_t first = unit - unit % GROUP;   // the group's first unit: every unit from there to this one exists
  uint64_t before = first + lane < unit ? unit_cnt[first + lane] : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
  return group_base[unit / GROUP] + before;
}
// word_off of this lane's word of a step from its popcount c: the wave's exclusive scan on top of `base`, which moves on by the step's sum.
__device__ __forceinline__ uint64_t walk_word_off(uint64_t c, int lane, uint64_t& base) {
  uint64_t incl = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  const uint64_t off = base + incl - c;
  base += walk_lane(incl, 63);
  return off;
}

}  // namespace
}  // namespace m2s
