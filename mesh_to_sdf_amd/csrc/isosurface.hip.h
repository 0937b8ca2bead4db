// isosurface.hip.h — what the two marching-cubes extractors share: isosurface.hip (m2s_grid_isosurface, a dense grid) and
// band_isosurface.hip (m2s_band_isosurface, a narrow band).  Moved here from isosurface.hip unchanged: the table, the grid
// description, the workgroup scan, the point decode, the scan of block sums and the rank of an active point from the mask.
// band_query.hip (m2s_band_create) builds the same index of a band as band_isosurface.hip: k_biso_mask and its flags are here for both.
// Everything is in an unnamed namespace: each translation unit that includes this has its own copy (of the __constant__ table too).
#pragma once
#include "../../include/m2s.h"
#include "common.h"

#define M2S_ISO_TABLE static __constant__ const
#include "isosurface_table.h"

namespace m2s {
namespace {

constexpr int kScanThreads = 1024;
constexpr int kItemThreads = 256;
constexpr int kItemsPerThread = 16;
constexpr int kItemBlock = kItemThreads * kItemsPerThread;   // active points per k_iso_info / vertices / triangles workgroup

struct IsoGrid {
  float first[3], cs[3];
  uint64_t n[3];
  uint64_t nyz;     // n[1] * n[2]
  uint64_t total;   // n[0] * n[1] * n[2]
  float iso;
};

// Exclusive scan over a workgroup of NT threads (64-wide waves); *total = the sum of all.
template <int NT>
__device__ __forceinline__ uint64_t block_exclusive_scan(uint64_t v, uint64_t* total) {
  __shared__ uint64_t wave_sum[NT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wave_sum[wave] = x;
  __syncthreads();
  uint64_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const uint64_t s = wave_sum[w];
    if (w < wave) before += s;
    all += s;
  }
  __syncthreads();   // wave_sum may be reused by the caller's next scan
  *total = all;
  return before + x - v;
}

struct Pt {
  uint64_t i, j, k;
};

__device__ __forceinline__ Pt decode(const IsoGrid& g, uint64_t L) {
  Pt p;
  p.i = L / g.nyz;
  const uint64_t r = L - p.i * g.nyz;
  p.j = r / g.n[2];
  p.k = r - p.j * g.n[2];
  return p;
}

// In-place exclusive scan of n counts in one workgroup; *total = their sum.
__global__ void __launch_bounds__(kScanThreads) k_scan_tiles(uint64_t* __restrict__ v, uint64_t n, uint64_t* __restrict__ total) {
  const uint64_t chunk = (n + kScanThreads - 1) / kScanThreads;
  const uint64_t b = threadIdx.x * chunk, e = b + chunk < n ? b + chunk : n;
  uint64_t s = 0;
  for (uint64_t i = b; i < e; ++i) s += v[i];
  uint64_t all;
  uint64_t run = block_exclusive_scan<kScanThreads>(s, &all);
  for (uint64_t i = b; i < e; ++i) {
    const uint64_t x = v[i];
    v[i] = run;
    run += x;
  }
  if (threadIdx.x == 0) *total = all;
}

// The index of active point L in the active list: its mask word's offset plus the active points before it in that word.
__device__ __forceinline__ uint64_t active_index(const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_off, uint64_t L) {
  const uint64_t w = L >> 6;
  const uint64_t below = mask[w] & ((1ull << (L & 63)) - 1);
  return word_off[w] + (uint64_t)__popcll(below);
}

// ---- the index of a band: shared by band_isosurface.hip and band_query.hip ----
// k_biso_mask, per band cell: strictly ascending and below the cell count (else flag bit 0), a finite value (else flag bit 1), its bit
// in the zeroed mask, and, from the first cell of each word, word_off[w] = its place in the list.  With active_index above, a grid
// point's place in the ascending list is two loads.
constexpr int kMaskThreads = 256;
constexpr uint64_t kNone = ~0ull;
constexpr uint32_t kFlagOrder = 1u, kFlagNonFinite = 2u;

__global__ void __launch_bounds__(kMaskThreads) k_biso_mask(uint64_t total, const uint64_t* __restrict__ cells, const float* __restrict__ dist,
                                                            uint64_t n, uint64_t* __restrict__ mask, uint64_t* __restrict__ word_off,
                                                            uint32_t* __restrict__ flag) {
  const uint64_t a = (uint64_t)blockIdx.x * kMaskThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  uint64_t w = kNone, acc = 0;   // no word: lanes past the end and cells past the grid
  uint32_t bad = 0;
  bool first = false;
  if (a < n) {
    const uint64_t L = cells[a];
    const uint64_t prev = a ? cells[a - 1] : 0;
    if (L >= total || (a && prev >= L)) bad |= kFlagOrder;
    if (!isfinite(dist[a])) bad |= kFlagNonFinite;
    if (L < total) {
      w = L >> 6;
      acc = 1ull << (L & 63);
      first = a == 0 || (prev >> 6) != w;
    }
  }
  if (first) word_off[w] = a;
  // a word has 64 points and the list ascends: the lanes of one word are a run of at most 64 neighbours
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t ow = __shfl_down(w, o, 64);
    const uint64_t oa = __shfl_down(acc, o, 64);
    if (lane + o < 64 && ow == w) acc |= oa;
  }
  const uint64_t pw = __shfl_up(w, 1, 64);
  if (w != kNone && (lane == 0 || pw != w)) atomicOr((unsigned long long*)(mask + w), (unsigned long long)acc);
  const uint32_t any = (__ballot(bad & kFlagOrder) ? kFlagOrder : 0u) | (__ballot(bad & kFlagNonFinite) ? kFlagNonFinite : 0u);
  if (any && lane == 0) atomicOr(flag, any);
}

unsigned item_blocks(uint64_t n_act) { return (unsigned)((n_act + kItemBlock - 1) / kItemBlock); }

}  // namespace
}  // namespace m2s
