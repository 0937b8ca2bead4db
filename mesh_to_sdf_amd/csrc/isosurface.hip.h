// isosurface.hip.h — what the two marching-cubes extractors share: isosurface.hip (m2s_grid_isosurface, a dense grid) and
// band_isosurface.hip (m2s_band_isosurface, a narrow band).  Moved here from isosurface.hip unchanged: the table, the grid
// description, the point decode and the rank of an active point from the mask; the workgroup scan and the scan of block sums
// (k_scan_tiles<kScanThreads, uint64_t>) come from scan.hip.h.
// band_query.hip (m2s_band_create) builds the same index of a band as band_isosurface.hip: k_biso_mask and its flags are here for both.
// Everything is in an unnamed namespace: each translation unit that includes this has its own copy (of the __constant__ table too).
#pragma once
#include "../../include/m2s.h"
#include "common.h"
#include "scan.hip.h"

#define M2S_ISO_TABLE static __constant__ const
#include "isosurface_table.h"

namespace m2s {
namespace {

constexpr int kScanThreads = 1024;   // the one workgroup that scans block sums
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
