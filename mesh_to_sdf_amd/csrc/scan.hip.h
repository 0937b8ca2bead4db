// scan.hip.h — the two-level exclusive scan that voxelize.hip, band.hip, sample.hip and the isosurface units share:
// one sum per tile, the tile sums scanned in place by one workgroup, then each tile again with its offset.
// Everything is in an unnamed namespace: each translation unit that includes this has its own copy of the kernels it launches.
#pragma once
#include "common.h"

namespace m2s {
namespace {

constexpr int kTileThreads = 256;                        // the workgroup of every kernel that walks a tile
constexpr int kScanItems = 16;                           // consecutive items per thread
constexpr int kScanTile = kTileThreads * kScanItems;     // items per tile
static_assert(kScanTile == MASK_SCAN_TILE, "k_band_emit and k_emit_cells read launch_voxel_count's offsets by common.h's tile");

inline uint32_t tiles_of(size_t n) { return (uint32_t)((n + kScanTile - 1) / kScanTile); }

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

// In-place exclusive scan of n sums by the one workgroup of NT threads that calls it, `chunk` consecutive sums per thread; *total = their
// sum, in every thread.  Count is the type of n and of the index arithmetic.  The copies this replaces clamped b for a 32-bit count and
// not for a 64-bit one; a thread past the end has an empty range either way, and each form is kept so that each kernel's instructions
// stay what they were (as for the total handed back through a pointer).
template <int NT, typename Count>
__device__ __forceinline__ void scan_tiles_in_place(uint64_t* v, Count n, uint64_t* total) {
  const Count chunk = (n + NT - 1) / NT;
  Count b = threadIdx.x * chunk;
  if constexpr (sizeof(Count) == 4) b = min(b, n);
  const Count e = min(b + chunk, n);
  uint64_t s = 0;
  for (Count i = b; i < e; ++i) s += v[i];
  uint64_t run = block_exclusive_scan<NT>(s, total);
  for (Count i = b; i < e; ++i) {
    const uint64_t x = v[i];
    v[i] = run;
    run += x;
  }
}

template <int NT, typename Count>
__global__ __launch_bounds__(NT) void k_scan_tiles(uint64_t* __restrict__ v, Count n, uint64_t* __restrict__ total) {
  uint64_t all;
  scan_tiles_in_place<NT, Count>(v, n, &all);
  if (threadIdx.x == 0) *total = all;
}

// What a tile adds up: uint64 counts, or the set bits of mask words.
template <bool POPC>
__device__ __forceinline__ uint64_t scan_item(const void* __restrict__ src, size_t i) {
  return POPC ? (uint64_t)__popc(static_cast<const uint32_t*>(src)[i]) : static_cast<const uint64_t*>(src)[i];
}
// The items of one tile, kScanItems consecutive ones per thread; returns their sum.
template <bool POPC>
__device__ __forceinline__ uint64_t tile_items(const void* __restrict__ src, size_t n, uint64_t (&w)[kScanItems]) {
  const size_t first = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanItems;
  uint64_t s = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    w[k] = first + k < n ? scan_item<POPC>(src, first + k) : 0;
    s += w[k];
  }
  return s;
}

template <bool POPC>
__global__ __launch_bounds__(kTileThreads) void k_tile_sums(const void* __restrict__ src, size_t n, uint64_t* __restrict__ tile_sum) {
  uint64_t w[kScanItems], all;
  const uint64_t s = tile_items<POPC>(src, n, w);
  (void)block_exclusive_scan<kTileThreads>(s, &all);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
}

// S[t] = cols[0] + ... + cols[t - 1];  S[n] is written by the thread that holds the last triangle.
// (A template so that only the units that launch it hold it: a plain __global__ here would be emitted in every unit that includes this.)
template <typename Count>
__global__ __launch_bounds__(kTileThreads) void k_col_scan(const uint64_t* __restrict__ cols, Count n, const uint64_t* __restrict__ tile_off,
                                                           uint64_t* __restrict__ S) {
  uint64_t w[kScanItems], all;
  const uint64_t s = tile_items<false>(cols, n, w);
  uint64_t run = tile_off[blockIdx.x] + block_exclusive_scan<kTileThreads>(s, &all);
  const size_t first = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanItems;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (first + k < n) S[first + k] = run;
    run += w[k];
    if (first + k + 1 == n) S[n] = run;
  }
}

}  // namespace
}  // namespace m2s
