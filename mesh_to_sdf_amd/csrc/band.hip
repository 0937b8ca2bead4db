// band.hip — narrow-band grid SDFs (m2s_narrow_band_sdf, m2s_mesh_narrow_band_sdf), gfx950.  DESIGN.md §4.13.
//
// The contract is include/m2s.h's: the dense grid result filtered to -interior <= D <= exterior.  Nothing here computes a distance: the
// exact minimum comes from launch_query_distance (bit-identical to the grid walks) and the Raycast sign from sign.hip's majority plane.
//   k_band_count    per triangle: the box of its finite vertices, its reach (band.hip.h) and the three intervals of cells whose axis gap is
//                   within reach (band_interval: binary searches on the predicate itself); the number of (i, j) columns in them.
//   the scan        exclusive running sums of the column counts in uint64 (scan.hip.h, as in voxelize.hip).
//   k_band_raster   one column per lane, grid-stride over the device-resident total.  A lane finds its triangle by a binary search in the
//                   sums, drops the column if its x and y gaps alone are out of reach, tightens the z interval by what they have spent
//                   (band_interval again) and by the distance to the triangle's plane (band_plane_interval), and sets that run of bits: one atomicOr per touched word.
//   k_band_fill     r = +inf: every cell is a candidate.
//   k_band_emit     candidates of rank [begin, end) in ascending L, from the per-tile offsets of launch_voxel_count: their L and centres
//                   (cell_center: the dense walk's own expression).  Tiles outside the range leave at once.
//   k_band_filter   per candidate: the plane bit applied (Raycast), -interior <= d <= exterior, the active bit, a flag.
//   compaction      k_band_flag_sums + k_scan_tiles + k_band_compact: flagged cells and distances to a running offset kept on the device,
//                   stable, so ascending chunks give ascending output.
//   algorithm 1     k_band_dense_mask (one mask word per lane over the dense grid) and k_band_gather.
#include <algorithm>

#include "common.h"
#include "geo.hip.h"
#include "scan.hip.h"
#include "band.hip.h"

namespace m2s {

namespace {

__global__ void k_warm_band() {}

constexpr int kThreads = kTileThreads;
constexpr unsigned kRasterBlocks = 4096;

__device__ __forceinline__ BandBox load_band_box(const TriRec* __restrict__ tris, uint32_t t) {
  const TriRec& r = tris[t];
  return band_box(mk3(r.ax, r.ay, r.az), mk3(r.bx, r.by, r.bz), mk3(r.cx, r.cy, r.cz));
}
__device__ __forceinline__ float reach_of(const BandBox& bx, float r, float grid_scale) {
  return band_reach(r, bx.amax > grid_scale ? bx.amax : grid_scale);
}

// iv[6 t ..]: x lo, x hi, y lo, y hi, z lo, z hi.
__global__ __launch_bounds__(kThreads) void k_band_count(const TriRec* __restrict__ tris, uint32_t n_tris, GridParams g, float r, float grid_scale,
                                                         uint32_t* __restrict__ iv, uint64_t* __restrict__ cols) {
  const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= n_tris) return;
  const BandBox bx = load_band_box(tris, t);
  const float reach = reach_of(bx, r, grid_scale), reach2 = reach * reach;
  uint32_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  bool any = bx.any;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    if (any) band_interval(bx.lo[m], bx.hi[m], g.first[m], g.size[m], 0u, g.n[m], 0.0f, 0.0f, reach2, &lo[m], &hi[m]);
    any = any && lo[m] < hi[m];
  }
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    iv[6 * (size_t)t + 2 * m] = lo[m];
    iv[6 * (size_t)t + 2 * m + 1] = hi[m];
  }
  cols[t] = any ? (uint64_t)(hi[0] - lo[0]) * (uint64_t)(hi[1] - lo[1]) : 0;   // < 2^32: a grid face has fewer lines (fill_grid_params)
}

// What bounds this kernel is what bounds k_vox_raster: the binary search in S, the record gather and the scattered
// atomics — one per touched word here, and a column of a band a few cells wide touches one or two.
__global__ __launch_bounds__(kThreads) void k_band_raster(const TriRec* __restrict__ tris, uint32_t n_tris, GridParams g, float r, float grid_scale,
                                                          const uint32_t* __restrict__ iv, const uint64_t* __restrict__ S,
                                                          uint32_t* __restrict__ bits) {
  const uint64_t total = S[n_tris];
  for (uint64_t w = (uint64_t)blockIdx.x * kThreads + threadIdx.x; w < total; w += (uint64_t)gridDim.x * kThreads) {
    // the triangle of column w: the smallest t with S[t + 1] > w
    uint32_t lo = 0, hi = n_tris - 1;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (S[mid + 1] > w) hi = mid;
      else lo = mid + 1;
    }
    const uint32_t t = lo;
    const uint32_t* v = iv + 6 * (size_t)t;
    const uint32_t xlo = v[0], ylo = v[2], yhi = v[3], zlo = v[4], zhi = min(v[5], g.n[2]);
    const uint32_t rows = yhi - ylo;
    const uint64_t local = w - S[t];
    if (rows == 0 || local >= (uint64_t)(v[1] - xlo) * rows) continue;   // (cannot happen with a consistent S; keeps a lane in bounds)
    const uint32_t i = xlo + (uint32_t)local / rows, j = ylo + (uint32_t)local % rows;
    if (i >= g.n[0] || j >= g.n[1]) continue;
    const TriRec& rec = tris[t];
    const f3 a = mk3(rec.ax, rec.ay, rec.az), b = mk3(rec.bx, rec.by, rec.bz), c = mk3(rec.cx, rec.cy, rec.cz);
    const BandBox bx = band_box(a, b, c);
    const float reach = reach_of(bx, r, grid_scale), reach2 = reach * reach;
    const float qx = cell_center(g.first[0], g.size[0], i), qy = cell_center(g.first[1], g.size[1], j);
    const float gx = band_gap(bx.lo[0], bx.hi[0], qx), gy = band_gap(bx.lo[1], bx.hi[1], qy);
    if (!band_near(gx, gy, 0.0f, reach2)) continue;
    uint32_t klo, khi;
    band_interval(bx.lo[2], bx.hi[2], g.first[2], g.size[2], zlo, zhi, gx, gy, reach2, &klo, &khi);
    if (klo >= khi) continue;
    const BandPlane pl = band_plane(a, b, c, reach, g.first, g.size, g.n);
    band_plane_interval(pl, band_plane_xy(pl, qx, qy), g.first[2], g.size[2], klo, khi, &klo, &khi);
    if (klo >= khi) continue;
    uint32_t* row = bits + ((size_t)i * g.n[1] + j) * g.nzw;
    for (uint32_t word = klo >> 5; word <= (khi - 1u) >> 5; ++word) {      // word < nzw: khi <= n[2]
      const uint32_t b0 = max(klo, word << 5) & 31u, b1 = min(khi, (word + 1u) << 5) - (word << 5);   // bits [b0, b1) of this word, b1 in 1 .. 32
      const uint32_t m = (b1 == 32u ? 0xffffffffu : (1u << b1) - 1u) & ~((1u << b0) - 1u);
      atomicOr(row + word, m);
    }
  }
}

// Every cell: whole words, the last word of a row cut at nz.
__global__ __launch_bounds__(kThreads) void k_band_fill(size_t words, uint32_t nzw, uint32_t nz, uint32_t* __restrict__ bits) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= words) return;
  const bool last = (uint32_t)(i % nzw) == nzw - 1u && (nz & 31u);
  bits[i] = last ? (1u << (nz & 31u)) - 1u : 0xffffffffu;
}

// The set bits of rank [begin, end) in ascending L: cells[rank - begin] and the three floats of the centre.  tile_off: the exclusive sums
// of the tiles' popcounts (launch_voxel_count), *total their sum.
__global__ __launch_bounds__(kThreads) void k_band_emit(const uint32_t* __restrict__ bits, size_t words, GridParams g, const uint64_t* __restrict__ tile_off,
                                                        const uint64_t* __restrict__ total, uint32_t tiles, uint64_t begin, uint64_t end,
                                                        uint64_t* __restrict__ cells, float* __restrict__ centres) {
  const uint64_t off0 = tile_off[blockIdx.x], off1 = blockIdx.x + 1u < tiles ? tile_off[blockIdx.x + 1u] : *total;
  if (off1 <= begin || off0 >= end) return;   // the whole workgroup
  const size_t first = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanItems;
  uint32_t w[kScanItems];
  uint64_t s = 0, all;
#pragma unroll
  for (int u = 0; u < kScanItems; ++u) {
    w[u] = first + u < words ? bits[first + u] : 0u;
    s += (uint64_t)__popc(w[u]);
  }
  uint64_t run = off0 + block_exclusive_scan<kThreads>(s, &all);
  for (int u = 0; u < kScanItems; ++u) {
    uint32_t m = w[u];
    if (m == 0u) continue;
    const size_t wi = first + u;
    const uint64_t rowi = wi / g.nzw;
    const uint32_t k0 = (uint32_t)(wi % g.nzw) * 32u;
    const uint32_t i = (uint32_t)(rowi / g.n[1]), j = (uint32_t)(rowi % g.n[1]);
    while (m) {
      const uint32_t b = (uint32_t)__ffs((int)m) - 1u;
      m &= m - 1u;
      if (run >= begin && run < end) {
        const uint64_t n = run - begin;
        cells[n] = rowi * g.n[2] + k0 + b;
        centres[3 * n] = cell_center(g.first[0], g.size[0], i);
        centres[3 * n + 1] = cell_center(g.first[1], g.size[1], j);
        centres[3 * n + 2] = cell_center(g.first[2], g.size[2], k0 + b);
      }
      ++run;
    }
  }
}

// The filter of the contract on one distance.  -0 <= 0 and 0 <= +0 hold, a NaN fails both.
__device__ __forceinline__ bool band_active(float d, float interior, float exterior) { return -interior <= d && d <= exterior; }

// d[n]: what the query walk left (Raycast: unsigned; Normal: the fold's result).  The plane bit negates as the dense walk's epilogue does.
// The cells ascend, so the lanes of one mask word are neighbours: their bits are OR-ed along the wave first (a segmented scan by shuffles:
// after the step of offset o a lane holds the bits of the next 2 o lanes of its word) and the first lane of each run issues the one atomicOr.
__global__ __launch_bounds__(kThreads) void k_band_filter(const uint64_t* __restrict__ cells, float* __restrict__ d, uint32_t n, const uint32_t* __restrict__ plane,
                                                          uint32_t nzw, uint32_t nz, float interior, float exterior, uint32_t* __restrict__ bits,
                                                          uint8_t* __restrict__ flags) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  const bool valid = q < n;
  unsigned long long w = ~0ull;   // no word: lanes past the end
  uint32_t acc = 0;
  if (valid) {
    const uint64_t L = cells[q], rowi = L / nz;
    const uint32_t k = (uint32_t)(L % nz);
    w = rowi * nzw + (k >> 5);
    float v = d[q];
    if (plane && ((plane[w] >> (k & 31u)) & 1u)) {
      v = -v;
      d[q] = v;
    }
    const bool on = band_active(v, interior, exterior);
    flags[q] = on ? 1 : 0;
    acc = on ? 1u << (k & 31u) : 0u;
  }
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 32; o <<= 1) {   // a word has 32 cells: a run is at most 32 lanes
    const unsigned long long ow = __shfl_down(w, o, 64);
    const uint32_t oa = __shfl_down(acc, o, 64);
    if (lane + o < 64 && ow == w) acc |= oa;
  }
  const unsigned long long pw = __shfl_up(w, 1, 64);
  if (valid && acc && (lane == 0 || pw != w)) atomicOr(bits + w, acc);
}

__device__ __forceinline__ uint64_t tile_flags(const uint8_t* __restrict__ flags, uint32_t n, uint32_t (&w)[kScanItems]) {
  const uint32_t first = blockIdx.x * kScanTile + threadIdx.x * kScanItems;
  uint64_t s = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    w[k] = first + k < n ? flags[first + k] : 0u;
    s += w[k];
  }
  return s;
}

__global__ __launch_bounds__(kThreads) void k_band_flag_sums(const uint8_t* __restrict__ flags, uint32_t n, uint64_t* __restrict__ tile_sum) {
  uint32_t w[kScanItems];
  uint64_t all;
  const uint64_t s = tile_flags(flags, n, w);
  (void)block_exclusive_scan<kThreads>(s, &all);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
}

// Flagged entries to out[*running + rank], entries from `capacity` on dropped.  *running is advanced by k_band_advance, behind this kernel.
__global__ __launch_bounds__(kThreads) void k_band_compact(const uint8_t* __restrict__ flags, const uint64_t* __restrict__ cells, const float* __restrict__ d,
                                                           uint32_t n, const uint64_t* __restrict__ tile_off, const uint64_t* __restrict__ running,
                                                           uint64_t capacity, uint64_t* __restrict__ cells_out, float* __restrict__ d_out) {
  uint32_t w[kScanItems];
  uint64_t all;
  const uint64_t s = tile_flags(flags, n, w);
  uint64_t run = *running + tile_off[blockIdx.x] + block_exclusive_scan<kThreads>(s, &all);
  const uint32_t first = blockIdx.x * kScanTile + threadIdx.x * kScanItems;
  for (int k = 0; k < kScanItems; ++k) {
    if (w[k] == 0u) continue;
    if (run < capacity) {
      if (cells_out) cells_out[run] = cells[first + k];
      if (d_out) d_out[run] = d[first + k];
    }
    ++run;
  }
}

__global__ void k_band_advance(uint64_t* __restrict__ running, const uint64_t* __restrict__ chunk_total) { *running += *chunk_total; }

// algorithm 1: the active mask straight from the dense grid, one word per lane (complete words: no atomics, no clearing first).
__global__ __launch_bounds__(kThreads) void k_band_dense_mask(const float* __restrict__ dense, size_t words, uint32_t nzw, uint32_t nz, float interior,
                                                              float exterior, uint32_t* __restrict__ bits) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= words) return;
  const uint32_t k0 = (uint32_t)(i % nzw) * 32u, cnt = min(32u, nz - k0);
  const float* row = dense + (uint64_t)(i / nzw) * nz + k0;
  uint32_t m = 0;
  for (uint32_t b = 0; b < cnt; ++b) m |= band_active(row[b], interior, exterior) ? 1u << b : 0u;
  bits[i] = m;
}

__global__ __launch_bounds__(kThreads) void k_band_gather(const float* __restrict__ dense, const uint64_t* __restrict__ cells, uint64_t n, float* __restrict__ d_out) {
  const uint64_t q = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q < n) d_out[q] = dense[cells[q]];
}

inline size_t mask_words(const GridParams& g) { return (size_t)g.n[0] * g.n[1] * g.nzw; }

}  // namespace

void warm_band(hipStream_t st) { hipLaunchKernelGGL(k_warm_band, dim3(1), dim3(64), 0, st); }

float band_grid_scale(const GridParams& g) {
  float s = 0.0f;
  for (int m = 0; m < 3; ++m) {
    const float a = fabsf(cell_center(g.first[m], g.size[m], 0u)), b = fabsf(cell_center(g.first[m], g.size[m], g.n[m] ? g.n[m] - 1u : 0u));
    s = std::max(s, std::max(a, b));
  }
  return s;
}

size_t band_chunk_bytes(size_t chunk) {
  const size_t a = 256;
  return (chunk * 8 + a) + (chunk * 12 + a) + (chunk * 4 + a) + (chunk + a) + ((size_t)tiles_of(chunk) + 1) * 8 + a + 1024;
}

int band_chunk_carve(Arena& ws, size_t chunk, BandChunk* c) {
  c->cells = ws.take<uint64_t>(chunk);
  c->centres = ws.take<float>(3 * chunk);
  c->dist = ws.take<float>(chunk);
  c->flags = ws.take<uint8_t>(chunk);
  c->tile_sum = ws.take<uint64_t>((size_t)tiles_of(chunk) + 1);
  c->hdr = ws.take<uint64_t>(4);
  return (c->cells && c->centres && c->dist && c->flags && c->tile_sum && c->hdr) ? 0 : -1;
}

int launch_band_candidates(hipStream_t st, const TriRec* tris, uint32_t n_tris, const GridParams& g, float r, const VoxelScratch& s, uint32_t* bits) {
  const size_t words = mask_words(g);
  if (words == 0) return 0;
  if (r == __builtin_inff()) {   // every cell, whatever the mesh
    hipLaunchKernelGGL(k_band_fill, dim3((unsigned)((words + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, words, g.nzw, g.n[2], bits);
    M2S_HIP_CHECK(hipGetLastError());
    return 0;
  }
  M2S_HIP_CHECK(hipMemsetAsync(bits, 0, words * 4, st));
  if (n_tris == 0) return 0;
  const uint32_t tiles = tiles_of(n_tris);
  const float gs = band_grid_scale(g);
  hipLaunchKernelGGL(k_band_count, dim3((n_tris + kThreads - 1) / kThreads), dim3(kThreads), 0, st, tris, n_tris, g, r, gs, s.iv, s.cols);
  hipLaunchKernelGGL(k_tile_sums<false>, dim3(tiles), dim3(kThreads), 0, st, (const void*)s.cols, (size_t)n_tris, s.tile_sum);
  hipLaunchKernelGGL((k_scan_tiles<kThreads, uint32_t>), dim3(1), dim3(kThreads), 0, st, s.tile_sum, tiles, s.hdr + 1);
  hipLaunchKernelGGL(k_col_scan<uint32_t>, dim3(tiles), dim3(kThreads), 0, st, (const uint64_t*)s.cols, n_tris, (const uint64_t*)s.tile_sum, s.S);
  hipLaunchKernelGGL(k_band_raster, dim3(kRasterBlocks), dim3(kThreads), 0, st, tris, n_tris, g, r, gs, (const uint32_t*)s.iv, (const uint64_t*)s.S, bits);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_band_emit(hipStream_t st, const GridParams& g, const uint32_t* cand, const VoxelScratch& s, uint64_t begin, uint64_t end, const BandChunk& c) {
  const size_t words = mask_words(g);
  const uint32_t tiles = tiles_of(words);
  hipLaunchKernelGGL(k_band_emit, dim3(tiles), dim3(kThreads), 0, st, cand, words, g, (const uint64_t*)s.tile_sum, (const uint64_t*)s.hdr, tiles, begin, end,
                     c.cells, c.centres);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_band_filter(hipStream_t st, const GridParams& g, const BandChunk& c, uint32_t n, const uint32_t* plane, float interior, float exterior,
                       uint32_t* bits, uint64_t* running, uint64_t capacity, uint64_t* cells_out, float* d_out) {
  if (n == 0) return 0;
  const uint32_t tiles = tiles_of(n);
  hipLaunchKernelGGL(k_band_filter, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, st, (const uint64_t*)c.cells, c.dist, n, plane, g.nzw, g.n[2],
                     interior, exterior, bits, c.flags);
  hipLaunchKernelGGL(k_band_flag_sums, dim3(tiles), dim3(kThreads), 0, st, (const uint8_t*)c.flags, n, c.tile_sum);
  hipLaunchKernelGGL((k_scan_tiles<kThreads, uint32_t>), dim3(1), dim3(kThreads), 0, st, c.tile_sum, tiles, c.hdr);
  if (cells_out || d_out)
    hipLaunchKernelGGL(k_band_compact, dim3(tiles), dim3(kThreads), 0, st, (const uint8_t*)c.flags, (const uint64_t*)c.cells, (const float*)c.dist, n,
                       (const uint64_t*)c.tile_sum, (const uint64_t*)running, capacity, cells_out, d_out);
  hipLaunchKernelGGL(k_band_advance, dim3(1), dim3(1), 0, st, running, (const uint64_t*)c.hdr);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_band_dense_mask(hipStream_t st, const GridParams& g, const float* dense, float interior, float exterior, uint32_t* bits) {
  const size_t words = mask_words(g);
  if (words == 0) return 0;
  hipLaunchKernelGGL(k_band_dense_mask, dim3((unsigned)((words + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, dense, words, g.nzw, g.n[2], interior,
                     exterior, bits);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_band_gather(hipStream_t st, const float* dense, const uint64_t* cells, uint64_t n, float* d_out) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_band_gather, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, dense, cells, n, d_out);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace m2s
