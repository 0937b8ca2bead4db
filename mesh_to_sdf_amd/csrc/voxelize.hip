// voxelize.hip — surface and solid occupancy of a grid (m2s_voxelize, m2s_mesh_voxelize), gfx950.  DESIGN.md §4.12.
//
// The contract is include/m2s.h's and its predicate is voxel.hip.h; tests/voxel_model.py restates both in numpy and the GPU tests compare
// the two bit for bit.  The mask is one bit per cell in the layout of sign.hip's planes; everything else is derived from it.
//   k_vox_count     per triangle: the intervals of cells that pass its three box clauses (vox_interval: two binary searches per axis with
//                   the clause's own operations, so the candidate box is exact however far the mesh is from the origin) and the number
//                   of (i, j) columns in them, 0 when any interval is empty or a coordinate is not finite.
//   the scan        exclusive running sums S of the column counts in uint64: k_tile_sums, k_scan_tiles, k_col_scan (the two-level
//                   pattern of scan.hip.h); S[n_tris] = the number of columns.
//   k_vox_raster    one column per lane, grid-stride over S[n_tris] (read on the device: no trip to the host).  A lane finds its triangle by
//                   a binary search in S — neighbouring lanes take neighbouring columns of the same few triangles, so the loads coalesce —
//                   evaluates the three cross axes with m = z once (the x and y box clauses hold by construction of the intervals), and on
//                   survival walks the z interval with the plane and the other six cross axes, gathering the hits of one 32-cell word in a
//                   register: one atomicOr per touched word.
//   epilogue        k_or_plane (SOLID: the sign plane's words, padding bits masked), k_tile_sums<popcount> + k_scan_tiles (the count),
//                   k_expand (occupancy bytes, 4 cells per lane), k_emit_cells (per-tile offsets + a workgroup scan: ascending L falls out
//                   of the layout).
//   k_vox_brute     algorithm 1, the definition: every cell against every triangle, all 13 clauses.
// The result is an OR over triangles: the order of the records does not matter, so a persistent mesh reads its resident (sorted) records
// and a one-shot call the input-order records of a records-only build.
#include <algorithm>

#include "common.h"
#include "geo.hip.h"
#include "scan.hip.h"
#include "voxel.hip.h"

namespace m2s {

namespace {

__global__ void k_warm_voxelize() {}

constexpr int kThreads = kTileThreads;
constexpr unsigned kRasterBlocks = 4096;   // 16 workgroups per CU's worth of grid-stride lanes

__device__ __forceinline__ VoxTri load_vox_tri(const TriRec* __restrict__ tris, uint32_t t) {
  const TriRec& r = tris[t];
  return vox_tri(mk3(r.ax, r.ay, r.az), mk3(r.bx, r.by, r.bz), mk3(r.cx, r.cy, r.cz));
}

// iv[6 t ..]: x lo, x hi, y lo, y hi, z lo, z hi.
__global__ __launch_bounds__(kThreads) void k_vox_count(const TriRec* __restrict__ tris, uint32_t n_tris, GridParams g, uint32_t* __restrict__ iv,
                                                        uint64_t* __restrict__ cols) {
  const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= n_tris) return;
  const VoxTri tr = load_vox_tri(tris, t);
  uint32_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  bool any = tr.finite;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    if (any) vox_interval(tr.a[m], tr.b[m], tr.c[m], g.first[m], g.size[m], g.n[m], &lo[m], &hi[m]);
    any = any && lo[m] < hi[m];
  }
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    iv[6 * (size_t)t + 2 * m] = lo[m];
    iv[6 * (size_t)t + 2 * m + 1] = hi[m];
  }
  cols[t] = any ? (uint64_t)(hi[0] - lo[0]) * (uint64_t)(hi[1] - lo[1]) : 0;   // < 2^32: a grid face has fewer lines (fill_grid_params)
}

__global__ __launch_bounds__(kThreads) void k_vox_raster(const TriRec* __restrict__ tris, uint32_t n_tris, GridParams g,
                                                         const uint32_t* __restrict__ iv, const uint64_t* __restrict__ S,
                                                         uint32_t* __restrict__ bits) {
  const uint64_t total = S[n_tris];
  const float h[3] = {g.size[0] * 0.5f, g.size[1] * 0.5f, g.size[2] * 0.5f};
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
    const VoxTri tr = load_vox_tri(tris, t);
    const float qx = vox_centre(g.first[0], g.size[0], i), qy = vox_centre(g.first[1], g.size[1], j);
    float v0[3] = {tr.a[0] - qx, tr.a[1] - qy, 0.0f}, v1[3] = {tr.b[0] - qx, tr.b[1] - qy, 0.0f}, v2[3] = {tr.c[0] - qx, tr.c[1] - qy, 0.0f};
    if (vox_column_miss(tr, v0, v1, v2, h)) continue;
    uint32_t* row = bits + ((size_t)i * g.n[1] + j) * g.nzw;
    uint32_t word = zlo >> 5, acc = 0;
    for (uint32_t k = zlo; k < zhi; ++k) {
      if ((k >> 5) != word) {
        if (acc) atomicOr(row + word, acc);
        word = k >> 5;
        acc = 0;
      }
      const float qz = vox_centre(g.first[2], g.size[2], k);
      v0[2] = tr.a[2] - qz;
      v1[2] = tr.b[2] - qz;
      v2[2] = tr.c[2] - qz;
      if (!vox_cell_miss(tr, v0, v1, v2, h)) acc |= 1u << (k & 31u);
    }
    if (acc) atomicOr(row + word, acc);
  }
}

// algorithm 1: one cell per lane, every triangle (a wave reads the same record: scalar loads), all 13 clauses.
__global__ __launch_bounds__(kThreads) void k_vox_brute(const TriRec* __restrict__ tris, uint32_t n_tris, GridParams g, uint64_t cells,
                                                        uint32_t* __restrict__ bits) {
  const uint64_t L = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (L >= cells) return;
  const uint32_t k = (uint32_t)(L % g.n[2]);
  const uint64_t rowi = L / g.n[2];
  const uint32_t j = (uint32_t)(rowi % g.n[1]), i = (uint32_t)(rowi / g.n[1]);
  const float q[3] = {vox_centre(g.first[0], g.size[0], i), vox_centre(g.first[1], g.size[1], j), vox_centre(g.first[2], g.size[2], k)};
  const float h[3] = {g.size[0] * 0.5f, g.size[1] * 0.5f, g.size[2] * 0.5f};
  bool set = false;
  for (uint32_t t = 0; t < n_tris && !set; ++t) set = vox_overlap(load_vox_tri(tris, t), q, h);
  if (set) atomicOr(bits + rowi * g.nzw + (k >> 5), 1u << (k & 31u));
}

// bits |= plane, the plane's bits at k >= nz dropped.
__global__ __launch_bounds__(kThreads) void k_or_plane(const uint32_t* __restrict__ plane, size_t words, uint32_t nzw, uint32_t nz,
                                                       uint32_t* __restrict__ bits) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= words) return;
  uint32_t p = plane[i];
  if ((uint32_t)(i % nzw) == nzw - 1u && (nz & 31u)) p &= (1u << (nz & 31u)) - 1u;
  if (p) bits[i] |= p;
}

// occupancy bytes: four consecutive cells per lane, one dword store where the run is whole (occ is then 4-byte aligned).
__global__ __launch_bounds__(kThreads) void k_expand(const uint32_t* __restrict__ bits, uint64_t cells, uint32_t nzw, uint32_t nz, bool dwords,
                                                     uint8_t* __restrict__ occ) {
  const uint64_t L0 = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
  if (L0 >= cells) return;
  uint64_t row = L0 / nz;
  uint32_t k = (uint32_t)(L0 % nz);
  uint32_t packed = 0;
  const uint32_t cnt = (uint32_t)min((uint64_t)4, cells - L0);
  for (uint32_t u = 0; u < cnt; ++u) {
    const uint32_t b = (bits[row * nzw + (k >> 5)] >> (k & 31u)) & 1u;
    packed |= b << (8 * u);
    if (++k == nz) { k = 0; ++row; }
  }
  if (dwords && cnt == 4) {
    *reinterpret_cast<uint32_t*>(occ + L0) = packed;
  } else {
    for (uint32_t u = 0; u < cnt; ++u) occ[L0 + u] = (uint8_t)(packed >> (8 * u));
  }
}

// cells_out: the L of every set bit, ascending.  tile_off: the exclusive sums of the tiles' popcounts.
__global__ __launch_bounds__(kThreads) void k_emit_cells(const uint32_t* __restrict__ bits, size_t words, uint32_t nzw, uint32_t nz,
                                                         const uint64_t* __restrict__ tile_off, uint64_t capacity, uint64_t* __restrict__ out) {
  uint64_t w[kScanItems], all;
  const uint64_t s = tile_items<true>(bits, words, w);
  uint64_t run = tile_off[blockIdx.x] + block_exclusive_scan<kThreads>(s, &all);
  const size_t first = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanItems;
  for (int u = 0; u < kScanItems; ++u) {
    if (first + u >= words || w[u] == 0) continue;
    const size_t i = first + u;
    const uint64_t base = (uint64_t)(i / nzw) * nz + (uint64_t)(i % nzw) * 32u;
    uint32_t m = bits[i];
    while (m) {
      const uint32_t b = (uint32_t)__ffs((int)m) - 1u;
      m &= m - 1u;
      if (run < capacity) out[run] = base + b;
      ++run;
    }
  }
}

inline size_t mask_words(const GridParams& g) { return (size_t)g.n[0] * g.n[1] * g.nzw; }
inline uint64_t grid_cells(const GridParams& g) { return (uint64_t)g.n[0] * g.n[1] * g.n[2]; }

}  // namespace

void warm_voxelize(hipStream_t st) { hipLaunchKernelGGL(k_warm_voxelize, dim3(1), dim3(64), 0, st); }

size_t voxel_scratch_bytes(const GridParams& g, size_t n_tris) {
  const size_t tiles = std::max(tiles_of(n_tris), tiles_of(mask_words(g)));
  return (n_tris * 24 + 255) / 256 * 256 + 2 * ((n_tris * 8 + 8 + 255) / 256 * 256) + (tiles * 8 + 255) / 256 * 256 + 1024;
}

int voxel_scratch_carve(Arena& ws, const GridParams& g, size_t n_tris, VoxelScratch* s) {
  const size_t tiles = std::max(tiles_of(n_tris), tiles_of(mask_words(g)));
  s->iv = ws.take<uint32_t>(6 * n_tris + 1);
  s->cols = ws.take<uint64_t>(n_tris + 1);
  s->S = ws.take<uint64_t>(n_tris + 1);
  s->tile_sum = ws.take<uint64_t>(tiles + 1);
  s->hdr = ws.take<uint64_t>(4);
  return (s->iv && s->cols && s->S && s->tile_sum && s->hdr) ? 0 : -1;
}

int launch_voxelize_surface(hipStream_t st, const TriRec* tris, uint32_t n_tris, const GridParams& g, int algorithm, const VoxelScratch& s,
                            uint32_t* bits) {
  const size_t words = mask_words(g);
  if (words == 0) return 0;
  M2S_HIP_CHECK(hipMemsetAsync(bits, 0, words * 4, st));
  if (n_tris == 0) return 0;
  if (algorithm == 1) {
    const uint64_t cells = grid_cells(g);
    hipLaunchKernelGGL(k_vox_brute, dim3((unsigned)((cells + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, tris, n_tris, g, cells, bits);
  } else {
    const uint32_t tiles = tiles_of(n_tris);
    hipLaunchKernelGGL(k_vox_count, dim3((n_tris + kThreads - 1) / kThreads), dim3(kThreads), 0, st, tris, n_tris, g, s.iv, s.cols);
    hipLaunchKernelGGL(k_tile_sums<false>, dim3(tiles), dim3(kThreads), 0, st, (const void*)s.cols, (size_t)n_tris, s.tile_sum);
    hipLaunchKernelGGL((k_scan_tiles<kThreads, uint32_t>), dim3(1), dim3(kThreads), 0, st, s.tile_sum, tiles, s.hdr + 1);
    hipLaunchKernelGGL(k_col_scan<uint32_t>, dim3(tiles), dim3(kThreads), 0, st, (const uint64_t*)s.cols, n_tris, (const uint64_t*)s.tile_sum, s.S);
    hipLaunchKernelGGL(k_vox_raster, dim3(kRasterBlocks), dim3(kThreads), 0, st, tris, n_tris, g, (const uint32_t*)s.iv, (const uint64_t*)s.S, bits);
  }
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_voxel_or_plane(hipStream_t st, const GridParams& g, const uint32_t* plane, uint32_t* bits) {
  const size_t words = mask_words(g);
  if (words == 0) return 0;
  hipLaunchKernelGGL(k_or_plane, dim3((unsigned)((words + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, plane, words, g.nzw, g.n[2], bits);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_voxel_count(hipStream_t st, const GridParams& g, const uint32_t* bits, const VoxelScratch& s) {
  const size_t words = mask_words(g);
  const uint32_t tiles = tiles_of(words);
  hipLaunchKernelGGL(k_tile_sums<true>, dim3(tiles), dim3(kThreads), 0, st, (const void*)bits, words, s.tile_sum);
  hipLaunchKernelGGL((k_scan_tiles<kThreads, uint32_t>), dim3(1), dim3(kThreads), 0, st, s.tile_sum, tiles, s.hdr);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_voxel_expand(hipStream_t st, const GridParams& g, const uint32_t* bits, uint8_t* occ) {
  const uint64_t cells = grid_cells(g), lanes = (cells + 3) / 4;
  const bool dwords = (reinterpret_cast<uintptr_t>(occ) & 3u) == 0;
  hipLaunchKernelGGL(k_expand, dim3((unsigned)((lanes + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, bits, cells, g.nzw, g.n[2], dwords, occ);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_voxel_cells(hipStream_t st, const GridParams& g, const uint32_t* bits, const VoxelScratch& s, uint64_t capacity, uint64_t* cells_out) {
  const size_t words = mask_words(g);
  hipLaunchKernelGGL(k_emit_cells, dim3(tiles_of(words)), dim3(kThreads), 0, st, bits, words, g.nzw, g.n[2], (const uint64_t*)s.tile_sum, capacity, cells_out);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace m2s
