// isosurface.hip — m2s_grid_isosurface: a welded, indexed triangle mesh of a level set of a finished grid SDF (marching cubes with
// the table of isosurface_table.h; the exact contract is include/m2s.h's).  tests/isosurface_model.py restates it in numpy and the
// GPU tests compare the two bit for bit.
//
// Passes:
//   k_iso_classify   the only pass over the whole grid.  A tile of 8192 consecutive points per workgroup; a point is ACTIVE if one of
//                    its three edges crosses the level or its cell's case is neither 0 nor 255.  Each wave ballots 64 points into a
//                    64-bit word of the active mask; the tile's count goes to tile_count.  Non-finite values raise a flag.
//   k_scan_tiles     exclusive scan of the tile counts in one workgroup; the total is the number of active points.
//   k_iso_compact    reads the mask (1 bit per point) and writes the active points' L in ascending order, and each mask word's
//                    offset in that list (so the index of an active point is two loads and a popcount away).
//   k_iso_info       per active point: edge flags (3 bits) and case; per 4096-point block the vertex and triangle sums.
//   k_scan_tiles     the block sums, twice (vertices, triangles): totals = the counts the call returns.
//   k_iso_vertices   per active point: its first vertex id (kept, u32) and its vertices' positions.
//   k_iso_triangles  per active cell: its triangles; an edge owned by another point finds that point's index from the mask word
//                    offsets, and its vertex id is the owner's first id plus the axis's rank among the owner's flags.
// 64-bit point indices throughout (a 1040 x 1024 x 1024 grid has byte offsets beyond 2^32).
// The table, IsoGrid, decode and active_index live in isosurface.hip.h, which band_isosurface.hip shares; the workgroup scan and
// k_scan_tiles in scan.hip.h.
#include "../../include/m2s.h"
#include "capi_internal.h"
#include "common.h"
#include "isosurface.hip.h"

#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace m2s {
namespace {

constexpr int kClassifyThreads = 256;
constexpr int kTile = 8192;                       // points per classify / compact workgroup = 128 mask words
constexpr int kTileIters = kTile / kClassifyThreads;

__device__ __forceinline__ void advance(const IsoGrid& g, Pt& p, uint64_t step) {
  // step <= nz wraps a row at most once: no 64-bit division on the common path
  p.k += step;
  if (p.k >= g.n[2]) {
    uint64_t q = 1;
    if (p.k < 2 * g.n[2]) p.k -= g.n[2];
    else { q = p.k / g.n[2]; p.k -= q * g.n[2]; }
    p.j += q;
    if (p.j >= g.n[1]) {
      if (p.j < 2 * g.n[1]) { p.j -= g.n[1]; ++p.i; }
      else { const uint64_t q2 = p.j / g.n[1]; p.j -= q2 * g.n[1]; p.i += q2; }
    }
  }
}

// The eight corner values a point needs (its own, its three edge ends, the rest of its cell) and which of them exist.
// Returns (edge flags) | (case << 3) | (has cell << 11).
__device__ __forceinline__ uint32_t point_bits(const IsoGrid& g, const float* __restrict__ d, uint64_t L, const Pt& p, float* d0_out) {
  const bool ex = p.i + 1 < g.n[0], ey = p.j + 1 < g.n[1], ez = p.k + 1 < g.n[2];
  const bool cell = ex && ey && ez;
  // every offset is computed first and clamped to the point itself where the neighbour does not exist, so the eight loads are
  // unconditional and issue together
  const uint64_t sx = ex ? g.nyz : 0, sy = ey ? g.n[2] : 0, sz = ez ? 1 : 0;
  const uint64_t cx = cell ? sx : 0, cy = cell ? sy : 0, cz = cell ? sz : 0;
  const float v000 = d[L];
  const float v001 = d[L + sz];
  const float v010 = d[L + sy];
  const float v100 = d[L + sx];
  const float v011 = d[L + cy + cz];
  const float v101 = d[L + cx + cz];
  const float v110 = d[L + cx + cy];
  const float v111 = d[L + cx + cy + cz];
  *d0_out = v000;
  const float iso = g.iso;
  const uint32_t i000 = v000 < iso, i001 = v001 < iso, i010 = v010 < iso, i100 = v100 < iso;
  uint32_t flags = (uint32_t)(ex && i100 != i000) | ((uint32_t)(ey && i010 != i000) << 1) | ((uint32_t)(ez && i001 != i000) << 2);
  uint32_t cs = 0;
  if (cell)
    cs = i000 | (i001 << 1) | (i010 << 2) | ((uint32_t)(v011 < iso) << 3) | (i100 << 4) | ((uint32_t)(v101 < iso) << 5) |
         ((uint32_t)(v110 < iso) << 6) | ((uint32_t)(v111 < iso) << 7);
  return flags | (cs << 3) | ((uint32_t)cell << 11);
}

__device__ __forceinline__ bool active_bits(uint32_t b) {
  const uint32_t cs = (b >> 3) & 255;
  return (b & 7) != 0 || (cs != 0 && cs != 255);
}

__global__ void __launch_bounds__(kClassifyThreads) k_iso_classify(IsoGrid g, const float* __restrict__ d, uint64_t* __restrict__ mask,
                                                                  uint64_t* __restrict__ tile_count, uint32_t* __restrict__ nonfinite) {
  __shared__ uint32_t wave_count[kClassifyThreads / 64];
  const uint64_t base = (uint64_t)blockIdx.x * kTile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t L = base + threadIdx.x;
  Pt p = decode(g, L < g.total ? L : 0);
  uint32_t count = 0;
  bool bad = false;
  for (int it = 0; it < kTileIters; ++it, L += kClassifyThreads) {
    bool act = false;
    if (L < g.total) {
      float d0;
      const uint32_t b = point_bits(g, d, L, p, &d0);
      act = active_bits(b);
      bad |= !isfinite(d0);
    }
    const uint64_t word = __ballot(act);
    const uint64_t w0 = L - lane;   // a multiple of 64
    if (lane == 0 && w0 < g.total) mask[w0 >> 6] = word;
    count += (uint32_t)__popcll(word);
    advance(g, p, kClassifyThreads);
  }
  if (__ballot(bad) != 0 && lane == 0) atomicOr(nonfinite, 1u);
  if (lane == 0) wave_count[wave] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t s = 0;
    for (int w = 0; w < kClassifyThreads / 64; ++w) s += wave_count[w];
    tile_count[blockIdx.x] = s;
  }
}

__global__ void __launch_bounds__(kTile / 64) k_iso_compact(const uint64_t* __restrict__ mask, uint64_t n_words,
                                                            const uint64_t* __restrict__ tile_off, uint64_t* __restrict__ act,
                                                            uint64_t* __restrict__ word_off) {
  const uint64_t w = (uint64_t)blockIdx.x * (kTile / 64) + threadIdx.x;
  uint64_t word = w < n_words ? mask[w] : 0;
  uint64_t tile_total;
  uint64_t o = tile_off[blockIdx.x] + block_exclusive_scan<kTile / 64>((uint64_t)__popcll(word), &tile_total);
  if (w < n_words) word_off[w] = o;
  while (word) {
    const int bit = __ffsll((long long)word) - 1;
    act[o++] = (w << 6) + (uint64_t)bit;
    word &= word - 1;
  }
}

// Per active point: info = point bits; per block of kItemBlock points: (vertex, triangle) sums.
__global__ void __launch_bounds__(kItemThreads) k_iso_info(IsoGrid g, const float* __restrict__ d, const uint64_t* __restrict__ act,
                                                           uint64_t n_act, uint32_t* __restrict__ info, uint64_t* __restrict__ vsum,
                                                           uint64_t* __restrict__ tsum) {
  const uint64_t b = (uint64_t)blockIdx.x * kItemBlock + (uint64_t)threadIdx.x * kItemsPerThread;
  uint64_t nv = 0, nt = 0;
  for (int r = 0; r < kItemsPerThread; ++r) {
    const uint64_t a = b + r;
    if (a >= n_act) break;
    const uint64_t L = act[a];
    float d0;
    const uint32_t bits = point_bits(g, d, L, decode(g, L), &d0);
    info[a] = bits;
    nv += __popc(bits & 7);
    nt += kIsoTriCount[(bits >> 3) & 255];
  }
  uint64_t tv, tt;
  (void)block_exclusive_scan<kItemThreads>(nv, &tv);
  (void)block_exclusive_scan<kItemThreads>(nt, &tt);
  if (threadIdx.x == 0) {
    vsum[blockIdx.x] = tv;
    tsum[blockIdx.x] = tt;
  }
}

// First vertex id of each active point (n_vertices < 2^32 is checked before this runs) and the positions of its vertices.
__global__ void __launch_bounds__(kItemThreads) k_iso_vertices(IsoGrid g, const float* __restrict__ d, const uint64_t* __restrict__ act,
                                                               uint64_t n_act, const uint32_t* __restrict__ info,
                                                               const uint64_t* __restrict__ voff_block, uint32_t* __restrict__ voff,
                                                               float* __restrict__ vout) {
  const uint64_t b = (uint64_t)blockIdx.x * kItemBlock + (uint64_t)threadIdx.x * kItemsPerThread;
  uint64_t nv = 0;
  for (int r = 0; r < kItemsPerThread && b + r < n_act; ++r) nv += __popc(info[b + r] & 7);
  uint64_t all;
  uint64_t v = voff_block[blockIdx.x] + block_exclusive_scan<kItemThreads>(nv, &all);
  for (int r = 0; r < kItemsPerThread; ++r) {
    const uint64_t a = b + r;
    if (a >= n_act) break;
    const uint32_t flags = info[a] & 7;
    voff[a] = (uint32_t)v;
    if (!flags) continue;
    const uint64_t L = act[a];
    const Pt p = decode(g, L);
    const float d0 = d[L];
    // pos = first + (float)i * cs per axis (m2s_grid_cell_center)
    const float px = g.first[0] + (float)p.i * g.cs[0];
    const float py = g.first[1] + (float)p.j * g.cs[1];
    const float pz = g.first[2] + (float)p.k * g.cs[2];
    const uint64_t step[3] = {g.nyz, g.n[2], 1};
    const uint64_t idx[3] = {p.i, p.j, p.k};
    for (int ax = 0; ax < 3; ++ax) {
      if (!((flags >> ax) & 1)) continue;
      const float d1 = d[L + step[ax]];
      const float t = (g.iso - d0) / (d1 - d0);
      const float p0 = ax == 0 ? px : (ax == 1 ? py : pz);
      const float p1 = g.first[ax] + (float)(idx[ax] + 1) * g.cs[ax];
      float c[3] = {px, py, pz};
      c[ax] = p0 + t * (p1 - p0);
      float* o = vout + v * 3;
      o[0] = c[0];
      o[1] = c[1];
      o[2] = c[2];
      ++v;
    }
  }
}

__global__ void __launch_bounds__(kItemThreads) k_iso_triangles(IsoGrid g, const uint64_t* __restrict__ act, uint64_t n_act,
                                                                const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_off,
                                                                const uint32_t* __restrict__ info, const uint32_t* __restrict__ voff,
                                                                const uint64_t* __restrict__ toff_block, uint32_t* __restrict__ tout) {
  const uint64_t b = (uint64_t)blockIdx.x * kItemBlock + (uint64_t)threadIdx.x * kItemsPerThread;
  uint64_t nt = 0;
  for (int r = 0; r < kItemsPerThread && b + r < n_act; ++r) nt += kIsoTriCount[(info[b + r] >> 3) & 255];
  uint64_t all;
  uint64_t t = toff_block[blockIdx.x] + block_exclusive_scan<kItemThreads>(nt, &all);
  for (int r = 0; r < kItemsPerThread; ++r) {
    const uint64_t a = b + r;
    if (a >= n_act) break;
    const uint32_t cs = (info[a] >> 3) & 255;
    const int count = kIsoTriCount[cs];
    if (!count) continue;
    const uint64_t L = act[a];
    for (int tri = 0; tri < count; ++tri) {
      uint32_t id[3];
      for (int c = 0; c < 3; ++c) {
        const int e = kIsoTris[cs][tri * 3 + c];
        const int ax = e >> 2;
        const uint64_t owner = L + kIsoEdgeOffset[e][0] * g.nyz + kIsoEdgeOffset[e][1] * g.n[2] + kIsoEdgeOffset[e][2];
        const uint64_t k = owner == L ? a : active_index(mask, word_off, owner);
        // the owner is active (its edge crosses), so k < n_act and act[k] == owner; the guard keeps a broken invariant in bounds
        if (k < n_act && act[k] == owner) id[c] = voff[k] + (uint32_t)__popc(info[k] & 7 & ((1u << ax) - 1));
        else id[c] = 0xffffffffu;
      }
      uint32_t* o = tout + t * 3;
      o[0] = id[0];
      o[1] = id[1];
      o[2] = id[2];
      ++t;
    }
  }
}

// Validation that needs no device (include/m2s.h: errors before any device work).
int iso_args(const m2s_grid* grid, const float* distances, float iso, float* vertices_out, uint32_t* indices_out, uint64_t* counts,
             const m2s_opts* opts, IsoGrid* g) {
  if (!grid || !distances || !counts) return fail(M2S_ERR_BAD_ARG, "grid / distances / counts is NULL");
  if ((vertices_out == nullptr) != (indices_out == nullptr)) return fail(M2S_ERR_BAD_ARG, "vertices_out and indices_out must both be NULL or both set");
  if (opts) {
    if (opts->algorithm != 0 || opts->x_begin != 0 || opts->x_end != 0)
      return fail(M2S_ERR_BAD_ARG, "m2s_opts.algorithm / x_begin / x_end must be 0 for m2s_grid_isosurface");
    if (opts->struct_size >= sizeof(m2s_opts) && (opts->x_period != 0 || opts->n_peer_out != 0 || opts->peer_out))
      return fail(M2S_ERR_BAD_ARG, "m2s_opts.x_period / peer_out must be 0 for m2s_grid_isosurface");
  }
  if (!std::isfinite(iso)) return fail(M2S_ERR_BAD_ARG, "iso = %g is not finite", (double)iso);
  for (int k = 0; k < 3; ++k) {
    const float cs = grid->cell_size[k];
    if (grid->cell_count[k] == 0) return fail(M2S_ERR_BAD_ARG, "cell_count[%d] = 0", k);
    if (!(cs > 0.0f) || !std::isfinite(cs)) return fail(M2S_ERR_BAD_ARG, "cell_size[%d] = %g must be > 0 and finite", k, (double)cs);
    if (!std::isfinite(grid->first_cell[k])) return fail(M2S_ERR_BAD_ARG, "first_cell[%d] is not finite", k);
    g->first[k] = grid->first_cell[k];
    g->cs[k] = cs;
    g->n[k] = grid->cell_count[k];
  }
  g->nyz = g->n[1] * g->n[2];
  if (g->n[1] != 0 && g->nyz / g->n[1] != g->n[2]) return fail(M2S_ERR_BAD_ARG, "the grid has too many cells");
  g->total = g->nyz * g->n[0];
  if (g->total / g->n[0] != g->nyz || g->total > ((uint64_t)1 << 56)) return fail(M2S_ERR_BAD_ARG, "the grid has too many cells");
  g->iso = iso;
  return 0;
}

}  // namespace
}  // namespace m2s

using namespace m2s;

int m2s_grid_isosurface(const m2s_grid* grid, const float* distances, float iso, float* vertices_out, uint64_t vertex_capacity,
                        uint32_t* indices_out, uint64_t triangle_capacity, uint64_t* counts, const m2s_opts* opts) {
  clear_error();
  IsoGrid g;
  int rc = iso_args(grid, distances, iso, vertices_out, indices_out, counts, opts, &g);
  if (rc) return rc;
  counts[0] = counts[1] = 0;
  CallCtx c;
  DeviceState* st = nullptr;
  rc = resolve_ctx(opts, &c, &st);
  if (rc) return rc;
  const bool host = c.mem_kind == M2S_MEM_HOST;
  const bool fill = vertices_out != nullptr;
  const uint64_t n_words = (g.total + 63) / 64, n_tiles = (g.total + kTile - 1) / kTile;
  // phase 1: [staged grid] hdr mask tile counts; phase 2 (sized once the active count is known): the active list, its info and
  // offsets, the block sums, [staged outputs, bounded by 3 vertices and M2S_ISO_MAX_TRIS triangles per active point]
  const size_t grid_bytes = host ? align_up(g.total * 4) : 0;
  const size_t phase1 = grid_bytes + 256 + align_up(n_words * 8) * 2 + align_up(n_tiles * 8) + 4096;
  size_t need = phase1;
  uint64_t hdr[4];   // n_active, non-finite flag, n_vertices, n_triangles
  for (int attempt = 0;; ++attempt) {
    rc = ensure_capacity(*st, need);
    if (rc) return rc;
    Arena ws{st->base, st->cap, 0};
    const float* d = distances;
    if (host) {
      char* dg = ws.take<char>(g.total * 4);
      if (!dg) return fail(M2S_ERR_HIP, "internal: workspace");
      rc = staged_h2d(*st, c.stream, dg, reinterpret_cast<const char*>(distances), g.total * 4);
      if (rc) return rc;
      d = reinterpret_cast<const float*>(dg);
    }
    uint64_t* d_hdr = ws.take<uint64_t>(4);
    uint64_t* mask = ws.take<uint64_t>(n_words);
    uint64_t* tiles = ws.take<uint64_t>(n_tiles);
    uint64_t* word_off = ws.take<uint64_t>(n_words);
    if (!d_hdr || !mask || !tiles || !word_off) return fail(M2S_ERR_HIP, "internal: workspace");
    if (c.timings) M2S_HIP_CHECK(hipEventRecord(st->ev[0], c.stream));
    M2S_HIP_CHECK(hipMemsetAsync(d_hdr, 0, 32, c.stream));
    hipLaunchKernelGGL(k_iso_classify, dim3((unsigned)n_tiles), dim3(kClassifyThreads), 0, c.stream, g, d, mask, tiles,
                       reinterpret_cast<uint32_t*>(d_hdr + 1));
    hipLaunchKernelGGL((k_scan_tiles<kScanThreads, uint64_t>), dim3(1), dim3(kScanThreads), 0, c.stream, tiles, n_tiles, d_hdr);
    M2S_HIP_CHECK(hipGetLastError());
    M2S_HIP_CHECK(hipMemcpyAsync(hdr, d_hdr, 16, hipMemcpyDeviceToHost, c.stream));
    M2S_HIP_CHECK(hipStreamSynchronize(c.stream));
    if (hdr[1]) return fail(M2S_ERR_NAN, "the grid holds a NaN or infinite distance");
    const uint64_t n_act = hdr[0], n_blk = item_blocks(n_act);
    need = ws.off + 4096 + align_up(n_act * 8) + align_up(n_act * 4) * 2 + align_up(n_blk * 8) * 2 + 1024;
    if (fill && host) need += align_up(n_act * 3 * 12) + align_up(n_act * M2S_ISO_MAX_TRIS * 12);
    if (need > st->cap) {
      if (attempt) return fail(M2S_ERR_HIP, "internal: workspace");
      continue;   // grow the workspace (which drops its contents) and start again: a second pass finds room
    }
    uint64_t* act = ws.take<uint64_t>(n_act ? n_act : 1);
    uint32_t* info = ws.take<uint32_t>(n_act ? n_act : 1);
    uint32_t* voff = ws.take<uint32_t>(n_act ? n_act : 1);
    uint64_t* vsum = ws.take<uint64_t>(n_blk ? n_blk : 1);
    uint64_t* tsum = ws.take<uint64_t>(n_blk ? n_blk : 1);
    if (n_act) {
      hipLaunchKernelGGL(k_iso_compact, dim3((unsigned)n_tiles), dim3(kTile / 64), 0, c.stream, mask, n_words, tiles, act, word_off);
      hipLaunchKernelGGL(k_iso_info, dim3((unsigned)n_blk), dim3(kItemThreads), 0, c.stream, g, d, act, n_act, info, vsum, tsum);
      hipLaunchKernelGGL((k_scan_tiles<kScanThreads, uint64_t>), dim3(1), dim3(kScanThreads), 0, c.stream, vsum, n_blk, d_hdr + 2);
      hipLaunchKernelGGL((k_scan_tiles<kScanThreads, uint64_t>), dim3(1), dim3(kScanThreads), 0, c.stream, tsum, n_blk, d_hdr + 3);
      M2S_HIP_CHECK(hipGetLastError());
      M2S_HIP_CHECK(hipMemcpyAsync(hdr + 2, d_hdr + 2, 16, hipMemcpyDeviceToHost, c.stream));
      M2S_HIP_CHECK(hipStreamSynchronize(c.stream));
    } else {
      hdr[2] = hdr[3] = 0;
    }
    counts[0] = hdr[2];
    counts[1] = hdr[3];
    if (hdr[2] >= ((uint64_t)1 << 32)) return fail(M2S_ERR_BAD_ARG, "%llu vertices: u32 indices cannot address them", (unsigned long long)hdr[2]);
    if (fill && (vertex_capacity < hdr[2] || triangle_capacity < hdr[3]))
      return fail(M2S_ERR_BAD_ARG, "capacity (%llu vertices, %llu triangles) below the counts (%llu, %llu)", (unsigned long long)vertex_capacity,
                  (unsigned long long)triangle_capacity, (unsigned long long)hdr[2], (unsigned long long)hdr[3]);
    if (fill && n_act) {
      float* vdev = vertices_out;
      uint32_t* tdev = indices_out;
      if (host) {
        vdev = ws.take<float>(hdr[2] * 3 + 1);
        tdev = ws.take<uint32_t>(hdr[3] * 3 + 1);
        if (!vdev || !tdev) return fail(M2S_ERR_HIP, "internal: workspace");
      }
      hipLaunchKernelGGL(k_iso_vertices, dim3((unsigned)n_blk), dim3(kItemThreads), 0, c.stream, g, d, act, n_act, info, vsum, voff, vdev);
      hipLaunchKernelGGL(k_iso_triangles, dim3((unsigned)n_blk), dim3(kItemThreads), 0, c.stream, g, act, n_act, mask, word_off, info, voff, tsum, tdev);
      M2S_HIP_CHECK(hipGetLastError());
      if (c.timings) M2S_HIP_CHECK(hipEventRecord(st->ev[1], c.stream));
      if (host) {
        if (hdr[2] && (rc = staged_d2h(*st, c.stream, reinterpret_cast<char*>(vertices_out), reinterpret_cast<const char*>(vdev), hdr[2] * 12)))
          return rc;
        if (hdr[3] && (rc = staged_d2h(*st, c.stream, reinterpret_cast<char*>(indices_out), reinterpret_cast<const char*>(tdev), hdr[3] * 12)))
          return rc;
      }
    } else if (c.timings) {
      M2S_HIP_CHECK(hipEventRecord(st->ev[1], c.stream));
    }
    break;
  }
  M2S_HIP_CHECK(hipStreamSynchronize(c.stream));
  if (c.timings) {
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, st->ev[0], st->ev[1]);
    memset(c.timings, 0, sizeof(*c.timings));
    c.timings->distance_ms = ms;
    c.timings->total_ms = ms;
    c.timings->n_units = g.total;
    c.timings->distance_launches = 1;
  }
  return M2S_OK;
}
