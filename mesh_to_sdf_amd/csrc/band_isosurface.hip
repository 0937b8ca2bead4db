// band_isosurface.hip — m2s_band_isosurface: the welded, indexed mesh of a level set straight from a narrow band (an ascending list of
// grid points and their values), gfx950.  The contract is include/m2s.h's: the dense m2s_grid_isosurface of any grid that agrees with
// the band on its points, filtered to the vertices whose edge has both ends in the band and the triangles whose cell has all eight
// corners in it.  tests/band_isosurface_model.py restates it in numpy and the GPU tests compare the two bit for bit.
//
// The work is per band cell; nothing reads or writes an array of distances sized by the grid.  Sized by the grid are the mask (one bit
// per point) and one 64-bit list offset per mask word, of which only the words that hold a band cell are ever written or read.
// Passes:
//   k_biso_mask       per band cell: strictly ascending and below the cell count (else flag bit 0), a finite value (else flag bit 1), its
//                     bit in the zeroed mask — the bits of the lanes of one word are OR-ed along the wave first, one atomicOr per run —
//                     and, from the first cell of each word, word_off[w] = its place in the list (the list is sorted: no scan).
//   k_biso_info       per band cell: the 7 other corners of its cell by mask + rank (isosurface.hip.h active_index) — the upper z-neighbour
//                     of a corner already found is the next list entry or absent, no lookup; an edge flag only where the far end is in
//                     the band and the edge crosses, the case only where all 8 corners are; n_open; per block of 4096 cells the vertex
//                     and triangle sums.
//   k_scan_tiles      the block sums, twice: the counts the call returns.  A count-only call stops here.
//   k_biso_vertices   per band cell: its first vertex id (u32) and its vertices' positions.
//   k_biso_triangles  per complete cell: its triangles; an edge owned by another point finds that point by mask + rank.
// In all three a wave's lanes hold neighbouring list entries (the two emitting kernels scan 256 entries at a time, 16 times per block, where
// the dense extractor gives each lane 16 entries in a row): neighbouring entries are neighbouring grid points, so their mask words, list
// places and outputs share cache lines.  Measured on k_biso_info at 1024^3: 1982 -> 299 us.
// Every kernel after the first leaves at once when the flag is raised, so a list that is not ascending or runs past the grid is never used
// as an index: k_biso_mask itself writes only at L < total.
// Shared with isosurface.hip through isosurface.hip.h: the table, IsoGrid, decode, active_index, and scan.hip.h's workgroup scan and k_scan_tiles; and with
// band_query.hip (the resident index of m2s_band_create): k_biso_mask and its flags, which live there too.  Copied
// from it, because there they are written into the bodies of kernels that read a dense grid: the vertex arithmetic of k_iso_vertices
// (operation for operation, under the same fp contract pragma), the triangle loop of k_iso_triangles and the grid checks of iso_args.
#include "../../include/m2s.h"
#include "capi_internal.h"
#include "common.h"
#include "isosurface.hip.h"

#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace m2s {
namespace {

// The place of grid point L (< total) in the band list, kNone if it is not in the band.
__device__ __forceinline__ uint64_t band_index(const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_off, uint64_t L, uint64_t n) {
  if (!((mask[L >> 6] >> (L & 63)) & 1ull)) return kNone;
  const uint64_t k = active_index(mask, word_off, L);
  return k < n ? k : kNone;   // k < n whenever the list ascends; the guard keeps a broken invariant in bounds
}

// Per band cell: info = (edge flags) | (case << 3), the case 0 unless all 8 corners are in the band; per block of kItemBlock cells the
// (vertex, triangle) sums; *n_open += the cells that are cut inside the band but incomplete.
__global__ void __launch_bounds__(kItemThreads) k_biso_info(IsoGrid g, const uint64_t* __restrict__ cells, const float* __restrict__ dist,
                                                            uint64_t n, const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_off,
                                                            const uint32_t* __restrict__ flag, uint32_t* __restrict__ info,
                                                            uint64_t* __restrict__ vsum, uint64_t* __restrict__ tsum,
                                                            unsigned long long* __restrict__ n_open) {
  if (*flag) {   // the whole workgroup
    if (threadIdx.x == 0) vsum[blockIdx.x] = tsum[blockIdx.x] = 0;
    return;
  }
  // only the block's sums leave this kernel, so neighbouring lanes take neighbouring cells: their mask words and list places are close
  const uint64_t b = (uint64_t)blockIdx.x * kItemBlock + threadIdx.x;
  uint64_t nv = 0, nt = 0, no = 0;
  for (int r = 0; r < kItemsPerThread; ++r) {
    const uint64_t a = b + (uint64_t)r * kItemThreads;
    if (a >= n) break;
    const uint64_t L = cells[a];
    const Pt p = decode(g, L);
    const bool ex = p.i + 1 < g.n[0], ey = p.j + 1 < g.n[1], ez = p.k + 1 < g.n[2];
    const bool cell = ex && ey && ez;
    // corner c = 4 dx + 2 dy + dz, as in the case; corners 3, 5, 6, 7 matter to a cell only
    const bool exists[8] = {true, ez, ey, cell, ex, cell, cell, cell};
    uint64_t at[8];
#pragma unroll
    for (int c = 0; c < 8; c += 2) {
      const uint64_t Lc = L + (c & 4 ? g.nyz : 0) + (c & 2 ? g.n[2] : 0);
      at[c] = c == 0 ? a : (exists[c] ? band_index(mask, word_off, Lc, n) : kNone);
      // the upper z-neighbour of a band cell is the next entry of the list or not in it (the list ascends): no mask, no rank
      if (!exists[c + 1]) at[c + 1] = kNone;
      else if (at[c] != kNone) at[c + 1] = at[c] + 1 < n && cells[at[c] + 1] == Lc + 1 ? at[c] + 1 : kNone;
      else at[c + 1] = band_index(mask, word_off, Lc + 1, n);
    }
    const float iso = g.iso;
    uint32_t have = 0, in = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (at[c] == kNone) continue;
      have |= 1u << c;
      in |= (uint32_t)(dist[at[c]] < iso) << c;
    }
    const uint32_t i000 = in & 1u;
    const uint32_t flags = (uint32_t)(((have >> 4) & 1u) && ((in >> 4) & 1u) != i000) | ((uint32_t)(((have >> 2) & 1u) && ((in >> 2) & 1u) != i000) << 1) |
                           ((uint32_t)(((have >> 1) & 1u) && ((in >> 1) & 1u) != i000) << 2);
    const uint32_t cs = have == 255u ? in : 0u;
    if (cell && have != 255u && in != 0u && in != have) ++no;
    info[a] = flags | (cs << 3);
    nv += __popc(flags);
    nt += kIsoTriCount[cs];
  }
  uint64_t tv, tt, to;
  (void)block_exclusive_scan<kItemThreads>(nv, &tv);
  (void)block_exclusive_scan<kItemThreads>(nt, &tt);
  (void)block_exclusive_scan<kItemThreads>(no, &to);
  if (threadIdx.x == 0) {
    vsum[blockIdx.x] = tv;
    tsum[blockIdx.x] = tt;
    if (to) atomicAdd(n_open, (unsigned long long)to);
  }
}

// First vertex id of each band cell (n_vertices < 2^32 is checked before this runs) and the positions of its vertices.
__global__ void __launch_bounds__(kItemThreads) k_biso_vertices(IsoGrid g, const uint64_t* __restrict__ cells, const float* __restrict__ dist,
                                                                uint64_t n, const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_off,
                                                                const uint32_t* __restrict__ info, const uint64_t* __restrict__ voff_block,
                                                                uint32_t* __restrict__ voff, float* __restrict__ vout) {
  // kItemsPerThread rounds of kItemThreads neighbouring cells, one per lane, each round scanned on its own: the order of the output is
  // the order of the list, and the lanes of a wave read and write neighbouring places
  const uint64_t b = (uint64_t)blockIdx.x * kItemBlock;
  uint64_t base = voff_block[blockIdx.x];
  for (int r = 0; r < kItemsPerThread && b + (uint64_t)r * kItemThreads < n; ++r) {   // the same for the whole workgroup
    const uint64_t a = b + (uint64_t)r * kItemThreads + threadIdx.x;
    const uint32_t flags = a < n ? info[a] & 7 : 0;
    uint64_t all;
    uint64_t v = base + block_exclusive_scan<kItemThreads>((uint64_t)__popc(flags), &all);
    base += all;
    if (a < n) voff[a] = (uint32_t)v;
    if (!flags) continue;
    const uint64_t L = cells[a];
    const Pt p = decode(g, L);
    const float d0 = dist[a];
    // pos = first + (float)i * cs per axis (m2s_grid_cell_center)
    const float px = g.first[0] + (float)p.i * g.cs[0];
    const float py = g.first[1] + (float)p.j * g.cs[1];
    const float pz = g.first[2] + (float)p.k * g.cs[2];
    const uint64_t step[3] = {g.nyz, g.n[2], 1};
    const uint64_t idx[3] = {p.i, p.j, p.k};
    for (int ax = 0; ax < 3; ++ax) {
      if (!((flags >> ax) & 1)) continue;
      const uint64_t far = band_index(mask, word_off, L + step[ax], n);   // in the band: the flag says so
      const float d1 = dist[far != kNone ? far : a];
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

__global__ void __launch_bounds__(kItemThreads) k_biso_triangles(IsoGrid g, const uint64_t* __restrict__ cells, uint64_t n,
                                                                 const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_off,
                                                                 const uint32_t* __restrict__ info, const uint32_t* __restrict__ voff,
                                                                 const uint64_t* __restrict__ toff_block, uint32_t* __restrict__ tout) {
  const uint64_t b = (uint64_t)blockIdx.x * kItemBlock;   // rounds as in k_biso_vertices
  uint64_t base = toff_block[blockIdx.x];
  for (int r = 0; r < kItemsPerThread && b + (uint64_t)r * kItemThreads < n; ++r) {
    const uint64_t a = b + (uint64_t)r * kItemThreads + threadIdx.x;
    const uint32_t cs = a < n ? (info[a] >> 3) & 255 : 0;
    const int count = kIsoTriCount[cs];
    uint64_t all;
    uint64_t t = base + block_exclusive_scan<kItemThreads>((uint64_t)count, &all);
    base += all;
    if (!count) continue;
    const uint64_t L = cells[a];
    for (int tri = 0; tri < count; ++tri) {
      uint32_t id[3];
      for (int c = 0; c < 3; ++c) {
        const int e = kIsoTris[cs][tri * 3 + c];
        const int ax = e >> 2;
        const uint64_t owner = L + kIsoEdgeOffset[e][0] * g.nyz + kIsoEdgeOffset[e][1] * g.n[2] + kIsoEdgeOffset[e][2];
        const uint64_t k = owner == L ? a : band_index(mask, word_off, owner, n);
        // the cell is complete, so the owner and the edge's far end are in the band and the owner has flagged the edge
        if (k != kNone && cells[k] == owner) id[c] = voff[k] + (uint32_t)__popc(info[k] & 7 & ((1u << ax) - 1));
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
int biso_args(const m2s_grid* grid, const uint64_t* cells, const float* distances, uint64_t n_cells, float iso, float* vertices_out,
              uint32_t* indices_out, uint64_t* counts, const m2s_opts* opts, IsoGrid* g) {
  if (!grid || !counts) return fail(M2S_ERR_BAD_ARG, "grid / counts is NULL");
  if (n_cells && (!cells || !distances)) return fail(M2S_ERR_BAD_ARG, "cells / distances is NULL with n_cells > 0");
  if ((vertices_out == nullptr) != (indices_out == nullptr)) return fail(M2S_ERR_BAD_ARG, "vertices_out and indices_out must both be NULL or both set");
  if (opts) {
    if (opts->algorithm != 0 || opts->x_begin != 0 || opts->x_end != 0)
      return fail(M2S_ERR_BAD_ARG, "m2s_opts.algorithm / x_begin / x_end must be 0 for m2s_band_isosurface");
    if (opts->struct_size >= sizeof(m2s_opts) && (opts->x_period != 0 || opts->n_peer_out != 0 || opts->peer_out))
      return fail(M2S_ERR_BAD_ARG, "m2s_opts.x_period / peer_out must be 0 for m2s_band_isosurface");
    if (opts->mem_kind != M2S_MEM_HOST && opts->mem_kind != M2S_MEM_DEVICE) return fail(M2S_ERR_BAD_ARG, "bad mem_kind");
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
  if (g->nyz / g->n[1] != g->n[2]) return fail(M2S_ERR_BAD_ARG, "the grid has too many cells");
  g->total = g->nyz * g->n[0];
  if (g->total / g->n[0] != g->nyz || g->total >= ((uint64_t)1 << 36)) return fail(M2S_ERR_BAD_ARG, "the grid has 2^36 or more cells");
  g->iso = iso;
  if (n_cells > g->total) return fail(M2S_ERR_BAD_ARG, "n_cells = %llu above the grid's %llu cells", (unsigned long long)n_cells, (unsigned long long)g->total);
  return 0;
}

}  // namespace
}  // namespace m2s

using namespace m2s;

int m2s_band_isosurface(const m2s_grid* grid, const uint64_t* cells, const float* distances, uint64_t n_cells, float iso, float* vertices_out,
                        uint64_t vertex_capacity, uint32_t* indices_out, uint64_t triangle_capacity, uint64_t* counts, const m2s_opts* opts) {
  clear_error();
  IsoGrid g;
  int rc = biso_args(grid, cells, distances, n_cells, iso, vertices_out, indices_out, counts, opts, &g);
  if (rc) return rc;
  const bool host = !opts || opts->mem_kind == M2S_MEM_HOST;
  if (host)   // host memory: the list is judged here, before any device work
    for (uint64_t a = 0; a < n_cells; ++a)
      if (cells[a] >= g.total || (a && cells[a - 1] >= cells[a]))
        return fail(M2S_ERR_BAD_ARG, "cells[%llu] = %llu is not above its predecessor or not below the grid's %llu cells", (unsigned long long)a,
                    (unsigned long long)cells[a], (unsigned long long)g.total);
  counts[0] = counts[1] = counts[2] = 0;
  if (n_cells == 0) return M2S_OK;
  CallCtx c;
  DeviceState* st = nullptr;
  rc = resolve_ctx(opts, &c, &st);
  if (rc) return rc;
  const bool fill = vertices_out != nullptr;
  const uint64_t n = n_cells, n_words = (g.total + 63) / 64, n_blk = item_blocks(n);
  // [staged cells and values] hdr, the mask, the word offsets, info, first vertex ids, the block sums; then, sized once the counts are
  // known, [staged outputs]
  const size_t fixed = (host ? align_up(n * 8) + align_up(n * 4) : 0) + 256 + align_up(n_words * 8) * 2 + align_up(n * 4) * 2 + align_up(n_blk * 8) * 2 + 4096;
  size_t need = fixed;
  uint64_t hdr[4];   // the flag, n_vertices, n_triangles, n_open
  for (int attempt = 0;; ++attempt) {
    rc = ensure_capacity(*st, need);
    if (rc) return rc;
    Arena ws{st->base, st->cap, 0};
    const uint64_t* dc = cells;
    const float* dd = distances;
    if (host) {
      char* sc = ws.take<char>(n * 8);
      char* sd = ws.take<char>(n * 4);
      if (!sc || !sd) return fail(M2S_ERR_HIP, "internal: workspace");
      if ((rc = staged_h2d(*st, c.stream, sc, reinterpret_cast<const char*>(cells), n * 8))) return rc;
      if ((rc = staged_h2d(*st, c.stream, sd, reinterpret_cast<const char*>(distances), n * 4))) return rc;
      dc = reinterpret_cast<const uint64_t*>(sc);
      dd = reinterpret_cast<const float*>(sd);
    }
    uint64_t* d_hdr = ws.take<uint64_t>(4);
    uint64_t* mask = ws.take<uint64_t>(n_words);
    uint64_t* word_off = ws.take<uint64_t>(n_words);
    uint32_t* info = ws.take<uint32_t>(n);
    uint32_t* voff = ws.take<uint32_t>(n);
    uint64_t* vsum = ws.take<uint64_t>(n_blk);
    uint64_t* tsum = ws.take<uint64_t>(n_blk);
    if (!d_hdr || !mask || !word_off || !info || !voff || !vsum || !tsum) return fail(M2S_ERR_HIP, "internal: workspace");
    const uint32_t* flag = reinterpret_cast<const uint32_t*>(d_hdr);
    if (c.timings) M2S_HIP_CHECK(hipEventRecord(st->ev[0], c.stream));
    M2S_HIP_CHECK(hipMemsetAsync(d_hdr, 0, 32, c.stream));
    M2S_HIP_CHECK(hipMemsetAsync(mask, 0, n_words * 8, c.stream));
    hipLaunchKernelGGL(k_biso_mask, dim3((unsigned)((n + kMaskThreads - 1) / kMaskThreads)), dim3(kMaskThreads), 0, c.stream, g.total, dc, dd, n, mask,
                       word_off, reinterpret_cast<uint32_t*>(d_hdr));
    hipLaunchKernelGGL(k_biso_info, dim3((unsigned)n_blk), dim3(kItemThreads), 0, c.stream, g, dc, dd, n, (const uint64_t*)mask, (const uint64_t*)word_off,
                       flag, info, vsum, tsum, reinterpret_cast<unsigned long long*>(d_hdr + 3));
    hipLaunchKernelGGL((k_scan_tiles<kScanThreads, uint64_t>), dim3(1), dim3(kScanThreads), 0, c.stream, vsum, n_blk, d_hdr + 1);
    hipLaunchKernelGGL((k_scan_tiles<kScanThreads, uint64_t>), dim3(1), dim3(kScanThreads), 0, c.stream, tsum, n_blk, d_hdr + 2);
    M2S_HIP_CHECK(hipGetLastError());
    M2S_HIP_CHECK(hipMemcpyAsync(hdr, d_hdr, 32, hipMemcpyDeviceToHost, c.stream));
    M2S_HIP_CHECK(hipStreamSynchronize(c.stream));
    const uint32_t raised = (uint32_t)hdr[0];
    if (raised & kFlagOrder) return fail(M2S_ERR_BAD_ARG, "cells is not strictly ascending or holds an entry at or above the grid's cell count");
    if (raised & kFlagNonFinite) return fail(M2S_ERR_NAN, "the band holds a NaN or infinite distance");
    counts[0] = hdr[1];
    counts[1] = hdr[2];
    counts[2] = hdr[3];
    if (hdr[1] >= ((uint64_t)1 << 32)) return fail(M2S_ERR_BAD_ARG, "%llu vertices: u32 indices cannot address them", (unsigned long long)hdr[1]);
    if (fill && (vertex_capacity < hdr[1] || triangle_capacity < hdr[2]))
      return fail(M2S_ERR_BAD_ARG, "capacity (%llu vertices, %llu triangles) below the counts (%llu, %llu)", (unsigned long long)vertex_capacity,
                  (unsigned long long)triangle_capacity, (unsigned long long)hdr[1], (unsigned long long)hdr[2]);
    if (fill) {
      float* vdev = vertices_out;
      uint32_t* tdev = indices_out;
      if (host) {
        need = ws.off + align_up(hdr[1] * 12 + 4) + align_up(hdr[2] * 12 + 4) + 1024;
        if (need > st->cap) {
          if (attempt) return fail(M2S_ERR_HIP, "internal: workspace");
          continue;   // grow the workspace (which drops its contents) and start again: a second pass finds room
        }
        vdev = ws.take<float>(hdr[1] * 3 + 1);
        tdev = ws.take<uint32_t>(hdr[2] * 3 + 1);
        if (!vdev || !tdev) return fail(M2S_ERR_HIP, "internal: workspace");
      }
      hipLaunchKernelGGL(k_biso_vertices, dim3((unsigned)n_blk), dim3(kItemThreads), 0, c.stream, g, dc, dd, n, (const uint64_t*)mask,
                         (const uint64_t*)word_off, (const uint32_t*)info, (const uint64_t*)vsum, voff, vdev);
      hipLaunchKernelGGL(k_biso_triangles, dim3((unsigned)n_blk), dim3(kItemThreads), 0, c.stream, g, dc, n, (const uint64_t*)mask,
                         (const uint64_t*)word_off, (const uint32_t*)info, (const uint32_t*)voff, (const uint64_t*)tsum, tdev);
      M2S_HIP_CHECK(hipGetLastError());
      if (c.timings) M2S_HIP_CHECK(hipEventRecord(st->ev[1], c.stream));
      if (host) {
        if (hdr[1] && (rc = staged_d2h(*st, c.stream, reinterpret_cast<char*>(vertices_out), reinterpret_cast<const char*>(vdev), hdr[1] * 12)))
          return rc;
        if (hdr[2] && (rc = staged_d2h(*st, c.stream, reinterpret_cast<char*>(indices_out), reinterpret_cast<const char*>(tdev), hdr[2] * 12)))
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
    c.timings->n_units = n_cells;
    c.timings->distance_launches = 1;
  }
  return M2S_OK;
}
