// band_shapes.hip — m2s_band_from_capsules: a resident band field of a union of capsules (spheres where a == b), with no mesh, gfx950.
// The contract is include/m2s.h's (per grid point, to the bit); shape.hip.h holds the distance and the index box with their error
// argument; tests/band_shapes_model.py restates both in numpy.  Nothing sized 4 bytes per grid point exists: the
// result's three index words per 64 points, its values, and per shape a record, a row count and its running sum (72 bytes).
//
//   k_sh_prepare   one lane per shape: whether it is sound, shape.hip.h's index box of its reach r + exterior, and the (i, j) rows in it.
//   the scan       scan.hip.h's k_tile_sums, k_scan_tiles and k_col_scan: S, the running sums of the row counts; S[n] = all rows.
//   k_sh_rows<0>   three bit planes by 64-bit atomic OR: near (d_s <= exterior) into the result's mask, inside (d_s < 0) into its sign
//                  mask, deep (d_s < -interior) into its word_off array, which has no other use until the offsets are known.
//                  The work items are ROWS of the shapes' boxes, not shapes: one ball of 400 cells' radius among a million small ones
//                  is 640 000 items among theirs.  A wave takes kShChunk consecutive rows at a time: one binary search in S for the
//                  first, then it steps through S.  Lanes run along k in chunks of 64 points that are aligned with the mask words;
//                  every point of the box is evaluated with the exact d_s (the box is only a superset); one ballot per plane and one
//                  atomic per touched word from lane 0.  A shape with a near point sets its hit flag (a plain store of 1).
//   k_sh_mask      band_walk.hip.h's units: mask = near & ~deep in place, the unit's popcount published, n_inside summed.
//   k_scan_tiles   the group sums; the total is the result's cell count, read by the host with the one synchronisation before the
//                  values are allocated at their true size.  k_sh_offsets writes word_off over the deep plane meanwhile, k_sh_tally
//                  counts the sound shapes without a hit.
//   k_sh_rows<1>   the same rows again: a point whose mask bit is set and whose d_s <= exterior takes an integer atomicMin of
//                  shape.hip.h's order-preserving key of d_s at word_off + rank, on values pre-filled with the key of +inf.  An active
//                  point has no deep shape and at least one near one, and every shape that is not near lies above all that are: the
//                  minimum over the near shapes is D.  An integer minimum is the same in any arrival order.
//   k_sh_decode    the keys back to floats, in place.
// All atomics are vector atomics on device memory; every loop that holds a ballot or a readlane is wave-uniform.
#include "../../include/m2s.h"
#include "band_handle.h"
#include "band_walk.hip.h"
#include "capi_internal.h"
#include "common.h"
#include "scan.hip.h"
#include "shape.hip.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace m2s {
namespace {

constexpr int kShGroup = 16;             // units per scanned sum, as band_csg.hip
constexpr int kShScanThreads = 1024;     // the one workgroup that scans the group sums and the tile sums
constexpr uint64_t kShChunk = 16;        // consecutive rows a wave takes per search in S
constexpr unsigned kShRowBlocks = 2048;  // 8192 waves share the rows: 8 per SIMD of the chip

struct ShGrid {
  float first[3], size[3];
  uint32_t cnt[3];
  float grid_scale;
  float exterior, neg_interior;
};

// A shape after k_sh_prepare.  rows = nI * nj where the box is not empty.
struct ShRec {
  Capsule s;
  uint32_t i0, j0, nj, klo, khi;
  uint32_t sound;
};

// counters: [1] += shapes that are not sound.
__global__ void __launch_bounds__(256) k_sh_prepare(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ radius, float r_all,
                                                    uint64_t n, ShGrid G, ShRec* __restrict__ recs, uint64_t* __restrict__ rows,
                                                    uint32_t* __restrict__ hit, uint64_t* __restrict__ counters) {
  for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (uint64_t)gridDim.x * 256) {
    ShRec r;
    const float* pb = b ? b : a;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      r.s.a[m] = a[3 * idx + m];
      r.s.b[m] = pb[3 * idx + m];
    }
    r.s.r = radius ? radius[idx] : r_all;
    r.sound = shape_sound(r.s) ? 1u : 0u;
    r.i0 = r.j0 = r.nj = r.klo = r.khi = 0;
    uint64_t nrows = 0;
    if (r.sound) {
      uint32_t lo[3], hi[3];
      shape_box(r.s, G.first, G.size, G.cnt, G.exterior, G.grid_scale, lo, hi);
      if (lo[0] < hi[0] && lo[1] < hi[1] && lo[2] < hi[2]) {
        r.i0 = lo[0];
        r.j0 = lo[1];
        r.nj = hi[1] - lo[1];
        r.klo = lo[2];
        r.khi = hi[2];
        nrows = (uint64_t)(hi[0] - lo[0]) * (uint64_t)r.nj;
      }
    } else {
      atomicAdd((unsigned long long*)(counters + 1), 1ull);
    }
    recs[idx] = r;
    rows[idx] = nrows;
    hit[idx] = 0;
  }
}

// counters: [3] += sound shapes without a hit.
__global__ void __launch_bounds__(256) k_sh_tally(const ShRec* __restrict__ recs, const uint32_t* __restrict__ hit, uint64_t n, uint64_t* __restrict__ counters) {
  uint32_t off = 0;
  for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (uint64_t)gridDim.x * 256) off += (recs[idx].sound && !hit[idx]) ? 1u : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) off += __shfl_xor(off, o, 64);
  if ((threadIdx.x & 63) == 0 && off) atomicAdd((unsigned long long*)(counters + 3), (unsigned long long)off);
}

// VALUES false: the three planes and the hit flags.  VALUES true: mask and word_off are the finished index, keys the values' keys (cap of them).
// S: n + 1 running sums of the row counts.  Everything but `lane`, the point and its distance is wave-uniform.
template <bool VALUES>
__global__ void __launch_bounds__(kWalkThreads) k_sh_rows(const ShRec* __restrict__ recs, const uint64_t* __restrict__ S, uint64_t n, ShGrid G, WalkGrid g,
                                                        uint64_t* mask, uint64_t* inside, uint64_t* word_off, uint32_t* hit, uint32_t* keys, uint64_t cap) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * kWalkWaves + (uint64_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t n_waves = (uint64_t)gridDim.x * kWalkWaves;
  const uint64_t total_rows = S[n];
  const uint64_t n_chunks = (total_rows + kShChunk - 1) / kShChunk;
  for (uint64_t chunk = wave; chunk < n_chunks; chunk += n_waves) {
    const uint64_t item0 = chunk * kShChunk, item1 = item0 + kShChunk < total_rows ? item0 + kShChunk : total_rows;
    uint64_t s = 0, top = n;   // the last shape whose rows begin at or before item0: S[s] <= item0 < S[s + 1]
    while (top - s > 1) {
      const uint64_t mid = s + ((top - s) >> 1);
      if (S[mid] <= item0) s = mid;
      else top = mid;
    }
    uint64_t s_begin = S[s], s_end = S[s + 1];
    ShRec r = recs[s];
    bool any = false;
    for (uint64_t item = item0; item < item1; ++item) {
      if (item >= s_end) {
        if (!VALUES && any && lane == 0) hit[s] = 1u;
        any = false;
        do {   // item < S[n]: the step ends at a shape that has rows, at most n - 1
          ++s;
          s_begin = s_end;
          s_end = S[s + 1];
        } while (item >= s_end);
        r = recs[s];
      }
      const uint64_t q = item - s_begin;
      const uint64_t qi = q / r.nj;
      const uint32_t i = r.i0 + (uint32_t)qi, j = r.j0 + (uint32_t)(q - qi * r.nj);
      const float cx = cell_center(G.first[0], G.size[0], i), cy = cell_center(G.first[1], G.size[1], j);
      const uint64_t Lr = ((uint64_t)i * g.ny + j) * g.nz;
      const uint64_t L_lo = Lr + r.klo, L_hi = Lr + r.khi;   // klo < khi <= nz: inside the grid
      for (uint64_t w = L_lo >> 6; w <= (L_hi - 1) >> 6; ++w) {
        const uint64_t L = (w << 6) + (uint64_t)lane;
        const bool in = L >= L_lo && L < L_hi;
        float d = 0.0f;
        if (in) d = shape_dist(r.s, cx, cy, cell_center(G.first[2], G.size[2], (uint32_t)(L - Lr)));
        const bool near = in && d <= G.exterior;
        const uint64_t bn = __ballot(near);
        if (!bn) continue;
        if (!VALUES) {
          const uint64_t bi = __ballot(in && d < 0.0f), bd = __ballot(in && d < G.neg_interior);
          any = true;
          if (lane == 0) {
            atomicOr((unsigned long long*)(mask + w), (unsigned long long)bn);
            if (bi) atomicOr((unsigned long long*)(inside + w), (unsigned long long)bi);
            if (bd) atomicOr((unsigned long long*)(word_off + w), (unsigned long long)bd);
          }
        } else {
          const uint64_t m = mask[w];
          if (!(m & bn)) continue;
          const uint64_t pos = word_off[w] + (uint64_t)__popcll(m & walk_below(lane));
          if (near && ((m >> lane) & 1ull) && pos < cap) atomicMin(keys + pos, shape_key(d));
        }
      }
    }
    if (!VALUES && any && lane == 0) hit[s] = 1u;
  }
}

// mask: near in, near & ~deep out.  deep: the plane in the word_off array.  counters[2] += the set bits of inside.
__global__ void __launch_bounds__(kWalkThreads) k_sh_mask(uint64_t n_words, uint64_t* __restrict__ mask, const uint64_t* __restrict__ deep,
                                                        const uint64_t* __restrict__ inside, uint32_t* __restrict__ unit_cnt,
                                                        uint64_t* __restrict__ group_sum, uint64_t* __restrict__ counters) {
  WALK_UNIT_HEAD(kWalkSteps, n_words)
  uint64_t cnt = 0, nin = 0;
  for (int step = 0; step < kWalkSteps; ++step) {
    WALK_STEP_HEAD(n_words)
    if (in_range) {
      const uint64_t m = mask[w] & ~deep[w];
      mask[w] = m;
      cnt += (uint64_t)__popcll(m);
      nin += (uint64_t)__popcll(inside[w]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nin += __shfl_xor(nin, o, 64);
  if (lane == 0 && nin) atomicAdd((unsigned long long*)(counters + 2), (unsigned long long)nin);
  walk_publish<kShGroup>(cnt, lane, unit, unit_cnt, group_sum);
}

// group_base: the scanned group sums.
__global__ void __launch_bounds__(kWalkThreads) k_sh_offsets(uint64_t n_words, const uint64_t* __restrict__ mask, const uint32_t* __restrict__ unit_cnt,
                                                           const uint64_t* __restrict__ group_base, uint64_t* __restrict__ word_off) {
  WALK_UNIT_HEAD(kWalkSteps, n_words)
  uint64_t base = walk_unit_base<kShGroup>(lane, unit, unit_cnt, group_base);
  for (int step = 0; step < kWalkSteps; ++step) {
    WALK_STEP_HEAD(n_words)
    const uint64_t m = in_range ? mask[w] : 0;
    const uint64_t off = walk_word_off((uint64_t)__popcll(m), lane, base);
    if (in_range) word_off[w] = off;
  }
}

__global__ void __launch_bounds__(256) k_sh_decode(uint32_t* __restrict__ keys, uint64_t n) {
  for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (uint64_t)gridDim.x * 256)
    keys[idx] = __float_as_uint(shape_unkey(keys[idx]));
}

// Device memory of a MEM_DEVICE caller must be reachable from the call's device: memory of another device is refused, and so is a
// pointer the runtime does not know (a host array passed as device memory).
int sh_device_pointer(const void* p, int device, const char* name) {
  if (!p) return 0;
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof(at));
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return fail(M2S_ERR_BAD_ARG, "%s is not device memory (mem_kind is M2S_MEM_DEVICE)", name);
  }
  if (at.type == hipMemoryTypeUnregistered) return fail(M2S_ERR_BAD_ARG, "%s is not device memory (mem_kind is M2S_MEM_DEVICE)", name);
  if (at.type == hipMemoryTypeDevice && at.device != device)
    return fail(M2S_ERR_BAD_ARG, "%s lives on device %d, the call runs on device %d", name, at.device, device);
  return 0;
}

}  // namespace

// m2s_warmup: the first launch of a kernel of this translation unit makes the runtime load its code object (all its kernels).
__global__ void k_warm_band_shapes() {}
void warm_band_shapes(hipStream_t st) { hipLaunchKernelGGL(k_warm_band_shapes, dim3(1), dim3(64), 0, st); }

}  // namespace m2s

using namespace m2s;

extern "C" {

int m2s_band_from_capsules(const m2s_grid* grid, const float* a, const float* b, const float* radius, uint64_t n, const m2s_band_shapes_opts* sopts,
                           const m2s_band_field_opts* fopts, const m2s_opts* opts, m2s_band** out, m2s_band_shapes_info* info, m2s_timings* timings) {
  clear_error();
  if (!out) return fail(M2S_ERR_BAD_ARG, "out is NULL");
  *out = nullptr;
  if (!grid) return fail(M2S_ERR_BAD_ARG, "grid is NULL");
  if (!sopts) return fail(M2S_ERR_BAD_ARG, "m2s_band_shapes_opts is NULL: the widths have no default");
  if (sopts->struct_size != sizeof(m2s_band_shapes_opts))
    return fail(M2S_ERR_BAD_ARG, "m2s_band_shapes_opts.struct_size is not sizeof(m2s_band_shapes_opts)");
  if (!good_background(sopts->exterior) || !good_background(sopts->interior))
    return fail(M2S_ERR_BAD_ARG, "the half-widths (%g exterior, %g interior) must be >= 0 and finite", (double)sopts->exterior, (double)sopts->interior);
  if (!good_background(sopts->radius)) return fail(M2S_ERR_BAD_ARG, "m2s_band_shapes_opts.radius = %g must be >= 0 and finite", (double)sopts->radius);
  int rc = band_field_opts_args(fopts);
  if (rc) return rc;
  if (n && !a) return fail(M2S_ERR_BAD_ARG, "a is NULL with n > 0");
  if (n >= ((uint64_t)1 << 32)) return fail(M2S_ERR_BAD_ARG, "n = %llu: at most 2^32 - 1 shapes", (unsigned long long)n);
  rc = band_opts_args(opts, "m2s_band_from_capsules");
  if (rc) return rc;
  GridQuery gq;
  int ignored = 0;
  rc = grid_query_args(grid, nullptr, false, nullptr, &gq, &ignored);   // what m2s_band_create rejects of a grid
  if (rc) return rc;
  uint64_t total = 0, n_words = 0;
  rc = band_grid_cells(grid, "grid", &total, &n_words);
  if (rc) return rc;
  ShGrid G;
  for (int m = 0; m < 3; ++m) {
    if (grid->cell_count[m] >= ((uint64_t)1 << 32)) return fail(M2S_ERR_BAD_ARG, "cell_count[%d] = %llu: at most 2^32 - 1 per axis", m, (unsigned long long)grid->cell_count[m]);
    G.first[m] = grid->first_cell[m];
    G.size[m] = grid->cell_size[m];
    G.cnt[m] = (uint32_t)grid->cell_count[m];
  }
  G.grid_scale = shape_grid_scale(G.first, G.size, G.cnt);
  G.exterior = sopts->exterior;
  G.neg_interior = -sopts->interior;
  const float bg_out = fopts ? fopts->background_outside : sopts->exterior;
  const float bg_in = fopts ? fopts->background_inside : sopts->interior;
  const WalkGrid g = walk_grid_of(grid->cell_count, total, n_words);

  m2s_opts o = m2s_opts{};
  if (opts) memcpy(&o, opts, (opts->struct_size >= sizeof(m2s_opts)) ? sizeof(m2s_opts) : (size_t)M2S_OPTS_V1_SIZE);
  else o.device = -1;
  o.synchronous = 1;
  if (timings) o.timings = timings;
  CallCtx c;
  DeviceState* st = nullptr;
  rc = resolve_ctx(&o, &c, &st);
  if (rc) return rc;
  const bool host = c.mem_kind == M2S_MEM_HOST;
  if (!host && n) {
    if ((rc = sh_device_pointer(a, c.device, "a")) || (rc = sh_device_pointer(b, c.device, "b")) || (rc = sh_device_pointer(radius, c.device, "radius")))
      return rc;
  }

  const uint64_t n_units = (n_words + kWalkUnit - 1) / kWalkUnit;   // below 2^22: a grid has fewer than 2^36 cells
  const uint64_t n_groups = (n_units + kShGroup - 1) / kShGroup;
  const unsigned unit_blocks = (unsigned)((n_units + kWalkWaves - 1) / kWalkWaves);
  const uint32_t tiles = tiles_of((size_t)n);
  BandBlock res;   // the result: its three index arrays now, its values once the count is known
  auto drop = [&](int code) {
    res.free();
    return code;
  };
  auto hip_fail = [&](hipError_t e) { return drop(fail(M2S_ERR_HIP, "HIP error: %s", hipGetErrorString(e))); };
  size_t need = 4096 + 256 + align_up((size_t)n_units * 4) + align_up((size_t)n_groups * 8);
  need += align_up((size_t)n * sizeof(ShRec)) + align_up((size_t)n * 8) + align_up(((size_t)n + 1) * 8) + align_up((size_t)n * 4) + align_up((size_t)tiles * 8 + 8);
  if (host) need += 2 * align_up((size_t)n * 12) + align_up((size_t)n * 4);
  rc = ensure_capacity(*st, need);
  if (rc) return rc;
  Arena ws{st->base, st->cap, 0};
  uint64_t* d_hdr = ws.take<uint64_t>(8);   // [0] the cell count (the scan's total), [1] n_skipped, [2] n_inside, [3] n_off_grid, [4] the tile scan's total
  uint32_t* unit_cnt = ws.take<uint32_t>(n_units);
  uint64_t* group_sum = ws.take<uint64_t>(n_groups);
  ShRec* recs = ws.take<ShRec>(n);
  uint64_t* rows = ws.take<uint64_t>(n);
  uint64_t* S = ws.take<uint64_t>(n + 1);
  uint32_t* hit = ws.take<uint32_t>(n);
  uint64_t* tile_sum = ws.take<uint64_t>((size_t)tiles + 1);
  if (!d_hdr || !unit_cnt || !group_sum || !recs || !rows || !S || !hit || !tile_sum) return fail(M2S_ERR_HIP, "internal: workspace");
  hipStream_t s = c.stream;
  const float *da = a, *db = b, *dr = radius;
  if (host && n) {   // the shapes of a host caller, staged in the workspace
    char* sa = ws.take<char>(n * 12);
    char* sb = b ? ws.take<char>(n * 12) : nullptr;
    char* sr = radius ? ws.take<char>(n * 4) : nullptr;
    if (!sa || (b && !sb) || (radius && !sr)) return fail(M2S_ERR_HIP, "internal: workspace");
    if ((rc = staged_h2d(*st, s, sa, reinterpret_cast<const char*>(a), n * 12))) return rc;
    if (b && (rc = staged_h2d(*st, s, sb, reinterpret_cast<const char*>(b), n * 12))) return rc;
    if (radius && (rc = staged_h2d(*st, s, sr, reinterpret_cast<const char*>(radius), n * 4))) return rc;
    da = reinterpret_cast<const float*>(sa);
    db = reinterpret_cast<const float*>(sb);
    dr = reinterpret_cast<const float*>(sr);
  }
  hipError_t e = res.alloc_index(n_words);
  if (e != hipSuccess) return hip_fail(e);

  // ---- the boxes, the planes, the mask and its offsets ----
  if (c.timings) e = hipEventRecord(st->ev[0], s);
  if (e == hipSuccess) e = hipMemsetAsync(d_hdr, 0, 64, s);
  if (e == hipSuccess) e = hipMemsetAsync(res.mask, 0, 3 * align_up(n_words * 8), s);   // near, deep (in word_off) and inside
  if (e != hipSuccess) return hip_fail(e);
  uint64_t hdr[4] = {0, 0, 0, 0};
  if (n) {
    if ((e = hipMemsetAsync(group_sum, 0, n_groups * 8, s)) != hipSuccess) return hip_fail(e);
    hipLaunchKernelGGL(k_sh_prepare, dim3(blocks_for(n)), dim3(256), 0, s, da, db, dr, sopts->radius, n, G, recs, rows, hit, d_hdr);
    hipLaunchKernelGGL(k_tile_sums<false>, dim3(tiles), dim3(kTileThreads), 0, s, (const void*)rows, (size_t)n, tile_sum);
    hipLaunchKernelGGL((k_scan_tiles<kShScanThreads, uint32_t>), dim3(1), dim3(kShScanThreads), 0, s, tile_sum, tiles, d_hdr + 4);
    hipLaunchKernelGGL(k_col_scan<uint64_t>, dim3(tiles), dim3(kTileThreads), 0, s, (const uint64_t*)rows, n, (const uint64_t*)tile_sum, S);
    hipLaunchKernelGGL(k_sh_rows<false>, dim3(kShRowBlocks), dim3(kWalkThreads), 0, s, (const ShRec*)recs, (const uint64_t*)S, n, G, g, res.mask, res.inside,
                       res.word_off, hit, (uint32_t*)nullptr, (uint64_t)0);
    hipLaunchKernelGGL(k_sh_mask, dim3(unit_blocks), dim3(kWalkThreads), 0, s, n_words, res.mask, (const uint64_t*)res.word_off, (const uint64_t*)res.inside,
                       unit_cnt, group_sum, d_hdr);
    hipLaunchKernelGGL((k_scan_tiles<kShScanThreads, uint64_t>), dim3(1), dim3(kShScanThreads), 0, s, group_sum, n_groups, d_hdr);
    hipLaunchKernelGGL(k_sh_offsets, dim3(unit_blocks), dim3(kWalkThreads), 0, s, n_words, (const uint64_t*)res.mask, (const uint32_t*)unit_cnt,
                       (const uint64_t*)group_sum, res.word_off);
    hipLaunchKernelGGL(k_sh_tally, dim3(std::min(1024u, blocks_for(n))), dim3(256), 0, s, (const ShRec*)recs, (const uint32_t*)hit, n, d_hdr);
    e = hipGetLastError();
  }
  if (e == hipSuccess && c.timings) e = hipEventRecord(st->ev[1], s);
  if (e == hipSuccess && n) e = hipMemcpyAsync(hdr, d_hdr, 32, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);   // the call's one synchronisation before its end: the count sizes the values
  if (e != hipSuccess) return hip_fail(e);
  const uint64_t n_cells = hdr[0];
  if (n_cells > g.total) return drop(fail(M2S_ERR_HIP, "internal: the result has %llu cells, the grid %llu", (unsigned long long)n_cells, (unsigned long long)g.total));
  const uint64_t cap = std::max<uint64_t>(n_cells, 1);   // at least one float: a lane's guarded read needs an address
  e = res.alloc_values(cap);
  if (e != hipSuccess) return hip_fail(e);

  // ---- the values ----
  if (c.timings) e = hipEventRecord(st->ev[2], s);
  if (e == hipSuccess) e = hipMemsetAsync(res.dist, 0, 4, s);   // an empty result still has one defined float
  if (e != hipSuccess) return hip_fail(e);
  if (n_cells) {
    uint32_t* keys = reinterpret_cast<uint32_t*>(res.dist);
    e = hipMemsetD32Async((hipDeviceptr_t)keys, (int)SHAPE_KEY_INF, (size_t)n_cells, s);
    if (e != hipSuccess) return hip_fail(e);
    hipLaunchKernelGGL(k_sh_rows<true>, dim3(kShRowBlocks), dim3(kWalkThreads), 0, s, (const ShRec*)recs, (const uint64_t*)S, n, G, g, res.mask, res.inside,
                       res.word_off, (uint32_t*)nullptr, keys, n_cells);
    hipLaunchKernelGGL(k_sh_decode, dim3(blocks_for(n_cells)), dim3(256), 0, s, keys, n_cells);
    e = hipGetLastError();
  }
  if (e == hipSuccess && c.timings) e = hipEventRecord(st->ev[3], s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);   // the end of the call: the result is complete when it returns
  if (e != hipSuccess) return hip_fail(e);
  if (c.timings) {
    float plane_ms = 0.0f, value_ms = 0.0f, all_ms = 0.0f;
    (void)hipEventElapsedTime(&plane_ms, st->ev[0], st->ev[1]);
    (void)hipEventElapsedTime(&value_ms, st->ev[2], st->ev[3]);
    (void)hipEventElapsedTime(&all_ms, st->ev[0], st->ev[3]);
    memset(c.timings, 0, sizeof(*c.timings));
    c.timings->seed_ms = plane_ms;
    c.timings->distance_ms = value_ms;
    c.timings->total_ms = all_ms;
    c.timings->n_units = n_cells;
    c.timings->n_triangles = n - hdr[1];
    c.timings->distance_launches = n_cells ? 1 : 0;
  }
  if (info) {
    info->n_cells = n_cells;
    info->n_inside = hdr[2];
    info->n_skipped = hdr[1];
    info->n_off_grid = hdr[3];
  }
  *out = band_adopt(res, c.device, *grid, n_cells, g.total, n_words, bg_out, bg_in);
  return M2S_OK;
}

}  // extern "C"
