// band_csg.hip — m2s_band_csg / m2s_band_export / m2s_band_field_info: union, intersection and difference of two resident bands, and a
// handle's lists back out, gfx950.  The contract is include/m2s.h's (the rules per grid point, to the bit); tests/band_csg_model.py
// restates it in numpy.  Nothing sized 4 bytes per grid point exists: the work is the index words of the operands plus their band cells.
//
// A CSG call is three launches over the mask words, band_walk.hip.h's walk and offsets.  A lane loads its word of all
// four index arrays (mask and sign mask of A and B), coalesced.
//   k_csg_mask   a word with maskA | maskB == 0 (the common case: a band is O(n^2) of n^3) is settled by its own lane: result mask 0,
//                result sign word = the op of the two sign words (B's complemented for A \ B).  In the others lane t reads its operand
//                values at their list places — contiguous runs —, takes the backgrounds by select and evaluates the rules; two ballots
//                are the result's mask word and sign word.  The unit's popcount is published.
//   k_scan_tiles the group sums; the total is the result's cell count, read by the host.
//   k_csg_emit   the same units: the result's word_off, and lane t of a word with active points stores r at word_off + rank.
// The unit is 256 words and the group 16 units (profiles/band_csg.txt has the measurements; DESIGN.md §4.16 the reasons).
// r is computed twice rather than kept: where it would go is known only after the scan, and a buffer of candidates would be the size
// of the result.  All stores are plain vector stores.
// Export: k_csg_cells (L = 64 w + bit at word_off + rank, the word taken by the wave as above), a copy of dist, and k_csg_unsign, the
// inverse of band_query.hip's k_bq_sign (one lane per output uint32: 32 bits of the sign mask from bit L0 on, over a word boundary
// where a row starts mid-word).
#include "../../include/m2s.h"
#include "band_handle.h"
#include "band_walk.hip.h"
#include "capi_internal.h"
#include "common.h"
#include "isosurface.hip.h"

#include <algorithm>
#include <cstring>

#pragma clang fp contract(off)

namespace m2s {
namespace {

constexpr int kCsgGroup = 16;                               // units per scanned sum

// D'_X at bit t of one mask word: the value, whether the band supplies it, and the sign s_X of the definition.  NEG: the same of -X.
struct CsgPoint {
  float x;
  bool act, s;
};
// The two backgrounds come as kernel arguments of their own: selecting between two neighbouring fields of the by-value BandDev made
// hipcc copy them to scratch and index that copy per point.
template <bool NEG>
__device__ __forceinline__ CsgPoint csg_point(const BandDev& X, float bg_out, float bg_in_neg, uint64_t m, uint64_t in, uint64_t wo, int t) {
  CsgPoint p;
  p.act = (m >> t) & 1ull;
  const bool ins = (in >> t) & 1ull;
  const uint64_t at = walk_rank(m, wo, t, X.n);
  float x = ins ? bg_in_neg : bg_out;
  if (p.act) x = X.dist[at];
  if (NEG) {
    x = -x;   // the sign bit flipped: the backgrounds swap with it
    p.s = p.act ? (x < 0.0f) : !ins;
  } else {
    p.s = p.act ? (x < 0.0f) : ins;
  }
  p.x = x;
  return p;
}

// The rules of include/m2s.h: OP 0 union (min), 1 intersection (max).
template <int OP>
__device__ __forceinline__ void csg_rule(const CsgPoint& a, const CsgPoint& b, float* r, bool* active, bool* s) {
  const bool b_wins = OP == 0 ? (b.x < a.x) : (b.x > a.x);
  const bool a_wins = OP == 0 ? (a.x < b.x) : (a.x > b.x);
  const bool pick_b = b_wins || (a.x == b.x && !a.act);
  *r = pick_b ? b.x : a.x;
  *active = (a.act && !b_wins) || (b.act && !a_wins);
  *s = OP == 0 ? (a.s || b.s) : (a.s && b.s);
}

// Lane l's word of a step, and what a lane needs of its operands to take part in it.
struct CsgWord {
  uint64_t mA, mB, iA, iB, woA, woB;
};
__device__ __forceinline__ CsgWord csg_load(const BandDev& A, const BandDev& B, uint64_t w, bool wanted) {
  CsgWord x{0, 0, 0, 0, 0, 0};
  if (wanted) {
    x.mA = A.mask[w];
    x.mB = B.mask[w];
    if (A.inside) x.iA = A.inside[w];
    if (B.inside) x.iB = B.inside[w];
    if (x.mA) x.woA = A.word_off[w];
    if (x.mB) x.woB = B.word_off[w];
  }
  return x;
}
__device__ __forceinline__ CsgWord csg_broadcast(const CsgWord& x, int j) {
  return CsgWord{walk_lane(x.mA, j), walk_lane(x.mB, j), walk_lane(x.iA, j), walk_lane(x.iB, j), walk_lane(x.woA, j), walk_lane(x.woB, j)};
}

template <int OP, bool NEG>
__global__ void __launch_bounds__(kWalkThreads) k_csg_mask(BandDev A, BandDev B, float a_out, float a_in_neg, float b_out, float b_in_neg, uint64_t n_words, uint64_t total, uint64_t* __restrict__ out_mask,
                                                          uint64_t* __restrict__ out_inside, uint32_t* __restrict__ unit_cnt,
                                                          uint64_t* __restrict__ group_sum) {
  WALK_UNIT_HEAD(kWalkSteps, n_words)
  uint64_t cnt = 0;
  for (int step = 0; step < kWalkSteps; ++step) {
    WALK_STEP_HEAD(n_words)
    const CsgWord x = csg_load(A, B, w, in_range);
    const uint64_t valid = walk_valid(w, in_range, total);
    const uint64_t iBs = NEG ? ~x.iB : x.iB;
    uint64_t rm = 0;
    uint64_t ri = (OP == 0 ? (x.iA | iBs) : (x.iA & iBs)) & valid;
    uint64_t todo = __ballot((x.mA | x.mB) != 0);
    while (todo) {   // wave-uniform: every lane takes every round
      const int j = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const CsgWord y = csg_broadcast(x, j);
      const CsgPoint a = csg_point<false>(A, a_out, a_in_neg, y.mA, y.iA, y.woA, lane);
      const CsgPoint b = csg_point<NEG>(B, b_out, b_in_neg, y.mB, y.iB, y.woB, lane);
      float r;
      bool active, s;
      csg_rule<OP>(a, b, &r, &active, &s);
      const uint64_t am = __ballot(active), sm = __ballot(s);
      if (lane == j) {
        rm = am & valid;
        ri = sm & valid;
      }
    }
    if (in_range) {
      out_mask[w] = rm;
      out_inside[w] = ri;
    }
    cnt += (uint64_t)__popcll(rm);
  }
  walk_publish<kCsgGroup>(cnt, lane, unit, unit_cnt, group_sum);
}

// group_base: the scanned group sums.  cap: the floats out_dist holds.
template <int OP, bool NEG>
__global__ void __launch_bounds__(kWalkThreads) k_csg_emit(BandDev A, BandDev B, float a_out, float a_in_neg, float b_out, float b_in_neg, uint64_t n_words, const uint64_t* __restrict__ out_mask,
                                                          const uint32_t* __restrict__ unit_cnt, const uint64_t* __restrict__ group_base,
                                                          uint64_t* __restrict__ out_word_off,
                                                          float* __restrict__ out_dist, uint64_t cap) {
  WALK_UNIT_HEAD(kWalkSteps, n_words)
  uint64_t base = walk_unit_base<kCsgGroup>(lane, unit, unit_cnt, group_base);
  for (int step = 0; step < kWalkSteps; ++step) {
    WALK_STEP_HEAD(n_words)
    const uint64_t rm = in_range ? out_mask[w] : 0;
    const uint64_t off = walk_word_off((uint64_t)__popcll(rm), lane, base);
    if (in_range) out_word_off[w] = off;
    const CsgWord x = csg_load(A, B, w, rm != 0);
    uint64_t todo = __ballot(rm != 0);
    while (todo) {   // wave-uniform
      const int j = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const CsgWord y = csg_broadcast(x, j);
      const uint64_t rmj = walk_lane(rm, j), offj = walk_lane(off, j);
      const CsgPoint a = csg_point<false>(A, a_out, a_in_neg, y.mA, y.iA, y.woA, lane);
      const CsgPoint b = csg_point<NEG>(B, b_out, b_in_neg, y.mB, y.iB, y.woB, lane);
      float r;
      bool active, s;
      csg_rule<OP>(a, b, &r, &active, &s);
      const uint64_t pos = offj + (uint64_t)__popcll(rmj & walk_below(lane));
      if (((rmj >> lane) & 1ull) && pos < cap) out_dist[pos] = r;
    }
  }
}

// Export: the cells of a handle from its mask, 64 words per wave and step.
__global__ void __launch_bounds__(kWalkThreads) k_csg_cells(const uint64_t* __restrict__ mask, const uint64_t* __restrict__ word_off, uint64_t n_words,
                                                           uint64_t n, uint64_t* __restrict__ cells) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint64_t wb = ((uint64_t)blockIdx.x * kWalkWaves + wave) * 64; wb < n_words; wb += (uint64_t)gridDim.x * kWalkThreads) {
    const uint64_t w = wb + lane;
    const uint64_t m = w < n_words ? mask[w] : 0;
    const uint64_t wo = m ? word_off[w] : 0;
    uint64_t todo = __ballot(m != 0);
    while (todo) {   // wave-uniform
      const int j = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const uint64_t mj = walk_lane(m, j), oj = walk_lane(wo, j);
      const uint64_t pos = oj + (uint64_t)__popcll(mj & walk_below(lane));
      if (((mj >> lane) & 1ull) && pos < n) cells[pos] = ((wb + (uint64_t)j) << 6) + (uint64_t)lane;
    }
  }
}

// Export: the sign mask from the mask's layout back to the caller's uint32[nx][ny][ceil(nz / 32)] (k_bq_sign undone).  One lane per
// output word: its up to 32 points are consecutive in L, in one mask-layout word or across two.  inside == nullptr: zeros.
__global__ void __launch_bounds__(256) k_csg_unsign(const uint64_t* __restrict__ inside, uint64_t nz, uint64_t n_out, uint64_t n_words,
                                                    uint32_t* __restrict__ bits) {
  const uint64_t nzw = (nz + 31) / 32;
  for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < n_out; idx += (uint64_t)gridDim.x * 256) {
    uint32_t out = 0;
    if (inside) {
      const uint64_t row = idx / nzw, k0 = (idx - row * nzw) * 32;
      const uint64_t nb = nz - k0 < 32 ? nz - k0 : 32;
      const uint64_t L0 = row * nz + k0;
      const uint64_t w = L0 >> 6, sh = L0 & 63;
      uint64_t v = inside[w] >> sh;
      if (sh + nb > 64 && w + 1 < n_words) v |= inside[w + 1] << (64 - sh);   // sh > 32 here
      out = (uint32_t)v & (nb == 32 ? ~0u : ((1u << nb) - 1u));
    }
    bits[idx] = out;
  }
}

template <int OP, bool NEG>
void launch_csg_as(hipStream_t st, const BandDev& A, const BandDev& B, uint64_t n_words, uint64_t total, uint64_t n_units, const BandBlock& res,
                   uint64_t cap, uint32_t* unit_cnt, uint64_t* group_sum, uint64_t* d_total) {
  const unsigned blocks = (unsigned)((n_units + kWalkWaves - 1) / kWalkWaves);
  const uint64_t n_groups = (n_units + kCsgGroup - 1) / kCsgGroup;
  hipLaunchKernelGGL((k_csg_mask<OP, NEG>), dim3(blocks), dim3(kWalkThreads), 0, st, A, B, A.bg_out, A.bg_in_neg, B.bg_out, B.bg_in_neg, n_words, total,
                     res.mask, res.inside, unit_cnt, group_sum);
  hipLaunchKernelGGL((k_scan_tiles<kScanThreads, uint64_t>), dim3(1), dim3(kScanThreads), 0, st, group_sum, n_groups, d_total);
  hipLaunchKernelGGL((k_csg_emit<OP, NEG>), dim3(blocks), dim3(kWalkThreads), 0, st, A, B, A.bg_out, A.bg_in_neg, B.bg_out, B.bg_in_neg, n_words,
                     (const uint64_t*)res.mask, (const uint32_t*)unit_cnt, (const uint64_t*)group_sum, res.word_off, res.dist, cap);
}

}  // namespace

// m2s_warmup: the first launch of a kernel of this translation unit makes the runtime load its code object (all its kernels).
__global__ void k_warm_band_csg() {}
void warm_band_csg(hipStream_t st) { hipLaunchKernelGGL(k_warm_band_csg, dim3(1), dim3(64), 0, st); }

}  // namespace m2s

using namespace m2s;

extern "C" {

int m2s_band_csg(const m2s_band* a, const m2s_band* b, int op, const m2s_band_field_opts* fopts, const m2s_opts* opts, m2s_band** out) {
  clear_error();
  if (!out) return fail(M2S_ERR_BAD_ARG, "out is NULL");
  *out = nullptr;
  if (op != M2S_CSG_UNION && op != M2S_CSG_INTERSECTION && op != M2S_CSG_DIFFERENCE) return fail(M2S_ERR_BAD_ARG, "bad m2s_csg_op %d", op);
  if (!a || !b) return fail(M2S_ERR_BAD_ARG, "band is NULL");
  if (a->device != b->device) return fail(M2S_ERR_BAD_ARG, "the bands live on devices %d and %d", a->device, b->device);
  if (!band_same_grid(a->grid, b->grid))
    return fail(M2S_ERR_BAD_ARG, "the bands' grids differ (first_cell, cell_size and cell_count must agree in every bit)");
  int rc = band_field_opts_args(fopts);
  if (rc) return rc;
  rc = band_opts_args(opts, "m2s_band_csg");
  if (rc) return rc;
  m2s_opts o;
  rc = band_call_opts(a, opts, &o);
  if (rc) return rc;
  CallCtx c;
  DeviceState* st = nullptr;
  rc = resolve_ctx(&o, &c, &st);
  if (rc) return rc;
  const bool neg = op == M2S_CSG_DIFFERENCE;
  // B* = B, or -B for the difference: its backgrounds swapped
  const float bs_out = neg ? b->bg_in : b->bg_out, bs_in = neg ? b->bg_out : b->bg_in;
  const float bg_out = fopts ? fopts->background_outside : std::min(a->bg_out, bs_out);
  const float bg_in = fopts ? fopts->background_inside : std::min(a->bg_in, bs_in);
  const uint64_t total = a->total, n_words = a->n_words;
  const uint64_t cap = std::max<uint64_t>(1, std::min(a->n + b->n, total));   // the bound of the result's cells: at least one float
  const uint64_t n_units = (n_words + kWalkUnit - 1) / kWalkUnit;               // below 2^22: a grid has fewer than 2^36 cells
  BandBlock res;
  M2S_HIP_CHECK(res.alloc(n_words, cap));
  auto drop = [&](int code) { res.free(); return code; };
  const uint64_t n_groups = (n_units + kCsgGroup - 1) / kCsgGroup;
  rc = ensure_capacity(*st, 4096 + 256 + align_up((size_t)n_units * 4) + align_up((size_t)n_groups * 8));
  if (rc) return drop(rc);
  Arena ws{st->base, st->cap, 0};
  uint64_t* d_total = ws.take<uint64_t>(4);
  uint32_t* unit_cnt = ws.take<uint32_t>(n_units);
  uint64_t* group_sum = ws.take<uint64_t>(n_groups);
  if (!d_total || !unit_cnt || !group_sum) return drop(fail(M2S_ERR_HIP, "internal: workspace"));
  const BandDev A = dev_of(a), B = dev_of(b);
  hipError_t e = hipSuccess;
  if (c.timings) e = hipEventRecord(st->ev[0], c.stream);
  if (e == hipSuccess) e = hipMemsetAsync(res.dist, 0, 4, c.stream);   // an empty result still has one defined float
  if (e == hipSuccess) e = hipMemsetAsync(group_sum, 0, n_groups * 8, c.stream);
  if (e != hipSuccess) return drop(fail(M2S_ERR_HIP, "HIP error: %s", hipGetErrorString(e)));
  if (op == M2S_CSG_UNION) launch_csg_as<0, false>(c.stream, A, B, n_words, total, n_units, res, cap, unit_cnt, group_sum, d_total);
  else if (op == M2S_CSG_INTERSECTION) launch_csg_as<1, false>(c.stream, A, B, n_words, total, n_units, res, cap, unit_cnt, group_sum, d_total);
  else launch_csg_as<1, true>(c.stream, A, B, n_words, total, n_units, res, cap, unit_cnt, group_sum, d_total);
  e = hipGetLastError();
  if (e == hipSuccess && c.timings) e = hipEventRecord(st->ev[1], c.stream);
  uint64_t n = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&n, d_total, 8, hipMemcpyDeviceToHost, c.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
  if (e != hipSuccess) return drop(fail(M2S_ERR_HIP, "HIP error: %s", hipGetErrorString(e)));
  if (n > cap) return drop(fail(M2S_ERR_HIP, "internal: the result has %llu cells, above the bound %llu", (unsigned long long)n, (unsigned long long)cap));
  if (c.timings) {
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, st->ev[0], st->ev[1]);
    memset(c.timings, 0, sizeof(*c.timings));
    c.timings->seed_ms = ms;
    c.timings->total_ms = ms;
    c.timings->n_units = n;
  }
  *out = band_adopt(res, a->device, a->grid, n, total, n_words, bg_out, bg_in);
  return M2S_OK;
}

int m2s_band_export(const m2s_band* band, uint64_t* cells_out, float* distances_out, uint64_t capacity, uint32_t* inside_bits_out,
                    const m2s_opts* opts) {
  clear_error();
  if (!cells_out && !distances_out && !inside_bits_out) return fail(M2S_ERR_BAD_ARG, "no output requested");
  if (!band) return fail(M2S_ERR_BAD_ARG, "band is NULL");
  if (capacity < band->n)
    return fail(M2S_ERR_BAD_ARG, "capacity = %llu below the band's %llu cells", (unsigned long long)capacity, (unsigned long long)band->n);
  int rc = band_opts_args(opts, "m2s_band_export");
  if (rc) return rc;
  m2s_opts o;
  rc = band_call_opts(band, opts, &o);
  if (rc) return rc;
  o.synchronous = 1;
  const uint64_t n = band->n, n_words = band->n_words, nz = band->grid.cell_count[2];
  const uint64_t sign_words = (nz + 31) / 32 * band->grid.cell_count[0] * band->grid.cell_count[1];
  QueryIo io[3] = {{cells_out, cells_out ? n * 8 : 0, true}, {distances_out, distances_out ? n * 4 : 0, true},
                   {inside_bits_out, inside_bits_out ? sign_words * 4 : 0, true}};
  return run_query(&o, io, 3, n, [&](hipStream_t s) {
    if (cells_out && n)
      hipLaunchKernelGGL(k_csg_cells, dim3(blocks_for(n_words)), dim3(kWalkThreads), 0, s, band->mask, band->word_off, n_words, n,
                         reinterpret_cast<uint64_t*>(io[0].dev));
    if (distances_out && n) M2S_HIP_CHECK(hipMemcpyAsync(io[1].dev, band->dist, n * 4, hipMemcpyDeviceToDevice, s));
    if (inside_bits_out)
      hipLaunchKernelGGL(k_csg_unsign, dim3(blocks_for(sign_words)), dim3(256), 0, s, band->inside, nz, sign_words, n_words,
                         reinterpret_cast<uint32_t*>(io[2].dev));
    M2S_HIP_CHECK(hipGetLastError());
    return 0;
  });
}

int m2s_band_field_info(const m2s_band* band, m2s_band_field_opts* fopts_out, int* has_inside) {
  clear_error();
  if (!band) return fail(M2S_ERR_BAD_ARG, "band is NULL");
  if (fopts_out) {
    fopts_out->struct_size = sizeof(m2s_band_field_opts);
    fopts_out->background_outside = band->bg_out;
    fopts_out->background_inside = band->bg_in;
  }
  if (has_inside) *has_inside = band->inside != nullptr;
  return M2S_OK;
}

}  // extern "C"
