// band_resample.hip — m2s_band_resample: a resident band evaluated at the cell centres of another grid under a 3 x 4 map from target space
// to source space, as a new resident band on that grid, gfx950.  The contract is include/m2s.h's (per target grid point, to the bit);
// tests/band_resample_model.py restates it in numpy.  Nothing sized 4 bytes per point of either grid exists: per 64 target points the
// result's three index words and the unit counts, per result cell its value.
//
// The two passes are band_csg.hip's on band_walk.hip.h's walk and offsets with one difference: here EVERY target
// word has work, not one in a few hundred, so a word is not "settled by its own lane" but taken by the whole wave, one after the other.
//   k_rs_mask    per point: the centre p, the source point q, and whether q is on the source box.  A word whose 64 points are all off the
//                box (one ballot) is settled as 0 / 0 with no memory read.  Otherwise prepare<MODE> and the K source mask bits; only a
//                lane with full support fetches its values (band_fetch.hip.h) for the isfinite rule; an inactive lane on the box reads
//                sX at its SNAP cell.  Two ballots are the result's mask word and sign word.  The unit's popcount is published;
//                n_partial and n_nonfinite go by one atomic add per wave.
//   k_scan_tiles the group sums; the total is the result's cell count, read by the host with the call's one synchronisation inside it;
//                the values are then allocated at their true size.
//   k_rs_emit    the same units: the result's word_off, and lane t of a word with active points computes r again and stores it at
//                word_off + rank.  r is computed twice rather than kept: where it goes is known only after the scan.
//   k_rs_open    n_open: band_redistance.hip's neighbour look-ups on the result's mask and sign words, units of 256 words (most are empty).
// A unit is kRsSteps * 64 words.  With every word at work a wave's unit is a chain of that many rounds of dependent loads, so it is one
// step: at 256^3 (262 144 words) units of 256 words are one wave per SIMD of the chip.  The groups hold 64 units, so that k_scan_tiles
// sees as many sums as in a CSG call.  The unit and step heads are band_walk.hip.h's; its three offsets helpers (walk_publish,
// walk_unit_base, walk_word_off) are written out in k_rs_mask and k_rs_emit: hipcc orders the inlined helpers' instructions otherwise,
// k_rs_mask came out 6 - 7 instructions longer and the TRILINEAR k_rs_emit measured 0.5 - 2 % slower (profiles/band_walk_isa_check.txt).
// A change to a helper is made here too.  All stores are plain vector stores; the ballot loops are wave-uniform; no LDS but the scan's.
#include "../../include/m2s.h"
#include "band_fetch.hip.h"
#include "band_handle.h"
#include "band_walk.hip.h"
#include "capi_internal.h"
#include "common.h"
#include "grid_query.hip.h"
#include "isosurface.hip.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace m2s {
namespace {

#ifndef M2S_RS_STEPS   // tools/exp_band_resample.py measures a build with -DM2S_RS_STEPS=4 -DM2S_RS_GROUP=16 (band_csg.hip's units) beside this one
#define M2S_RS_STEPS 1
#define M2S_RS_GROUP 64
#endif
constexpr int kRsSteps = M2S_RS_STEPS;                      // steps of 64 words per wave
constexpr uint64_t kRsUnit = 64 * kRsSteps;                 // words per wave
constexpr int kRsGroup = M2S_RS_GROUP;                      // units per scanned sum (at most 64: one lane each in k_rs_emit)
static_assert(kRsSteps >= 1 && kRsGroup >= 1 && kRsGroup <= 64, "a group's units are summed by one lane each");

// The target grid's scalars and the map: p = first + (float)idx * cs, q_a = ((m[4a] p.x + m[4a+1] p.y) + m[4a+2] p.z) + m[4a+3].
struct RsTarget {
  float first[3], cs[3];
  float m[12];
  float scale;
};

__device__ __forceinline__ void rs_source(const RsTarget& t, const WalkIjk& p, float* q) {
  const float px = t.first[0] + (float)p.i * t.cs[0];
  const float py = t.first[1] + (float)p.j * t.cs[1];
  const float pz = t.first[2] + (float)p.k * t.cs[2];
#pragma unroll
  for (int a = 0; a < 3; ++a) q[a] = ((t.m[4 * a] * px + t.m[4 * a + 1] * py) + t.m[4 * a + 2] * pz) + t.m[4 * a + 3];
}

// prepare()'s state == 0: no NaN coordinate and on the closed box.
__device__ __forceinline__ bool rs_on_box(const GridQuery& q, const float* p) {
  const bool nan = p[0] != p[0] || p[1] != p[1] || p[2] != p[2];
  const bool out = p[0] < q.start[0] || p[1] < q.start[1] || p[2] < q.start[2] || p[0] > q.end[0] || p[1] > q.end[1] || p[2] > q.end[2];
  return !nan && !out;
}

__device__ __forceinline__ bool rs_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// The support of a prepared sample from the mask words alone: fetch_rounds' round 1 (a corner shares the word of its lower neighbour).
template <int MODE>
__device__ __forceinline__ uint32_t rs_support(const BandDev& X, const Prep<MODE>& p) {
  constexpr int K = Corners<MODE>::K;
  constexpr int S = MODE == M2S_SAMPLE_TRILINEAR ? 4 : 1;
  uint64_t mw[K];
  uint32_t hits = 0;
#pragma unroll
  for (int c = 0; c < K; ++c) {
    const uint64_t w = p.off[c] >> 6;
    const bool same = c >= S && (p.off[c >= S ? c - S : 0] >> 6) == w;
    mw[c] = same ? mw[c >= S ? c - S : 0] : X.mask[w];
    hits += (uint32_t)((mw[c] >> (p.off[c] & 63)) & 1ull);
  }
  return hits;
}

// sX at the source cell c (inside the grid): act ? (x < 0) : inside bit.
template <bool SIGN>
__device__ __forceinline__ bool rs_sign(const BandDev& X, uint64_t c) {
  const uint64_t w = c >> 6;
  const int b = (int)(c & 63);
  const uint64_t m = X.mask[w];
  if ((m >> b) & 1ull) {
    uint64_t at = X.word_off[w] + (uint64_t)__popcll(m & walk_below(b));
    at = at < X.n ? at : 0;   // at < n whenever the index is sound; the guard keeps a broken invariant in bounds
    return X.dist[at] < 0.0f;
  }
  return SIGN ? (bool)((X.inside[w] >> b) & 1ull) : false;
}

// r of a point whose K reads are all active: the band's sample (no background enters it) times value_scale.
template <int MODE>
__device__ __forceinline__ float rs_value(const GridQuery& q, const BandDev& X, const Prep<MODE>& p, float scale) {
  float v[1][Corners<MODE>::K];
  uint32_t sup;
  fetch<MODE, 1, false, 0>(X, &p, v, &sup);
  return combine<MODE>(q, p, v[0]) * scale;
}

// q, X: the source grid (iso 0) and handle; t, g: the target.  counters[1] += n_partial, counters[2] += n_nonfinite.
template <int MODE, bool SIGN>
__global__ void __launch_bounds__(kWalkThreads) k_rs_mask(GridQuery q, BandDev X, RsTarget t, WalkGrid g, uint64_t* __restrict__ out_mask,
                                                        uint64_t* __restrict__ out_inside, uint32_t* __restrict__ unit_cnt,
                                                        uint64_t* __restrict__ group_sum, uint64_t* __restrict__ counters) {
  constexpr int K = Corners<MODE>::K;
  WALK_UNIT_HEAD(kRsSteps, g.n_words)
  uint64_t cnt = 0;
  uint32_t n_partial = 0, n_nonfinite = 0;
  for (int step = 0; step < kRsSteps; ++step) {
    WALK_STEP_HEAD(g.n_words)
    WalkIjk base{0, 0, 0};
    if (in_range) base = walk_base(w << 6, g);
    uint64_t rm = 0, ri = 0;
    const int rounds = (int)(g.n_words - wb < 64 ? g.n_words - wb : 64);   // wave-uniform
    for (int j = 0; j < rounds; ++j) {
      const WalkIjk p = walk_step(walk_bcast(base, j), (uint32_t)lane, g);
      const uint64_t L = ((wb + (uint64_t)j) << 6) + (uint64_t)lane;
      float sp[3];
      rs_source(t, p, sp);
      const bool on = L < g.total && rs_on_box(q, sp);
      if (__ballot(on) == 0) continue;   // the whole word is off the source box: 0 / 0, nothing read
      bool active = false, s = false;
      if (on) {
        const Prep<MODE> pr = prepare<MODE>(q, sp[0], sp[1], sp[2]);
        const uint32_t sup = rs_support<MODE>(X, pr);
        if (sup == (uint32_t)K) {
          const float r = rs_value<MODE>(q, X, pr, t.scale);
          active = rs_finite(r);
          s = r < 0.0f;
          n_nonfinite += active ? 0u : 1u;
        } else if (sup) {
          ++n_partial;
        }
        if (!active) s = rs_sign<SIGN>(X, prepare<M2S_SAMPLE_SNAP>(q, sp[0], sp[1], sp[2]).off[0]);
      }
      const uint64_t am = __ballot(active), sm = __ballot(s);
      if (lane == j) {
        rm = am;
        ri = sm;
      }
    }
    if (in_range) {
      out_mask[w] = rm;
      out_inside[w] = ri;
    }
    cnt += (uint64_t)__popcll(rm);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {   // walk_publish written out: one reduction and one lane-0 block with the two counters
    cnt += __shfl_xor(cnt, o, 64);
    n_partial += __shfl_xor(n_partial, o, 64);
    n_nonfinite += __shfl_xor(n_nonfinite, o, 64);
  }
  if (lane == 0) {
    unit_cnt[unit] = (uint32_t)cnt;   // at most 64 * kRsUnit
    if (cnt) atomicAdd((unsigned long long*)(group_sum + unit / kRsGroup), (unsigned long long)cnt);   // zeroed by the launcher
    if (n_partial) atomicAdd((unsigned long long*)(counters + 1), (unsigned long long)n_partial);
    if (n_nonfinite) atomicAdd((unsigned long long*)(counters + 2), (unsigned long long)n_nonfinite);
  }
}

// group_base: the scanned group sums.  cap: the floats out_dist holds.
template <int MODE>
__global__ void __launch_bounds__(kWalkThreads) k_rs_emit(GridQuery q, BandDev X, RsTarget t, WalkGrid g, const uint64_t* __restrict__ out_mask,
                                                        const uint32_t* __restrict__ unit_cnt, const uint64_t* __restrict__ group_base,
                                                        uint64_t* __restrict__ out_word_off, float* __restrict__ out_dist, uint64_t cap) {
  WALK_UNIT_HEAD(kRsSteps, g.n_words)
  // walk_unit_base and walk_word_off written out (see the head of the file)
  const uint64_t first = unit - unit % kRsGroup;   // the group's first unit: every unit from there to this one exists
  uint64_t before = first + lane < unit ? unit_cnt[first + lane] : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
  uint64_t run = group_base[unit / kRsGroup] + before;
  for (int step = 0; step < kRsSteps; ++step) {
    WALK_STEP_HEAD(g.n_words)
    const uint64_t rm = in_range ? out_mask[w] : 0;
    const uint64_t c = (uint64_t)__popcll(rm);
    uint64_t incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t y = __shfl_up(incl, o, 64);
      if (lane >= o) incl += y;
    }
    const uint64_t off = run + incl - c;
    run += walk_lane(incl, 63);
    if (in_range) out_word_off[w] = off;
    WalkIjk base{0, 0, 0};
    if (rm) base = walk_base(w << 6, g);
    uint64_t todo = __ballot(rm != 0);
    while (todo) {   // wave-uniform
      const int j = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const uint64_t rmj = walk_lane(rm, j), offj = walk_lane(off, j);
      const WalkIjk p = walk_step(walk_bcast(base, j), (uint32_t)lane, g);
      const uint64_t pos = offj + (uint64_t)__popcll(rmj & walk_below(lane));
      if (((rmj >> lane) & 1ull) && pos < cap) {   // an active point is inside the target grid and on the source box
        float sp[3];
        rs_source(t, p, sp);
        const Prep<MODE> pr = prepare<MODE>(q, sp[0], sp[1], sp[2]);
        out_dist[pos] = rs_value<MODE>(q, X, pr, t.scale);
      }
    }
  }
}

__device__ __forceinline__ bool rs_bit(const uint64_t* __restrict__ a, uint64_t L) { return (a[L >> 6] >> (L & 63)) & 1ull; }

// counters[3] += the ordered pairs (L active, M an inactive axis neighbour inside the grid, s[M] != s[L]): k_rd_frozen's look-ups.
__global__ void __launch_bounds__(kWalkThreads) k_rs_open(const uint64_t* __restrict__ mask, const uint64_t* __restrict__ S, WalkGrid g,
                                                        uint64_t* __restrict__ counters) {
  WALK_UNIT_HEAD(kWalkSteps, g.n_words)
  uint64_t n_open = 0;
  for (int step = 0; step < kWalkSteps; ++step) {
    WALK_STEP_HEAD(g.n_words)
    const uint64_t m = in_range ? mask[w] : 0;
    const uint64_t sw = m ? S[w] : 0;
    WalkIjk base{0, 0, 0};
    if (m) base = walk_base(w << 6, g);
    uint64_t todo = __ballot(m != 0);
    while (todo) {   // wave-uniform
      const int j = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const uint64_t mj = walk_lane(m, j), sj = walk_lane(sw, j);
      const WalkIjk p = walk_step(walk_bcast(base, j), (uint32_t)lane, g);
      const uint64_t L = ((wb + (uint64_t)j) << 6) + (uint64_t)lane;
      const bool sL = (sj >> lane) & 1ull;
      if ((mj >> lane) & 1ull) {   // an active point is inside the grid
#define RS_NB(cond, M)                                               \
  if (cond) {                                                        \
    const uint64_t Mv = (M);                                         \
    if (rs_bit(S, Mv) != sL && !rs_bit(mask, Mv)) ++n_open;          \
  }
        RS_NB(p.i + 1 < g.nx, L + g.si)
        RS_NB(p.i > 0, L - g.si)
        RS_NB(p.j + 1 < g.ny, L + g.sj)
        RS_NB(p.j > 0, L - g.sj)
        RS_NB(p.k + 1 < g.nz, L + 1)
        RS_NB(p.k > 0, L - 1)
#undef RS_NB
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_open += __shfl_xor(n_open, o, 64);
  if (lane == 0 && n_open) atomicAdd((unsigned long long*)(counters + 3), (unsigned long long)n_open);
}

template <int MODE>
void launch_mask_as(hipStream_t st, unsigned blocks, bool sign, const GridQuery& q, const BandDev& X, const RsTarget& t, const WalkGrid& g,
                    uint64_t* mask, uint64_t* inside, uint32_t* unit_cnt, uint64_t* group_sum, uint64_t* counters) {
  if (sign) hipLaunchKernelGGL((k_rs_mask<MODE, true>), dim3(blocks), dim3(kWalkThreads), 0, st, q, X, t, g, mask, inside, unit_cnt, group_sum, counters);
  else hipLaunchKernelGGL((k_rs_mask<MODE, false>), dim3(blocks), dim3(kWalkThreads), 0, st, q, X, t, g, mask, inside, unit_cnt, group_sum, counters);
}

template <int MODE>
void launch_emit_as(hipStream_t st, unsigned blocks, const GridQuery& q, const BandDev& X, const RsTarget& t, const WalkGrid& g, const uint64_t* mask,
                    const uint32_t* unit_cnt, const uint64_t* group_base, uint64_t* word_off, float* dist, uint64_t cap) {
  hipLaunchKernelGGL((k_rs_emit<MODE>), dim3(blocks), dim3(kWalkThreads), 0, st, q, X, t, g, mask, unit_cnt, group_base, word_off, dist, cap);
}

}  // namespace

// m2s_warmup: the first launch of a kernel of this translation unit makes the runtime load its code object (all its kernels).
__global__ void k_warm_band_resample() {}
void warm_band_resample(hipStream_t st) { hipLaunchKernelGGL(k_warm_band_resample, dim3(1), dim3(64), 0, st); }

}  // namespace m2s

using namespace m2s;

extern "C" {

int m2s_band_resample(const m2s_band* band, const m2s_grid* target, const m2s_band_resample_opts* ropts, const m2s_band_field_opts* fopts,
                      const m2s_opts* opts, m2s_band** out, m2s_band_resample_info* info_out) {
  clear_error();
  if (!out) return fail(M2S_ERR_BAD_ARG, "out is NULL");
  *out = nullptr;
  if (!band) return fail(M2S_ERR_BAD_ARG, "band is NULL");
  if (!target) return fail(M2S_ERR_BAD_ARG, "target is NULL");
  RsTarget t{};
  int mode = M2S_SAMPLE_TRILINEAR;
  t.m[0] = t.m[5] = t.m[10] = 1.0f;
  t.scale = 1.0f;
  if (ropts) {
    if (ropts->struct_size != sizeof(m2s_band_resample_opts))
      return fail(M2S_ERR_BAD_ARG, "m2s_band_resample_opts.struct_size is not sizeof(m2s_band_resample_opts)");
    mode = ropts->mode;
    if (mode != M2S_SAMPLE_SNAP && mode != M2S_SAMPLE_TRILINEAR && mode != M2S_SAMPLE_TETRAHEDRAL) return fail(M2S_ERR_BAD_ARG, "bad sample mode %d", mode);
    for (int a = 0; a < 12; ++a) {
      if (!std::isfinite(ropts->to_source[a])) return fail(M2S_ERR_BAD_ARG, "to_source[%d] = %g is not finite", a, (double)ropts->to_source[a]);
      t.m[a] = ropts->to_source[a];
    }
    if (!(ropts->value_scale > 0.0f) || !std::isfinite(ropts->value_scale))
      return fail(M2S_ERR_BAD_ARG, "value_scale = %g must be > 0 and finite", (double)ropts->value_scale);
    t.scale = ropts->value_scale;
  }
  int rc = band_field_opts_args(fopts);
  if (rc) return rc;
  if (info_out && info_out->struct_size != sizeof(m2s_band_resample_info))
    return fail(M2S_ERR_BAD_ARG, "m2s_band_resample_info.struct_size is not sizeof(m2s_band_resample_info)");
  rc = band_opts_args(opts, "m2s_band_resample");
  if (rc) return rc;
  GridQuery qt;
  int ignored = 0;
  rc = grid_query_args(target, nullptr, false, nullptr, &qt, &ignored);   // what m2s_band_create rejects of a grid
  if (rc) return rc;
  uint64_t total = 0, n_words = 0;
  rc = band_grid_cells(target, "target grid", &total, &n_words);
  if (rc) return rc;
  const WalkGrid g = walk_grid_of(target->cell_count, total, n_words);
  for (int a = 0; a < 3; ++a) {
    t.first[a] = target->first_cell[a];
    t.cs[a] = target->cell_size[a];
  }
  // ---- from here on the handle is read ----
  m2s_opts o;
  rc = band_call_opts(band, opts, &o);
  if (rc) return rc;
  const float bg_out = fopts ? fopts->background_outside : band->bg_out * t.scale;
  const float bg_in = fopts ? fopts->background_inside : band->bg_in * t.scale;
  if (!good_background(bg_out) || !good_background(bg_in))
    return fail(M2S_ERR_BAD_ARG, "the input's backgrounds times value_scale (%g outside, %g inside) are not finite: give m2s_band_field_opts", (double)bg_out,
                (double)bg_in);
  GridQuery q;
  rc = grid_query_args(&band->grid, nullptr, false, nullptr, &q, &ignored);
  if (rc) return rc;
  q.iso = 0.0f;
  q.outside = band->bg_out;
  CallCtx c;
  DeviceState* st = nullptr;
  rc = resolve_ctx(&o, &c, &st);
  if (rc) return rc;

  const uint64_t n_units = (n_words + kRsUnit - 1) / kRsUnit;          // below 2^24: a grid has fewer than 2^36 cells
  const uint64_t n_groups = (n_units + kRsGroup - 1) / kRsGroup;
  const unsigned blocks = (unsigned)((n_units + kWalkWaves - 1) / kWalkWaves);
  const uint64_t open_units = (n_words + kWalkUnit - 1) / kWalkUnit;
  const unsigned open_blocks = (unsigned)((open_units + kWalkWaves - 1) / kWalkWaves);
  BandBlock res;   // the result: its three index arrays now, its values once the count is known
  auto drop = [&](int code) {
    res.free();
    return code;
  };
  auto hip_fail = [&](hipError_t e) { return drop(fail(M2S_ERR_HIP, "HIP error: %s", hipGetErrorString(e))); };
  rc = ensure_capacity(*st, 4096 + 256 + align_up((size_t)n_units * 4) + align_up((size_t)n_groups * 8));
  if (rc) return rc;
  Arena ws{st->base, st->cap, 0};
  uint64_t* d_hdr = ws.take<uint64_t>(4);   // [0] the cell count (the scan's total), [1] n_partial, [2] n_nonfinite, [3] n_open
  uint32_t* unit_cnt = ws.take<uint32_t>(n_units);
  uint64_t* group_sum = ws.take<uint64_t>(n_groups);
  if (!d_hdr || !unit_cnt || !group_sum) return fail(M2S_ERR_HIP, "internal: workspace");
  hipError_t e = res.alloc_index(n_words);
  if (e != hipSuccess) return hip_fail(e);
  const BandDev X = dev_of(band);
  hipStream_t s = c.stream;

  // ---- the mask pass and the scan ----
  if (c.timings) e = hipEventRecord(st->ev[0], s);
  if (e == hipSuccess) e = hipMemsetAsync(d_hdr, 0, 32, s);
  if (e == hipSuccess) e = hipMemsetAsync(group_sum, 0, n_groups * 8, s);
  if (e != hipSuccess) return hip_fail(e);
  const bool sign = X.inside != nullptr;
  if (mode == M2S_SAMPLE_SNAP) launch_mask_as<M2S_SAMPLE_SNAP>(s, blocks, sign, q, X, t, g, res.mask, res.inside, unit_cnt, group_sum, d_hdr);
  else if (mode == M2S_SAMPLE_TRILINEAR) launch_mask_as<M2S_SAMPLE_TRILINEAR>(s, blocks, sign, q, X, t, g, res.mask, res.inside, unit_cnt, group_sum, d_hdr);
  else launch_mask_as<M2S_SAMPLE_TETRAHEDRAL>(s, blocks, sign, q, X, t, g, res.mask, res.inside, unit_cnt, group_sum, d_hdr);
  hipLaunchKernelGGL((k_scan_tiles<kScanThreads, uint64_t>), dim3(1), dim3(kScanThreads), 0, s, group_sum, n_groups, d_hdr);
  e = hipGetLastError();
  if (e == hipSuccess && c.timings) e = hipEventRecord(st->ev[1], s);
  uint64_t hdr[4] = {0, 0, 0, 0};
  if (e == hipSuccess) e = hipMemcpyAsync(hdr, d_hdr, 24, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);   // the call's one synchronisation before its end: the count sizes the values
  if (e != hipSuccess) return hip_fail(e);
  const uint64_t n = hdr[0];
  if (n > g.total) return drop(fail(M2S_ERR_HIP, "internal: the result has %llu cells, the grid %llu", (unsigned long long)n, (unsigned long long)g.total));
  const uint64_t cap = std::max<uint64_t>(n, 1);   // at least one float: a lane's guarded read needs an address
  e = res.alloc_values(cap);
  if (e != hipSuccess) return hip_fail(e);

  // ---- the value pass, then n_open ----
  if (c.timings) e = hipEventRecord(st->ev[2], s);
  if (e == hipSuccess) e = hipMemsetAsync(res.dist, 0, 4, s);   // an empty result still has one defined float
  if (e != hipSuccess) return hip_fail(e);
  if (mode == M2S_SAMPLE_SNAP) launch_emit_as<M2S_SAMPLE_SNAP>(s, blocks, q, X, t, g, res.mask, unit_cnt, group_sum, res.word_off, res.dist, cap);
  else if (mode == M2S_SAMPLE_TRILINEAR) launch_emit_as<M2S_SAMPLE_TRILINEAR>(s, blocks, q, X, t, g, res.mask, unit_cnt, group_sum, res.word_off, res.dist, cap);
  else launch_emit_as<M2S_SAMPLE_TETRAHEDRAL>(s, blocks, q, X, t, g, res.mask, unit_cnt, group_sum, res.word_off, res.dist, cap);
  e = hipGetLastError();
  if (e == hipSuccess && c.timings) e = hipEventRecord(st->ev[3], s);
  if (e != hipSuccess) return hip_fail(e);
  hipLaunchKernelGGL(k_rs_open, dim3(open_blocks), dim3(kWalkThreads), 0, s, (const uint64_t*)res.mask, (const uint64_t*)res.inside, g, d_hdr);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(&hdr[3], d_hdr + 3, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && c.timings) e = hipEventRecord(st->ev[4], s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);   // the end of the call: the result is complete when it returns
  if (e != hipSuccess) return hip_fail(e);
  if (c.timings) {
    float mask_ms = 0.0f, value_ms = 0.0f, total = 0.0f;
    (void)hipEventElapsedTime(&mask_ms, st->ev[0], st->ev[1]);
    (void)hipEventElapsedTime(&value_ms, st->ev[2], st->ev[3]);
    (void)hipEventElapsedTime(&total, st->ev[0], st->ev[4]);
    memset(c.timings, 0, sizeof(*c.timings));
    c.timings->seed_ms = mask_ms;
    c.timings->distance_ms = value_ms;
    c.timings->total_ms = total;
    c.timings->n_units = n;
  }
  if (info_out) {
    info_out->reserved = 0;
    info_out->n_cells = n;
    info_out->n_partial = hdr[1];
    info_out->n_nonfinite = hdr[2];
    info_out->n_open = hdr[3];
  }
  *out = band_adopt(res, band->device, *target, n, g.total, n_words, bg_out, bg_in);
  return M2S_OK;
}

}  // extern "C"
