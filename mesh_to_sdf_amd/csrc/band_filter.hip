// band_filter.hip — m2s_band_filter: the values of a resident band smoothed by a mean, a Laplacian or a mean-curvature flow, on the whole
// band or inside a region, gfx950.  The contract is include/m2s.h's (per grid point, to the bit); tests/band_filter_model.py restates it in
// numpy.  Nothing sized 4 bytes per grid point exists: the arrays are per mask word (the result's sign word) or per active cell.
//
// The two kernels that walk the mask words are band_walk.hip.h's walk, units of 256 words; they live in
// band_stencil.hip.h, which band_advect.hip shares.
//   k_bf_table   per active cell, once: the list places of its 6 or 18 clamped neighbours as 32-bit slots (a rank look-up each: mask word,
//                word_off, popcount below); an inactive neighbour becomes one of the two places n and n + 1 behind the values, which hold
//                +background_outside and -background_inside; the cell's `where` bit; its value into the first value buffer.
//   k_bf_pass    one Jacobi pass, one lane per active cell: the slots, their values from the pass's input buffer, the arithmetic of the
//                header, a store to the OTHER buffer; non-finite candidates counted by one atomic add per wave.  It reads no index word,
//                takes no branch per neighbour and divides nothing but what the definition divides.
//   k_bf_final   the result's sign words (a ballot per mask word), its values, n_changed, n_sign_flips and max_change.
// All stores are plain vector stores; the ballot loops are wave-uniform; no LDS is used.
#include "../../include/m2s.h"
#include "band_handle.h"
#include "band_walk.hip.h"
#include "capi_internal.h"
#include "common.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

#include "band_stencil.hip.h"

namespace m2s {
namespace {

// The host constants of the definition, computed in binary32 on the host.
struct BfConst {
  float w[3];     // w_a = r_a * r_a
  float gs[3];    // 0.5f * r_a
  float xs[3];    // 0.25f * (r_a * r_b) for ab = ij, ik, jk
  float dt;       // 1 / (2 * ((w_i + w_j) + w_k))
};

// t_a = ((N(+a) - c) + (N(-a) - c)) * w_a
__device__ __forceinline__ float bf_second(float np, float nm, float c, float w) { return ((np - c) + (nm - c)) * w; }

// One Jacobi pass, one lane per active cell: v_out[r] = in the region and finite ? cand : c, from v_in only (v_out is the other buffer).
// KIND: m2s_filter_kind; AXIS: the axis of a M2S_FILTER_MEAN pass.  counters[0] += the candidates that were not finite.
template <int KIND, int AXIS>
__global__ void __launch_bounds__(256) k_bf_pass(const uint32_t* __restrict__ slots, const uint8_t* __restrict__ in_region, const float* __restrict__ v_in,
                                                 float* __restrict__ v_out, uint64_t n, BfConst k, uint64_t* __restrict__ counters) {
  uint32_t bad = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (uint64_t)gridDim.x * 256) {
    const float c = v_in[r];
    float next = c;
    if (in_region[r]) {
      float cand;
      if (KIND == M2S_FILTER_MEAN) {
        const float np = v_in[slots[(uint64_t)(2 * AXIS) * n + r]], nm = v_in[slots[(uint64_t)(2 * AXIS + 1) * n + r]];
        cand = ((nm + c) + np) / 3.0f;
      } else {
        float N[kBfAllSlots];
#pragma unroll
        for (int s = 0; s < (KIND == M2S_FILTER_LAPLACIAN ? kBfAxisSlots : kBfAllSlots); ++s) N[s] = v_in[slots[(uint64_t)s * n + r]];
        const float ti = bf_second(N[0], N[1], c, k.w[0]), tj = bf_second(N[2], N[3], c, k.w[1]), tk = bf_second(N[4], N[5], c, k.w[2]);
        if (KIND == M2S_FILTER_LAPLACIAN) {
          cand = c + k.dt * ((ti + tj) + tk);
        } else {
          const float gi = (N[0] - N[1]) * k.gs[0], gj = (N[2] - N[3]) * k.gs[1], gk = (N[4] - N[5]) * k.gs[2];
          const float xij = ((N[6] - N[7]) - (N[8] - N[9])) * k.xs[0];
          const float xik = ((N[10] - N[11]) - (N[12] - N[13])) * k.xs[1];
          const float xjk = ((N[14] - N[15]) - (N[16] - N[17])) * k.xs[2];
          const float qi = gi * gi, qj = gj * gj, qk = gk * gk;
          const float num = ((ti * (qj + qk) + tj * (qi + qk)) + tk * (qi + qj)) - 2.0f * (((gi * gj) * xij + (gi * gk) * xik) + (gj * gk) * xjk);
          const float g2 = (qi + qj) + qk;
          cand = g2 > 0.0f ? c + k.dt * (num / g2) : c;
        }
      }
      if (bf_finite(cand)) next = cand;
      else ++bad;
    }
    v_out[r] = next;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd((unsigned long long*)counters, (unsigned long long)bad);
}


template <int KIND, int AXIS>
void launch_pass(hipStream_t st, unsigned blocks, const uint32_t* slots, const uint8_t* in_region, const float* v_in, float* v_out, uint64_t n,
                 const BfConst& k, uint64_t* counters) {
  hipLaunchKernelGGL((k_bf_pass<KIND, AXIS>), dim3(blocks), dim3(256), 0, st, slots, in_region, v_in, v_out, n, k, counters);
}

}  // namespace

// m2s_warmup: the first launch of a kernel of this translation unit makes the runtime load its code object (all its kernels).
__global__ void k_warm_band_filter() {}
void warm_band_filter(hipStream_t st) { hipLaunchKernelGGL(k_warm_band_filter, dim3(1), dim3(64), 0, st); }

}  // namespace m2s

using namespace m2s;

extern "C" {

int m2s_band_filter(const m2s_band* band, const m2s_band* where, const m2s_band_filter_opts* fl, const m2s_band_field_opts* fopts,
                    const m2s_opts* opts, m2s_band** out, m2s_band_filter_info* info_out) {
  clear_error();
  if (!out) return fail(M2S_ERR_BAD_ARG, "out is NULL");
  *out = nullptr;
  if (!band) return fail(M2S_ERR_BAD_ARG, "band is NULL");
  if (!fl) return fail(M2S_ERR_BAD_ARG, "m2s_band_filter_opts is NULL");
  if (fl->struct_size != sizeof(m2s_band_filter_opts))
    return fail(M2S_ERR_BAD_ARG, "m2s_band_filter_opts.struct_size is not sizeof(m2s_band_filter_opts)");
  if (fl->kind != M2S_FILTER_MEAN && fl->kind != M2S_FILTER_LAPLACIAN && fl->kind != M2S_FILTER_MEAN_CURVATURE)
    return fail(M2S_ERR_BAD_ARG, "bad m2s_filter_kind %d", fl->kind);
  if (fl->iterations == 0 || fl->iterations > 65536) return fail(M2S_ERR_BAD_ARG, "iterations = %u: must be 1 .. 65536", fl->iterations);
  if (fl->width != 1) return fail(M2S_ERR_BAD_ARG, "width = %u: must be 1", fl->width);
  int rc = band_field_opts_args(fopts);
  if (rc) return rc;
  if (info_out && info_out->struct_size != sizeof(m2s_band_filter_info))
    return fail(M2S_ERR_BAD_ARG, "m2s_band_filter_info.struct_size is not sizeof(m2s_band_filter_info)");
  rc = band_opts_args(opts, "m2s_band_filter");
  if (rc) return rc;
  if (where) {
    if (where->device != band->device) return fail(M2S_ERR_BAD_ARG, "the band and the region live on devices %d and %d", band->device, where->device);
    if (!band_same_grid(band->grid, where->grid))
      return fail(M2S_ERR_BAD_ARG, "the band's and the region's grids differ (first_cell, cell_size and cell_count must agree in every bit)");
  }
  const uint64_t n = band->n;
  if (n + 2 >= (1ull << 32))
    return fail(M2S_ERR_BAD_ARG, "%llu cells: the neighbour table holds 32-bit places, and two more are the backgrounds", (unsigned long long)n);
  m2s_opts o;
  rc = band_call_opts(band, opts, &o);
  if (rc) return rc;
  CallCtx c;
  DeviceState* st = nullptr;
  rc = resolve_ctx(&o, &c, &st);
  if (rc) return rc;

  const int kind = fl->kind;
  const uint64_t passes = (uint64_t)fl->iterations * (kind == M2S_FILTER_MEAN ? 3 : 1);
  const int n_slots = kind == M2S_FILTER_MEAN_CURVATURE ? kBfAllSlots : kBfAxisSlots;
  BfConst k;
  float r[3];
  for (int a = 0; a < 3; ++a) {
    r[a] = 1.0f / band->grid.cell_size[a];
    k.w[a] = r[a] * r[a];
    k.gs[a] = 0.5f * r[a];
  }
  k.xs[0] = 0.25f * (r[0] * r[1]);
  k.xs[1] = 0.25f * (r[0] * r[2]);
  k.xs[2] = 0.25f * (r[1] * r[2]);
  k.dt = 1.0f / (2.0f * ((k.w[0] + k.w[1]) + k.w[2]));
  const WalkGrid g = walk_grid_of(band->grid.cell_count, band->total, band->n_words);

  const uint64_t n_words = g.n_words;
  const uint64_t n_units = (n_words + kWalkUnit - 1) / kWalkUnit;   // below 2^22: a grid has fewer than 2^36 cells
  const unsigned blocks = (unsigned)((n_units + kWalkWaves - 1) / kWalkWaves);
  const size_t b_v = align_up((n + 2) * 4), b_slots = align_up((uint64_t)n_slots * n * 4 + 4), b_region = align_up(n + 1);
  const uint64_t cap = std::max<uint64_t>(n, 1);   // at least one float
  char* tmp = nullptr;     // two value buffers, the table, the region bytes: 33 or 81 bytes per active cell
  BandBlock res;           // the result
  auto drop = [&](int code) {
    (void)hipFree(tmp);
    res.free();
    return code;
  };
  auto hip_fail = [&](hipError_t e) { return drop(fail(M2S_ERR_HIP, "HIP error: %s", hipGetErrorString(e))); };
  rc = ensure_capacity(*st, 4096);
  if (rc) return rc;
  Arena ws{st->base, st->cap, 0};
  uint64_t* d_hdr = ws.take<uint64_t>(4);   // [0] n_nonfinite, [1] n_changed, [2] n_sign_flips, [3] the bits of max_change
  if (!d_hdr) return fail(M2S_ERR_HIP, "internal: workspace");
  hipError_t e = hipMalloc((void**)&tmp, 2 * b_v + b_slots + b_region);
  if (e == hipSuccess) e = res.alloc(n_words, cap);
  if (e != hipSuccess) return hip_fail(e);
  float* v[2] = {reinterpret_cast<float*>(tmp), reinterpret_cast<float*>(tmp + b_v)};
  uint32_t* slots = reinterpret_cast<uint32_t*>(tmp + 2 * b_v);
  uint8_t* in_region = reinterpret_cast<uint8_t*>(tmp + 2 * b_v + b_slots);
  const BandDev X = dev_of(band);
  const BandDev Wh = where ? dev_of(where) : X;
  hipStream_t s = c.stream;

  // ---- the table ----
  if (c.timings) e = hipEventRecord(st->ev[0], s);
  if (e == hipSuccess) e = hipMemsetAsync(d_hdr, 0, 32, s);
  if (e == hipSuccess) e = hipMemsetAsync(res.dist, 0, 4, s);   // an empty result still has one defined float
  if (e == hipSuccess) e = hipMemcpyAsync(res.mask, band->mask, n_words * 8, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(res.word_off, band->word_off, n_words * 8, hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return hip_fail(e);
  if (n_slots == kBfAllSlots)
    hipLaunchKernelGGL((k_bf_table<kBfAllSlots>), dim3(blocks), dim3(kWalkThreads), 0, s, X, Wh, where ? 1 : 0, g, slots, in_region, v[0], v[1]);
  else
    hipLaunchKernelGGL((k_bf_table<kBfAxisSlots>), dim3(blocks), dim3(kWalkThreads), 0, s, X, Wh, where ? 1 : 0, g, slots, in_region, v[0], v[1]);
  e = hipGetLastError();
  if (e == hipSuccess && c.timings) e = hipEventRecord(st->ev[1], s);
  if (e != hipSuccess) return hip_fail(e);

  // ---- the passes, back to back: pass p reads v[p & 1] and writes the other buffer ----
  const unsigned pass_blocks = blocks_for(n);
  if (n) {
    for (uint64_t p = 0; p < passes; ++p) {
      const float* v_in = v[p & 1];
      float* v_out = v[(p + 1) & 1];
      if (kind == M2S_FILTER_LAPLACIAN) launch_pass<M2S_FILTER_LAPLACIAN, 0>(s, pass_blocks, slots, in_region, v_in, v_out, n, k, d_hdr);
      else if (kind == M2S_FILTER_MEAN_CURVATURE) launch_pass<M2S_FILTER_MEAN_CURVATURE, 0>(s, pass_blocks, slots, in_region, v_in, v_out, n, k, d_hdr);
      else if (p % 3 == 0) launch_pass<M2S_FILTER_MEAN, 0>(s, pass_blocks, slots, in_region, v_in, v_out, n, k, d_hdr);
      else if (p % 3 == 1) launch_pass<M2S_FILTER_MEAN, 1>(s, pass_blocks, slots, in_region, v_in, v_out, n, k, d_hdr);
      else launch_pass<M2S_FILTER_MEAN, 2>(s, pass_blocks, slots, in_region, v_in, v_out, n, k, d_hdr);
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess && c.timings) e = hipEventRecord(st->ev[2], s);
  if (e != hipSuccess) return hip_fail(e);

  // ---- the result ----
  hipLaunchKernelGGL(k_bf_final, dim3(blocks), dim3(kWalkThreads), 0, s, X, g, (const float*)v[passes & 1], res.inside, res.dist, d_hdr);
  e = hipGetLastError();
  uint64_t hdr[4] = {0, 0, 0, 0};
  if (e == hipSuccess) e = hipMemcpyAsync(hdr, d_hdr, 32, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && c.timings) e = hipEventRecord(st->ev[3], s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);   // the call's one synchronisation
  if (e != hipSuccess) return hip_fail(e);
  if (c.timings) {
    float table_ms = 0.0f, pass_ms = 0.0f, total = 0.0f;
    (void)hipEventElapsedTime(&table_ms, st->ev[0], st->ev[1]);
    (void)hipEventElapsedTime(&pass_ms, st->ev[1], st->ev[2]);
    (void)hipEventElapsedTime(&total, st->ev[0], st->ev[3]);
    memset(c.timings, 0, sizeof(*c.timings));
    c.timings->seed_ms = table_ms;
    c.timings->distance_ms = pass_ms;
    c.timings->total_ms = total;
    c.timings->n_units = n;
    c.timings->distance_launches = (uint32_t)(n ? passes : 0);
  }
  (void)hipFree(tmp);
  if (info_out) {
    const uint32_t top = (uint32_t)hdr[3];
    info_out->passes = (uint32_t)passes;
    memcpy(&info_out->max_change, &top, 4);
    info_out->reserved = 0;
    info_out->n_changed = hdr[1];
    info_out->n_sign_flips = hdr[2];
    info_out->n_nonfinite = hdr[0];
  }
  *out = band_adopt(res, band->device, band->grid, n, g.total, n_words, fopts ? fopts->background_outside : band->bg_out,
                    fopts ? fopts->background_inside : band->bg_in);
  return M2S_OK;
}

}  // extern "C"
