// band_advect.hip — m2s_band_advect: the values of a resident band moved by first-order upwind steps, by a velocity per cell
// (phi_t + u . grad phi = 0) or a speed along the normal per cell (phi_t + F |grad phi| = 0, Godunov), gfx950.  The contract is
// include/m2s.h's (per grid point, to the bit); tests/band_advect_model.py restates it in numpy.  Nothing sized 4 bytes per grid point
// exists: the arrays are per mask word (the result's sign word) or per active cell.
//
// The table and the result are band_stencil.hip.h's kernels, the ones m2s_band_filter runs (6 slots, no region).
//   k_bf_table   per active cell, once: the list places of its 6 clamped neighbours, its value into the first value buffer.
//   k_ba_field   per active cell, once, in list order: the moving byte from the cell's field entry, n_moving, and max_cfl by an atomicMax on
//                the bits of a non-negative float; grid-stride, one atomic pair per block (32 bytes of LDS for the block's four waves).
//   k_ba_step    one Jacobi step, one lane per active cell: the slots, their values from the step's input buffer, the cell's field entry,
//                the arithmetic of the header, a store to the OTHER buffer; non-finite candidates counted by one atomic add per wave.  It
//                reads no index word and takes no branch per neighbour: the upwind choices are selects.
//   k_bf_final   the result's sign words, its values, n_changed, n_sign_flips and max_change.
// Bounds: a slot is below n + 2 (bf_slot), the value buffers hold n + 2 floats; a field entry is read at r < n only.
// All stores are plain vector stores; the table, step and final kernels use no LDS.
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
struct BaConst {
  float r[3];   // r_a = 1 / h_a
  float dt;
};

// counters: [0] n_nonfinite, [1] n_changed, [2] n_sign_flips, [3] the bits of max_change (k_bf_final's three), [4] n_moving,
// [5] the bits of max_cfl.
constexpr int kBaCounters = 6;
// k_ba_field's grid: two blocks of 256 for each of the 256 CUs, a streaming pass over 13 or 5 bytes a cell, and few enough that their two
// atomics each cost nothing.  Bands above 131 072 cells take the grid-stride loop (the 70 x 64 x 64 cases of the tests do).
constexpr unsigned kBaFieldBlocks = 512;

// Per active cell r, once: moving[r] = any component of its entry != 0 (a NaN is != 0); counters[4] += the moving cells;
// counters[5] = max(the bits of the cell's CFL figure where it is not a NaN): it is non-negative, and such floats order as their bits.
template <int KIND>
__global__ void __launch_bounds__(256) k_ba_field(const float* __restrict__ field, uint64_t n, BaConst k, uint8_t* __restrict__ moving,
                                                  uint64_t* __restrict__ counters) {
  uint32_t n_moving = 0, top = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (uint64_t)gridDim.x * 256) {
    bool mv;
    float cfl;
    if (KIND == M2S_ADVECT_VELOCITY) {
      const float ui = field[3 * r], uj = field[3 * r + 1], uk = field[3 * r + 2];
      mv = ui != 0.0f || uj != 0.0f || uk != 0.0f;
      cfl = k.dt * ((fabsf(ui) * k.r[0] + fabsf(uj) * k.r[1]) + fabsf(uk) * k.r[2]);
    } else {
      const float f = field[r];
      mv = f != 0.0f;
      cfl = k.dt * (fabsf(f) * ((k.r[0] + k.r[1]) + k.r[2]));
    }
    moving[r] = mv ? 1 : 0;
    n_moving += mv ? 1u : 0u;
    const uint32_t bits = cfl == cfl ? __float_as_uint(cfl) : 0u;
    top = bits > top ? bits : top;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n_moving += __shfl_xor(n_moving, o, 64);
    const uint32_t other = __shfl_xor(top, o, 64);
    top = other > top ? other : top;
  }
  // one atomic pair per block, not per wave: at one cell per lane the waves' atomics on two addresses cost more than the pass itself
  __shared__ uint32_t wave_moving[4], wave_top[4];
  if ((threadIdx.x & 63) == 0) {
    wave_moving[threadIdx.x >> 6] = n_moving;
    wave_top[threadIdx.x >> 6] = top;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    n_moving = (wave_moving[0] + wave_moving[1]) + (wave_moving[2] + wave_moving[3]);
    top = max(max(wave_top[0], wave_top[1]), max(wave_top[2], wave_top[3]));
    if (n_moving) atomicAdd((unsigned long long*)(counters + 4), (unsigned long long)n_moving);
    if (top) atomicMax((unsigned int*)(counters + 5), top);
  }
}

// One Jacobi step, one lane per active cell: v_out[r] = moving and finite ? cand : c, from v_in only (v_out is the other buffer).
// KIND: m2s_advect_kind.  counters[0] += the candidates that were not finite.
template <int KIND>
__global__ void __launch_bounds__(256) k_ba_step(const uint32_t* __restrict__ slots, const uint8_t* __restrict__ moving, const float* __restrict__ field,
                                                 const float* __restrict__ v_in, float* __restrict__ v_out, uint64_t n, BaConst k,
                                                 uint64_t* __restrict__ counters) {
  uint32_t bad = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (uint64_t)gridDim.x * 256) {
    const float c = v_in[r];
    float next = c;
    if (moving[r]) {
      float N[kBfAxisSlots];   // i+, i-, j+, j-, k+, k-
#pragma unroll
      for (int s = 0; s < kBfAxisSlots; ++s) N[s] = v_in[slots[(uint64_t)s * n + r]];
      float Dm[3], Dp[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        Dm[a] = (c - N[2 * a + 1]) * k.r[a];
        Dp[a] = (N[2 * a] - c) * k.r[a];
      }
      float cand;
      if (KIND == M2S_ADVECT_VELOCITY) {
        float t[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const float u = field[3 * r + a];
          t[a] = u > 0.0f ? u * Dm[a] : u * Dp[a];
        }
        cand = c - k.dt * ((t[0] + t[1]) + t[2]);
      } else {
        const float f = field[r];
        const bool grow = f > 0.0f;
        float q[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const float pos_m = Dm[a] > 0.0f ? Dm[a] : 0.0f, neg_m = Dm[a] < 0.0f ? Dm[a] : 0.0f;
          const float pos_p = Dp[a] > 0.0f ? Dp[a] : 0.0f, neg_p = Dp[a] < 0.0f ? Dp[a] : 0.0f;
          const float A = grow ? pos_m : neg_m, B = grow ? neg_p : pos_p;
          const float qa = A * A, qb = B * B;
          q[a] = qb > qa ? qb : qa;
        }
        const float g = sqrtf((q[0] + q[1]) + q[2]);
        cand = c - k.dt * (f * g);
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

}  // namespace

// m2s_warmup: the first launch of a kernel of this translation unit makes the runtime load its code object (all its kernels).
__global__ void k_warm_band_advect() {}
void warm_band_advect(hipStream_t st) { hipLaunchKernelGGL(k_warm_band_advect, dim3(1), dim3(64), 0, st); }

}  // namespace m2s

using namespace m2s;

extern "C" {

int m2s_band_advect(const m2s_band* band, const float* field, const m2s_band_advect_opts* aopts, const m2s_band_field_opts* fopts,
                    const m2s_opts* opts, m2s_band** out, m2s_band_advect_info* info_out) {
  clear_error();
  if (!out) return fail(M2S_ERR_BAD_ARG, "out is NULL");
  *out = nullptr;
  if (!band) return fail(M2S_ERR_BAD_ARG, "band is NULL");
  if (!aopts) return fail(M2S_ERR_BAD_ARG, "m2s_band_advect_opts is NULL");
  if (aopts->struct_size != sizeof(m2s_band_advect_opts))
    return fail(M2S_ERR_BAD_ARG, "m2s_band_advect_opts.struct_size is not sizeof(m2s_band_advect_opts)");
  if (aopts->kind != M2S_ADVECT_VELOCITY && aopts->kind != M2S_ADVECT_NORMAL) return fail(M2S_ERR_BAD_ARG, "bad m2s_advect_kind %d", aopts->kind);
  if (aopts->scheme != 0) return fail(M2S_ERR_BAD_ARG, "scheme = %u: must be 0 (first-order upwind)", aopts->scheme);
  if (aopts->steps == 0 || aopts->steps > 65536) return fail(M2S_ERR_BAD_ARG, "steps = %u: must be 1 .. 65536", aopts->steps);
  if (!(std::isfinite(aopts->dt) && aopts->dt > 0.0f)) return fail(M2S_ERR_BAD_ARG, "dt = %g: must be finite and > 0", (double)aopts->dt);
  int rc = band_field_opts_args(fopts);
  if (rc) return rc;
  if (info_out && info_out->struct_size != sizeof(m2s_band_advect_info))
    return fail(M2S_ERR_BAD_ARG, "m2s_band_advect_info.struct_size is not sizeof(m2s_band_advect_info)");
  rc = band_opts_args(opts, "m2s_band_advect");
  if (rc) return rc;
  const uint64_t n = band->n;
  if (!field && n > 0) return fail(M2S_ERR_BAD_ARG, "field is NULL with %llu cells", (unsigned long long)n);
  if (n + 2 >= (1ull << 32))
    return fail(M2S_ERR_BAD_ARG, "%llu cells: the neighbour table holds 32-bit places, and two more are the backgrounds", (unsigned long long)n);
  m2s_opts o;
  rc = band_call_opts(band, opts, &o);
  if (rc) return rc;
  CallCtx c;
  DeviceState* st = nullptr;
  rc = resolve_ctx(&o, &c, &st);
  if (rc) return rc;

  const int kind = aopts->kind;
  const uint64_t steps = aopts->steps;
  const bool host = c.mem_kind == M2S_MEM_HOST;
  const uint64_t per_cell = kind == M2S_ADVECT_VELOCITY ? 3 : 1;   // the floats of a field entry
  BaConst k;
  for (int a = 0; a < 3; ++a) k.r[a] = 1.0f / band->grid.cell_size[a];
  k.dt = aopts->dt;
  const WalkGrid g = walk_grid_of(band->grid.cell_count, band->total, band->n_words);

  const uint64_t n_words = g.n_words;
  const uint64_t n_units = (n_words + kWalkUnit - 1) / kWalkUnit;   // below 2^22: a grid has fewer than 2^36 cells
  const unsigned blocks = (unsigned)((n_units + kWalkWaves - 1) / kWalkWaves);
  const size_t b_v = align_up((n + 2) * 4), b_slots = align_up((uint64_t)kBfAxisSlots * n * 4 + 4), b_moving = align_up(n + 1);
  const size_t b_field = host ? align_up(per_cell * n * 4 + 4) : 0;
  const uint64_t cap = std::max<uint64_t>(n, 1);   // at least one float
  char* tmp = nullptr;     // two value buffers, the table, the moving bytes, a host caller's field: 33 bytes per active cell, and 12 or 4
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
  uint64_t* d_hdr = ws.take<uint64_t>(kBaCounters);
  if (!d_hdr) return fail(M2S_ERR_HIP, "internal: workspace");
  hipError_t e = hipMalloc((void**)&tmp, 2 * b_v + b_slots + b_moving + b_field);
  if (e == hipSuccess) e = res.alloc(n_words, cap);
  if (e != hipSuccess) return hip_fail(e);
  float* v[2] = {reinterpret_cast<float*>(tmp), reinterpret_cast<float*>(tmp + b_v)};
  uint32_t* slots = reinterpret_cast<uint32_t*>(tmp + 2 * b_v);
  uint8_t* moving = reinterpret_cast<uint8_t*>(tmp + 2 * b_v + b_slots);
  const float* d_field = field;
  const BandDev X = dev_of(band);
  hipStream_t s = c.stream;
  if (host && n) {
    float* copy = reinterpret_cast<float*>(tmp + 2 * b_v + b_slots + b_moving);
    e = hipMemcpyAsync(copy, field, per_cell * n * 4, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return hip_fail(e);
    d_field = copy;
  }

  // ---- the table: the neighbour places, then the moving bytes over the bytes the table kernel set to 1 ----
  const unsigned cell_blocks = blocks_for(n);
  const unsigned field_blocks = std::min(cell_blocks, kBaFieldBlocks);
  if (c.timings) e = hipEventRecord(st->ev[0], s);
  if (e == hipSuccess) e = hipMemsetAsync(d_hdr, 0, kBaCounters * 8, s);
  if (e == hipSuccess) e = hipMemsetAsync(res.dist, 0, 4, s);   // an empty result still has one defined float
  if (e == hipSuccess) e = hipMemcpyAsync(res.mask, band->mask, n_words * 8, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(res.word_off, band->word_off, n_words * 8, hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return hip_fail(e);
  hipLaunchKernelGGL((k_bf_table<kBfAxisSlots>), dim3(blocks), dim3(kWalkThreads), 0, s, X, X, 0, g, slots, moving, v[0], v[1]);
  if (n) {
    if (kind == M2S_ADVECT_VELOCITY) hipLaunchKernelGGL((k_ba_field<M2S_ADVECT_VELOCITY>), dim3(field_blocks), dim3(256), 0, s, d_field, n, k, moving, d_hdr);
    else hipLaunchKernelGGL((k_ba_field<M2S_ADVECT_NORMAL>), dim3(field_blocks), dim3(256), 0, s, d_field, n, k, moving, d_hdr);
  }
  e = hipGetLastError();
  if (e == hipSuccess && c.timings) e = hipEventRecord(st->ev[1], s);
  if (e != hipSuccess) return hip_fail(e);

  // ---- the steps, back to back: step p reads v[p & 1] and writes the other buffer ----
  if (n) {
    for (uint64_t p = 0; p < steps; ++p) {
      const float* v_in = v[p & 1];
      float* v_out = v[(p + 1) & 1];
      if (kind == M2S_ADVECT_VELOCITY)
        hipLaunchKernelGGL((k_ba_step<M2S_ADVECT_VELOCITY>), dim3(cell_blocks), dim3(256), 0, s, (const uint32_t*)slots, (const uint8_t*)moving, d_field, v_in, v_out, n, k, d_hdr);
      else
        hipLaunchKernelGGL((k_ba_step<M2S_ADVECT_NORMAL>), dim3(cell_blocks), dim3(256), 0, s, (const uint32_t*)slots, (const uint8_t*)moving, d_field, v_in, v_out, n, k, d_hdr);
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess && c.timings) e = hipEventRecord(st->ev[2], s);
  if (e != hipSuccess) return hip_fail(e);

  // ---- the result ----
  hipLaunchKernelGGL(k_bf_final, dim3(blocks), dim3(kWalkThreads), 0, s, X, g, (const float*)v[steps & 1], res.inside, res.dist, d_hdr);
  e = hipGetLastError();
  uint64_t hdr[kBaCounters] = {0, 0, 0, 0, 0, 0};
  if (e == hipSuccess) e = hipMemcpyAsync(hdr, d_hdr, kBaCounters * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && c.timings) e = hipEventRecord(st->ev[3], s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);   // the call's one synchronisation
  if (e != hipSuccess) return hip_fail(e);
  if (c.timings) {
    float table_ms = 0.0f, step_ms = 0.0f, total = 0.0f;
    (void)hipEventElapsedTime(&table_ms, st->ev[0], st->ev[1]);
    (void)hipEventElapsedTime(&step_ms, st->ev[1], st->ev[2]);
    (void)hipEventElapsedTime(&total, st->ev[0], st->ev[3]);
    memset(c.timings, 0, sizeof(*c.timings));
    c.timings->seed_ms = table_ms;
    c.timings->distance_ms = step_ms;
    c.timings->total_ms = total;
    c.timings->n_units = n;
    c.timings->distance_launches = (uint32_t)(n ? steps : 0);
  }
  (void)hipFree(tmp);
  if (info_out) {
    const uint32_t change = (uint32_t)hdr[3], cfl = (uint32_t)hdr[5];
    info_out->steps = (uint32_t)steps;
    memcpy(&info_out->max_change, &change, 4);
    memcpy(&info_out->max_cfl, &cfl, 4);
    info_out->n_moving = hdr[4];
    info_out->n_changed = hdr[1];
    info_out->n_sign_flips = hdr[2];
    info_out->n_nonfinite = hdr[0];
  }
  *out = band_adopt(res, band->device, band->grid, n, g.total, n_words, fopts ? fopts->background_outside : band->bg_out,
                    fopts ? fopts->background_inside : band->bg_in);
  return M2S_OK;
}

}  // extern "C"
