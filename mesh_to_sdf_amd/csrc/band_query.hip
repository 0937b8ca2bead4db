// band_query.hip — m2s_band_create / m2s_band_sample / m2s_band_raymarch: the grid queries of grid_query.hip on a narrow band behind a
// resident index, gfx950.  The contract is include/m2s.h's: the dense m2s_sample_grid / m2s_raymarch_grid on the grid D' the band stands
// for (its values on the band's cells, a signed background elsewhere), bit for bit, and no array sized by 4 bytes per grid point exists.
// tests/band_query_model.py restates it in numpy.
//
// The handle (band_handle.h, shared with the other band calls) owns, in device memory:
//   mask      1 bit per grid point, word L >> 6, bit L & 63            k_biso_mask (isosurface.hip.h: the index m2s_band_isosurface builds)
//   word_off  per mask word: the list place of its first active point  k_biso_mask; zeroed first, so every word is defined
//   dist      the band's distances, in list order                      a copy
//   inside    the sign mask, re-laid to the mask's layout              k_bq_sign (only when the caller gave inside_bits)
// The index costs 1 bit + 8 bytes per 64 grid points (1 GiB + 1 GiB at 2048^3, where a dense grid is 32 GiB), as in band_isosurface; the sign mask one more bit per
// point.  The caller's inside_bits are addressed by (i, j, k); re-laid by L they are read at the mask word's own index, so a corner's
// sign costs one more load in the first round and no division.
//
// The arithmetic is grid_query.hip.h's prepare / combine, shared with grid_query.hip under the same fp contract pragma.  What is new is
// the fetch of a sample's K cell values (fetch_rounds, in band_fetch.hip.h, which band_resample.hip shares): all addresses first, then three
// rounds of independent loads —
//   1  the mask words of the corners (and the sign words),
//   2  the word_off of the words that hold an active corner,
//   3  the values of the active corners; an inactive corner takes its background by select.
// A corner whose mask word is the word of its lower z-neighbour (trilinear: corner c and c + 4; tetrahedral: the corner before it)
// reuses that word and its offset: 4 + 4 reads for a trilinear sample unless L & 63 == 63 puts the neighbour in the next word.  Both
// corners' list places are word_off + popcount(mask below the bit), so "the next list entry" needs no special case, and the z-clamp
// case (both reads the same cell) is the same word and the same bit.
// A normal fetches its six samples in groups: all six at once for SNAP and TETRAHEDRAL (24 corners), two groups of three for
// TRILINEAR — 48 corners hold 96 registers of offsets, 96 of mask words and 96 of sign words at the peak of round 1, which spills.
// The group size sets the kernel's registers, and with them the occupancy of the whole kernel, the march loop included: measured
// (profiles/band_query.txt), the larger groups win where normals dominate (m2s_band_sample) and the smaller ones in the march, whose loop
// fetches one sample at a time (16 trilinear / 12 tetrahedral corners per group: 189 / 136 VGPRs against 256 / 254).  M2S_BAND_FETCH: -1
// that choice, 0 / 2 the larger / smaller groups everywhere, 1 the per-corner chain (fetch_chain: mask, then offset, then value, corner
// after corner), which loses from 512^3 on.
#include "../../include/m2s.h"
#include "band_fetch.hip.h"
#include "band_handle.h"
#include "capi_internal.h"
#include "common.h"
#include "grid_query.hip.h"
#include "isosurface.hip.h"
#include "tuning.h"

#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace m2s {
namespace {

// The sign mask from the caller's layout uint32[nx][ny][ceil(nz / 32)] to the mask's (bit L & 63 of word L >> 6).  One lane per output
// word: the row and k of its first point by one division, then 64 steps along the list order.
__global__ void __launch_bounds__(256) k_bq_sign(uint64_t total, uint64_t nz, uint64_t n_words, const uint32_t* __restrict__ bits,
                                                 uint64_t* __restrict__ inside) {
  const uint64_t nzw = (nz + 31) / 32;
  for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * 256) {
    const uint64_t L0 = w << 6;
    uint64_t row = L0 / nz, k = L0 - row * nz;
    const uint64_t cnt = total - L0 < 64 ? total - L0 : 64;
    uint64_t acc = 0;
    uint64_t at = ~0ull;
    uint32_t word = 0;
    for (uint64_t b = 0; b < cnt; ++b) {
      const uint64_t idx = row * nzw + (k >> 5);
      if (idx != at) { word = bits[idx]; at = idx; }
      acc |= (uint64_t)((word >> (k & 31)) & 1u) << b;
      if (++k == nz) { k = 0; ++row; }
    }
    inside[w] = acc;
  }
}

// estimate_normal as grid_query.hip's normal(): the six samples in groups of G, each group's rounds issued together.
template <int MODE, bool SIGN, int FORM>
__device__ __forceinline__ void normal(const GridQuery& q, const BandDev& b, float px, float py, float pz, float* nrm) {
  // corners in flight per group: 24 (FORM 0: 3 trilinear samples, 6 tetrahedral), 16 / 12 (FORM 2: 2 trilinear, 3 tetrahedral); SNAP: all 6
  constexpr int G = MODE == M2S_SAMPLE_SNAP ? 6 : (MODE == M2S_SAMPLE_TRILINEAR ? (FORM == 2 ? 2 : 3) : (FORM == 2 ? 3 : 6));
  const float e = q.eps;
  float s[6];
#pragma unroll
  for (int h = 0; h < 6; h += G) {
    Prep<MODE> p[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      // px + e, px - e, ... exactly as normal() writes them: the untouched coordinates pass through unchanged
      const int i = h + j;
      p[j] = prepare<MODE>(q, i < 2 ? (i == 0 ? px + e : px - e) : px, (i == 2 || i == 3) ? (i == 2 ? py + e : py - e) : py,
                           i >= 4 ? (i == 4 ? pz + e : pz - e) : pz);
    }
    float v[G][Corners<MODE>::K];
    uint32_t sup[G];
    fetch<MODE, G, SIGN, FORM>(b, p, v, sup);
#pragma unroll
    for (int j = 0; j < G; ++j) s[h + j] = combine<MODE>(q, p[j], v[j]);
  }
  const float nx = s[0] - s[1], ny = s[2] - s[3], nz = s[4] - s[5];
  const float len = sqrtf(nx * nx + ny * ny + nz * nz);
  if (px != px || py != py || pz != pz) {
    nrm[0] = nrm[1] = nrm[2] = qnan();
  } else if (len == 0.0f) {
    nrm[0] = nrm[1] = nrm[2] = 0.0f;
  } else {
    nrm[0] = nx / len; nrm[1] = ny / len; nrm[2] = nz / len;
  }
}

template <int MODE, bool SIGN, int FORM>
__global__ __launch_bounds__(256) void k_band_sample(GridQuery q, BandDev b, const float* __restrict__ pts, uint64_t n, float* __restrict__ value_out,
                                                     float* __restrict__ normal_out, uint8_t* __restrict__ support_out) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    if (value_out || support_out) {
      uint32_t sup;
      const float val = sample<MODE, SIGN, FORM>(q, b, px, py, pz, &sup);
      if (value_out) value_out[i] = val;
      if (support_out) support_out[i] = (uint8_t)sup;
    }
    if (normal_out) {
      float nrm[3];
      normal<MODE, SIGN, FORM>(q, b, px, py, pz, nrm);
      normal_out[3 * i] = nrm[0]; normal_out[3 * i + 1] = nrm[1]; normal_out[3 * i + 2] = nrm[2];
    }
  }
}

// sdf_3d as grid_query.hip's k_raymarch_grid, statement for statement; the sample is the band's.
template <int MODE, bool SIGN, int FORM>
__global__ __launch_bounds__(256) void k_band_raymarch(GridQuery q, BandDev b, const float* __restrict__ org, const float* __restrict__ dir, uint64_t n,
                                                       float* __restrict__ hit_out, uint32_t* __restrict__ steps_out, float* __restrict__ normal_out,
                                                       uint8_t* __restrict__ support_out) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const float ox = org[3 * i], oy = org[3 * i + 1], oz = org[3 * i + 2];
    const float dx = dir[3 * i], dy = dir[3 * i + 1], dz = dir[3 * i + 2];
    float px = ox, py = oy, pz = oz, dist = 0.0f;
    uint32_t steps = 0, sup = 0;
    bool march = true;
    if (ox != ox || oy != oy || oz != oz || dx != dx || dy != dy || dz != dz) {
      px = py = pz = dist = qnan();
      march = false;
    } else if (ox < q.start[0] || oy < q.start[1] || oz < q.start[2] || ox > q.end[0] || oy > q.end[1] || oz > q.end[2]) {
      const float t0x = (q.start[0] - ox) / dx, t0y = (q.start[1] - oy) / dy, t0z = (q.start[2] - oz) / dz;
      const float t1x = (q.end[0] - ox) / dx, t1y = (q.end[1] - oy) / dy, t1z = (q.end[2] - oz) / dz;
      const float nx = fminf(t0x, t1x), ny = fminf(t0y, t1y), nz = fminf(t0z, t1z);
      const float fx = fmaxf(t0x, t1x), fy = fmaxf(t0y, t1y), fz = fmaxf(t0z, t1z);
      const float t_near = fmaxf(fmaxf(nx, ny), nz);
      const float t_far = fminf(fminf(fx, fy), fz);
      if (t_near > t_far) {
        px = py = pz = 0.0f;
        dist = 1.0f;
        march = false;
      } else {
        const float t = t_near + q.eps;
        px = ox + t * dx; py = oy + t * dy; pz = oz + t * dz;
      }
    }
    if (march) {
      for (uint32_t s = 0; s < q.max_steps; ++s) {
        dist = sample<MODE, SIGN, FORM>(q, b, px, py, pz, &sup);   // sup: the support of the last sample evaluated
        if (dist < q.eps) break;
        px = px + dx * dist; py = py + dy * dist; pz = pz + dz * dist;
        ++steps;
      }
    }
    if (hit_out) { hit_out[4 * i] = px; hit_out[4 * i + 1] = py; hit_out[4 * i + 2] = pz; hit_out[4 * i + 3] = dist; }
    if (steps_out) steps_out[i] = steps;
    if (support_out) support_out[i] = (uint8_t)sup;
    if (normal_out) {
      float nrm[3] = {0.0f, 0.0f, 0.0f};
      if (march && dist < q.eps) normal<MODE, SIGN, FORM>(q, b, px, py, pz, nrm);
      normal_out[3 * i] = nrm[0]; normal_out[3 * i + 1] = nrm[1]; normal_out[3 * i + 2] = nrm[2];
    }
  }
}

template <int MODE, bool SIGN, int FORM>
void launch_sample_as(hipStream_t st, const GridQuery& q, const BandDev& b, const float* pts, uint64_t n, float* value_out, float* normal_out,
                      uint8_t* support_out) {
  hipLaunchKernelGGL((k_band_sample<MODE, SIGN, FORM>), dim3(blocks_for(n)), dim3(256), 0, st, q, b, pts, n, value_out, normal_out, support_out);
}

template <int MODE, bool SIGN, int FORM>
void launch_march_as(hipStream_t st, const GridQuery& q, const BandDev& b, const float* org, const float* dir, uint64_t n, float* hit_out,
                     uint32_t* steps_out, float* normal_out, uint8_t* support_out) {
  hipLaunchKernelGGL((k_band_raymarch<MODE, SIGN, FORM>), dim3(blocks_for(n)), dim3(256), 0, st, q, b, org, dir, n, hit_out, steps_out, normal_out,
                     support_out);
}

// mode x sign mask x fetch form -> the instantiation; AUTO is the form M2S_BAND_FETCH = -1 stands for in this kernel
#define M2S_BQ_DISPATCH(AUTO, CALL, ...)                                                         \
  do {                                                                                      \
    const bool sign_ = b.inside != nullptr;                                                 \
    const int form_ = tuning().band_fetch < 0 ? AUTO : tuning().band_fetch;                 \
    switch (mode) {                                                                         \
      case M2S_SAMPLE_SNAP: M2S_BQ_FORMS(CALL, M2S_SAMPLE_SNAP, __VA_ARGS__); break;          \
      case M2S_SAMPLE_TRILINEAR: M2S_BQ_FORMS(CALL, M2S_SAMPLE_TRILINEAR, __VA_ARGS__); break; \
      default: M2S_BQ_FORMS(CALL, M2S_SAMPLE_TETRAHEDRAL, __VA_ARGS__); break;                \
    }                                                                                       \
  } while (0)
#define M2S_BQ_FORMS(CALL, MODE, ...)                                      \
  do {                                                                     \
    if (sign_) {                                                           \
      if (form_ == 1) CALL<MODE, true, 1>(__VA_ARGS__);                    \
      else if (form_ == 2) CALL<MODE, true, 2>(__VA_ARGS__);               \
      else CALL<MODE, true, 0>(__VA_ARGS__);                               \
    } else {                                                               \
      if (form_ == 1) CALL<MODE, false, 1>(__VA_ARGS__);                   \
      else if (form_ == 2) CALL<MODE, false, 2>(__VA_ARGS__);              \
      else CALL<MODE, false, 0>(__VA_ARGS__);                              \
    }                                                                      \
  } while (0)

int launch_band_sample(hipStream_t st, const GridQuery& q, int mode, const BandDev& b, const float* pts, uint64_t n, float* value_out,
                       float* normal_out, uint8_t* support_out) {
  if (n == 0) return 0;
  M2S_BQ_DISPATCH(0, launch_sample_as, st, q, b, pts, n, value_out, normal_out, support_out);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_band_raymarch(hipStream_t st, const GridQuery& q, int mode, const BandDev& b, const float* org, const float* dir, uint64_t n,
                         float* hit_out, uint32_t* steps_out, float* normal_out, uint8_t* support_out) {
  if (n == 0) return 0;
  M2S_BQ_DISPATCH(2, launch_march_as, st, q, b, org, dir, n, hit_out, steps_out, normal_out, support_out);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace

// m2s_warmup: the first launch of a kernel of this translation unit makes the runtime load its code object (all its kernels).
__global__ void k_warm_band_query() {}
void warm_band_query(hipStream_t st) { hipLaunchKernelGGL(k_warm_band_query, dim3(1), dim3(64), 0, st); }

}  // namespace m2s

using namespace m2s;

extern "C" {

int m2s_band_create(const m2s_grid* grid, const uint64_t* cells, const float* distances, uint64_t n_cells, const uint32_t* inside_bits,
                    const m2s_band_field_opts* fopts, const m2s_opts* opts, m2s_band** out) {
  clear_error();
  if (!out) return fail(M2S_ERR_BAD_ARG, "out is NULL");
  *out = nullptr;
  if (!grid) return fail(M2S_ERR_BAD_ARG, "grid is NULL");
  if (!fopts) return fail(M2S_ERR_BAD_ARG, "m2s_band_field_opts is NULL: the backgrounds have no default");
  int rc = band_field_opts_args(fopts);
  if (rc) return rc;
  if (n_cells && (!cells || !distances)) return fail(M2S_ERR_BAD_ARG, "cells / distances is NULL with n_cells > 0");
  rc = band_opts_args(opts, "m2s_band_create");
  if (rc) return rc;
  GridQuery q;
  int mode = 0;
  rc = grid_query_args(grid, nullptr, false, nullptr, &q, &mode);   // what m2s_sample_grid rejects of a grid
  if (rc) return rc;
  const uint64_t nx = grid->cell_count[0], ny = grid->cell_count[1], nz = grid->cell_count[2];
  uint64_t total = 0, n_words = 0;
  rc = band_grid_cells(grid, "grid", &total, &n_words);
  if (rc) return rc;
  if (n_cells > total) return fail(M2S_ERR_BAD_ARG, "n_cells = %llu above the grid's %llu cells", (unsigned long long)n_cells, (unsigned long long)total);
  const bool host = !opts || opts->mem_kind == M2S_MEM_HOST;
  if (host) {   // host memory: the list and its values are judged here, before any device work
    for (uint64_t a = 0; a < n_cells; ++a)
      if (cells[a] >= total || (a && cells[a - 1] >= cells[a]))
        return fail(M2S_ERR_BAD_ARG, "cells[%llu] = %llu is not above its predecessor or not below the grid's %llu cells", (unsigned long long)a,
                    (unsigned long long)cells[a], (unsigned long long)total);
    for (uint64_t a = 0; a < n_cells; ++a)
      if (!std::isfinite(distances[a])) return fail(M2S_ERR_NAN, "distances[%llu] is NaN or infinite", (unsigned long long)a);
  }
  CallCtx c;
  DeviceState* st = nullptr;
  rc = resolve_ctx(opts, &c, &st);
  if (rc) return rc;
  const uint64_t n = n_cells;
  const uint64_t sign_words = (nz + 31) / 32 * nx * ny;
  // the handle's block: mask, word_off, [inside], dist (at least one float)
  BandBlock res;
  M2S_HIP_CHECK(res.alloc(n_words, n ? n : 1, inside_bits != nullptr));
  auto drop = [&](int code) { res.free(); return code; };
  // the workspace: the flag and, for host memory, the staged list and sign mask
  size_t need = 4096 + 256;
  if (host) need += align_up(n * 8) + (inside_bits ? align_up(sign_words * 4) : 0);
  rc = ensure_capacity(*st, need);
  if (rc) return drop(rc);
  Arena ws{st->base, st->cap, 0};
  uint32_t* d_flag = reinterpret_cast<uint32_t*>(ws.take<uint64_t>(4));
  if (!d_flag) return drop(fail(M2S_ERR_HIP, "internal: workspace"));
  const uint64_t* dc = cells;
  const uint32_t* db = inside_bits;
  if (host) {
    if (n) {
      char* sc = ws.take<char>(n * 8);
      if (!sc) return drop(fail(M2S_ERR_HIP, "internal: workspace"));
      if ((rc = staged_h2d(*st, c.stream, sc, reinterpret_cast<const char*>(cells), n * 8))) return drop(rc);
      if ((rc = staged_h2d(*st, c.stream, reinterpret_cast<char*>(res.dist), reinterpret_cast<const char*>(distances), n * 4))) return drop(rc);
      dc = reinterpret_cast<const uint64_t*>(sc);
    }
    if (inside_bits) {
      char* sb = ws.take<char>(sign_words * 4);
      if (!sb) return drop(fail(M2S_ERR_HIP, "internal: workspace"));
      if ((rc = staged_h2d(*st, c.stream, sb, reinterpret_cast<const char*>(inside_bits), sign_words * 4))) return drop(rc);
      db = reinterpret_cast<const uint32_t*>(sb);
    }
  } else if (n) {
    if (hipMemcpyAsync(res.dist, distances, n * 4, hipMemcpyDeviceToDevice, c.stream) != hipSuccess) return drop(fail(M2S_ERR_HIP, "hipMemcpyAsync failed"));
  }
  hipError_t e = hipSuccess;
  if (c.timings) e = hipEventRecord(st->ev[0], c.stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_flag, 0, 32, c.stream);
  if (e == hipSuccess) e = hipMemsetAsync(res.mask, 0, align_up(n_words * 8) * 2, c.stream);   // the mask and every word's offset
  if (e == hipSuccess && n == 0) e = hipMemsetAsync(res.dist, 0, 4, c.stream);
  if (e != hipSuccess) return drop(fail(M2S_ERR_HIP, "HIP error: %s", hipGetErrorString(e)));
  if (n)
    hipLaunchKernelGGL(k_biso_mask, dim3((unsigned)((n + kMaskThreads - 1) / kMaskThreads)), dim3(kMaskThreads), 0, c.stream, total, dc,
                       (const float*)res.dist, n, res.mask, res.word_off, d_flag);
  if (inside_bits)
    hipLaunchKernelGGL(k_bq_sign, dim3(blocks_for(n_words)), dim3(256), 0, c.stream, total, nz, n_words, db, res.inside);
  e = hipGetLastError();
  if (e == hipSuccess && c.timings) e = hipEventRecord(st->ev[1], c.stream);
  uint32_t raised[2] = {0, 0};
  if (e == hipSuccess) e = hipMemcpyAsync(raised, d_flag, 8, hipMemcpyDeviceToHost, c.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
  if (e != hipSuccess) return drop(fail(M2S_ERR_HIP, "HIP error: %s", hipGetErrorString(e)));
  if (raised[0] & kFlagOrder) return drop(fail(M2S_ERR_BAD_ARG, "cells is not strictly ascending or holds an entry at or above the grid's cell count"));
  if (raised[0] & kFlagNonFinite) return drop(fail(M2S_ERR_NAN, "the band holds a NaN or infinite distance"));
  if (c.timings) {
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, st->ev[0], st->ev[1]);
    memset(c.timings, 0, sizeof(*c.timings));
    c.timings->seed_ms = ms;
    c.timings->total_ms = ms;
    c.timings->n_units = n_cells;
  }
  *out = band_adopt(res, c.device, *grid, n, total, n_words, fopts->background_outside, fopts->background_inside);
  return M2S_OK;
}

void m2s_band_destroy(m2s_band* band) {
  if (!band) return;
  if (band->block || band->block2) {
    int cur = -1;
    const bool have = hipGetDevice(&cur) == hipSuccess;
    if (hipSetDevice(band->device) == hipSuccess) {
      (void)hipDeviceSynchronize();   // queries still in flight read the block
      (void)hipFree(band->block);
      (void)hipFree(band->block2);
    }
    if (have) (void)hipSetDevice(cur);
  }
  delete band;
}

int m2s_band_info(const m2s_band* band, m2s_grid* grid, uint64_t* n_cells, uint64_t* device_bytes) {
  clear_error();
  if (!band) return fail(M2S_ERR_BAD_ARG, "band is NULL");
  if (grid) *grid = band->grid;
  if (n_cells) *n_cells = band->n;
  if (device_bytes) *device_bytes = band->device_bytes;
  return M2S_OK;
}

int m2s_band_sample(const m2s_band* band, const float* points, size_t n_points, const m2s_sample_opts* sopts, float* value_out,
                    float* normal_out, uint8_t* support_out, const m2s_opts* opts) {
  clear_error();
  if (!band) return fail(M2S_ERR_BAD_ARG, "band is NULL");
  GridQuery q;
  int mode = 0;
  int rc = grid_query_args(&band->grid, sopts, false, opts, &q, &mode);
  if (rc) return rc;
  if (!value_out && !normal_out) return fail(M2S_ERR_BAD_ARG, "no output requested (support_out alone is none)");
  if (n_points && !points) return fail(M2S_ERR_BAD_ARG, "points is NULL");
  m2s_opts o;
  rc = band_call_opts(band, opts, &o);
  if (rc) return rc;
  if (n_points == 0) {
    if (opts && opts->timings) memset(opts->timings, 0, sizeof(*opts->timings));
    return M2S_OK;
  }
  const BandDev b = dev_of(band);
  QueryIo io[4] = {{points, n_points * 12, false}, {value_out, value_out ? n_points * 4 : 0, true}, {normal_out, normal_out ? n_points * 12 : 0, true},
                   {support_out, support_out ? n_points : 0, true}};
  return run_query(&o, io, 4, n_points, [&](hipStream_t s) {
    return launch_band_sample(s, q, mode, b, reinterpret_cast<const float*>(io[0].dev), n_points, value_out ? reinterpret_cast<float*>(io[1].dev) : nullptr,
                              normal_out ? reinterpret_cast<float*>(io[2].dev) : nullptr, support_out ? reinterpret_cast<uint8_t*>(io[3].dev) : nullptr);
  });
}

int m2s_band_raymarch(const m2s_band* band, const float* origins, const float* directions, size_t n_rays, const m2s_sample_opts* sopts,
                      float* hit_out, uint32_t* steps_out, float* normal_out, uint8_t* support_out, const m2s_opts* opts) {
  clear_error();
  if (!band) return fail(M2S_ERR_BAD_ARG, "band is NULL");
  GridQuery q;
  int mode = 0;
  int rc = grid_query_args(&band->grid, sopts, true, opts, &q, &mode);
  if (rc) return rc;
  if (!hit_out && !steps_out && !normal_out) return fail(M2S_ERR_BAD_ARG, "no output requested (support_out alone is none)");
  if (n_rays && (!origins || !directions)) return fail(M2S_ERR_BAD_ARG, "origins / directions is NULL");
  m2s_opts o;
  rc = band_call_opts(band, opts, &o);
  if (rc) return rc;
  if (n_rays == 0) {
    if (opts && opts->timings) memset(opts->timings, 0, sizeof(*opts->timings));
    return M2S_OK;
  }
  const BandDev b = dev_of(band);
  QueryIo io[6] = {{origins, n_rays * 12, false}, {directions, n_rays * 12, false}, {hit_out, hit_out ? n_rays * 16 : 0, true},
                   {steps_out, steps_out ? n_rays * 4 : 0, true}, {normal_out, normal_out ? n_rays * 12 : 0, true},
                   {support_out, support_out ? n_rays : 0, true}};
  return run_query(&o, io, 6, n_rays, [&](hipStream_t s) {
    return launch_band_raymarch(s, q, mode, b, reinterpret_cast<const float*>(io[0].dev), reinterpret_cast<const float*>(io[1].dev), n_rays,
                                hit_out ? reinterpret_cast<float*>(io[2].dev) : nullptr, steps_out ? reinterpret_cast<uint32_t*>(io[3].dev) : nullptr,
                                normal_out ? reinterpret_cast<float*>(io[4].dev) : nullptr, support_out ? reinterpret_cast<uint8_t*>(io[5].dev) : nullptr);
  });
}

}  // extern "C"
