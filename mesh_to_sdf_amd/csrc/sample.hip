// sample.hip — area-weighted surface sampling (m2s_sample_surface, m2s_mesh_sample_surface), gfx950.  DESIGN.md §4.11.
//
// The contract is include/m2s.h's and its arithmetic is sample.hip.h; tests/sample_model.py restates both in numpy and the GPU tests
// compare the two bit for bit.  Three stages on the call's stream:
//   k_tri_area      A_t = |(b - a) x (c - a)| per triangle, in the caller's triangle order, and Amax: a wave reduction, a workgroup
//                   reduction and one atomicMax per workgroup on the bit pattern (A_t >= 0, so unsigned order is float order).  The
//                   one-shot call reads the caller's vertices and indices (no tree is built), a persistent mesh reads its resident
//                   `corners` through `slot_of`.
//   the table       w_t = floor(A_t 2^(37 - e)) and C = their inclusive running sums in uint64, by the two-level pattern of
//                   scan.hip.h: k_weight_sums (one sum per tile of 4096 triangles), k_weight_scan_tiles (the tile sums, one workgroup;
//                   its total is W), k_weight_scan (each tile again, now with its offset).  At the limit of 2^25 triangles that is
//                   8192 tiles, 32 per thread of the middle pass.  k_table_top then copies an evenly strided SAMPLE_TOP entries of C.
//                   The sums are integers: any order gives the same table.
//   k_sample        one sample per lane: Philox, the pick, the fold, the point, the normal.
//
// ---- k_sample's shape ---------------------------------------------------------------------------------------------------------------
// The pick is a binary search, log2(n_tris) DEPENDENT loads per lane (17 at 100 k triangles), each lane on a path of its own.  The top
// 11 levels are taken out of memory: `top` holds C[(j + 1) 2^shift - 1] for at most SAMPLE_TOP = 2048 values of j (16 KB), every
// workgroup copies it into LDS once and then serves 2048 samples from it, so a lane searches `top` in LDS and only the last `shift`
// levels — 6 at 100 k triangles, 9 at a million — in the 2^shift consecutive entries of C that its chunk spans (512 B to 4 KB: few
// cache lines, and the L2 holds all of C at these sizes).  Meshes of up to 2048 triangles never leave LDS.
// 16 KB of `top` + 3 KB of output staging per workgroup of 256 lets 8 workgroups share a CU's 160 KB: 32 waves per CU, the hardware's
// limit, cover the remaining levels.
// Outputs leave through LDS: a wave's 64 points are 768 contiguous bytes, so each wave transposes them in a slice of its own and
// stores three runs of 256 contiguous bytes instead of 64 stores 12 bytes apart; the normals and (u, v) likewise.
#include "common.h"
#include "geo.hip.h"
#include "sample.hip.h"
#include "scan.hip.h"

namespace m2s {

void warm_sample(hipStream_t st);

namespace {

__global__ void k_warm_sample() {}

constexpr int kThreads = kTileThreads;
constexpr int kSampleIters = 8;                    // samples per lane of k_sample: one copy of `top` serves 2048 samples

__device__ __forceinline__ uint32_t load_index(const void* idx, int index_bytes, size_t i) {
  if (idx == nullptr) return (uint32_t)i;
  return index_bytes == 2 ? (uint32_t)((const uint16_t*)idx)[i] : ((const uint32_t*)idx)[i];
}

// Triangle t of the caller's order; false (and a, b, c = 0): a vertex index out of range.
__device__ __forceinline__ bool load_triangle(const SampleSrc& s, uint32_t t, f3* a, f3* b, f3* c) {
  if (s.corners) {
    const size_t slot = s.slot_of[t];
    const float4 c0 = s.corners[3 * slot], c1 = s.corners[3 * slot + 1], c2 = s.corners[3 * slot + 2];
    *a = mk3(c0.x, c0.y, c0.z);
    *b = mk3(c0.w, c1.x, c1.y);
    *c = mk3(c1.z, c1.w, c2.x);
    return true;
  }
  const size_t base = s.topology == 0 ? (size_t)t * 3 : (size_t)t;   // list: consecutive triples; strip: a sliding window
  const uint32_t i0 = load_index(s.indices, s.index_bytes, base), i1 = load_index(s.indices, s.index_bytes, base + 1),
                 i2 = load_index(s.indices, s.index_bytes, base + 2);
  if (i0 >= s.n_verts || i1 >= s.n_verts || i2 >= s.n_verts) {
    *a = *b = *c = mk3(0.0f, 0.0f, 0.0f);
    return false;
  }
  *a = mk3(s.verts[3 * (size_t)i0], s.verts[3 * (size_t)i0 + 1], s.verts[3 * (size_t)i0 + 2]);
  *b = mk3(s.verts[3 * (size_t)i1], s.verts[3 * (size_t)i1 + 1], s.verts[3 * (size_t)i1 + 2]);
  *c = mk3(s.verts[3 * (size_t)i2], s.verts[3 * (size_t)i2 + 1], s.verts[3 * (size_t)i2 + 2]);
  return true;
}

// hdr[0]: the bits of Amax (cleared by the launcher);  hdr[2], hdr[3]: W, written by k_weight_scan_tiles.
__global__ __launch_bounds__(kThreads) void k_tri_area(SampleSrc src, float* __restrict__ A, uint32_t* __restrict__ hdr, int* __restrict__ err) {
  __shared__ uint32_t wave_max[kThreads / 64];
  const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
  uint32_t bits = 0;
  if (t < src.n_tris) {
    f3 a, b, c, n;
    if (!load_triangle(src, t, &a, &b, &c)) atomicOr(err, ERRF_INDEX_OOB);
    const float area = tri_weight_area(a, b, c, &n);
    A[t] = area;
    bits = __float_as_uint(area);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bits = max(bits, (uint32_t)__shfl_xor((int)bits, o, 64));
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = bits;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t m = wave_max[0];
    for (int w = 1; w < kThreads / 64; ++w) m = max(m, wave_max[w]);
    if (m) atomicMax(&hdr[0], m);
  }
}

// The weights of one tile, kScanItems consecutive triangles per thread; returns their sum.
__device__ __forceinline__ uint64_t tile_weights(const float* __restrict__ A, uint32_t n_tris, int e, uint64_t (&w)[kScanItems]) {
  const size_t first = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanItems;
  uint64_t s = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    w[k] = first + k < n_tris ? sample_weight(A[first + k], e) : 0;
    s += w[k];
  }
  return s;
}

__global__ __launch_bounds__(kThreads) void k_weight_sums(const float* __restrict__ A, uint32_t n_tris, const uint32_t* __restrict__ hdr,
                                                          uint64_t* __restrict__ tile_sum) {
  const uint32_t amax = hdr[0];
  if (amax == 0u) return;   // nothing the sampler can reach: W stays 0
  uint64_t w[kScanItems], all;
  const uint64_t s = tile_weights(A, n_tris, sample_exponent(__uint_as_float(amax)), w);
  (void)block_exclusive_scan<kThreads>(s, &all);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
}

// The tile sums scanned in place by one workgroup; their total is W.
__global__ __launch_bounds__(kThreads) void k_weight_scan_tiles(uint64_t* __restrict__ v, uint32_t n, uint32_t* __restrict__ hdr) {
  if (hdr[0] == 0u) return;
  uint64_t all;
  scan_tiles_in_place<kThreads, uint32_t>(v, n, &all);
  if (threadIdx.x == 0) *reinterpret_cast<uint64_t*>(hdr + 2) = all;
}

__global__ __launch_bounds__(kThreads) void k_weight_scan(const float* __restrict__ A, uint32_t n_tris, const uint32_t* __restrict__ hdr,
                                                          const uint64_t* __restrict__ tile_off, uint64_t* __restrict__ C) {
  const uint32_t amax = hdr[0];
  if (amax == 0u) return;
  uint64_t w[kScanItems], all;
  const uint64_t s = tile_weights(A, n_tris, sample_exponent(__uint_as_float(amax)), w);
  uint64_t run = tile_off[blockIdx.x] + block_exclusive_scan<kThreads>(s, &all);
  const size_t first = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanItems;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    run += w[k];
    if (first + k < n_tris) C[first + k] = run;
  }
}

// top[j] = the last entry of chunk j of C, chunks of 2^shift entries (the last one may be short).
__global__ __launch_bounds__(kThreads) void k_table_top(const uint64_t* __restrict__ C, uint32_t n_tris, uint32_t shift, uint32_t n_top,
                                                        const uint32_t* __restrict__ hdr, uint64_t* __restrict__ top) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (hdr[0] == 0u || j >= n_top) return;
  const uint64_t end = min(((uint64_t)j + 1) << shift, (uint64_t)n_tris);
  top[j] = C[end - 1];
}

// A wave's K floats per lane, transposed in the wave's slice `wb` (64 K floats of LDS) and stored as K runs of 64 consecutive floats
// from dst on; n_valid = the lanes of this wave that hold a sample (the call's last wave may be short).  Every thread of the workgroup
// calls it: the barriers order the slice's writes, its reads, and its next use.
template <int K>
__device__ __forceinline__ void wave_store(float* __restrict__ dst, const float (&v)[K], float* wb, int lane, uint32_t n_valid) {
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) wb[K * lane + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < K; ++r) {
    const uint32_t idx = (uint32_t)(r * 64 + lane);
    if (idx < (uint32_t)K * n_valid) dst[idx] = wb[idx];
  }
}

// Sample i of the call is global sample first + i.  LINEAR: the pick scans C from its first entry (algorithm 1, the validation form).
template <bool LINEAR>
__global__ __launch_bounds__(kThreads) void k_sample(SampleSrc src, const uint64_t* __restrict__ C, const uint64_t* __restrict__ top, uint32_t shift,
                                                     uint32_t n_top, uint64_t W, uint64_t seed, uint64_t first, uint64_t n_samples, SampleOut out) {
  __shared__ uint64_t s_top[LINEAR ? 1 : SAMPLE_TOP];
  __shared__ float s_stage[kThreads / 64][3 * 64];
  if (!LINEAR) {
    for (uint32_t j = threadIdx.x; j < n_top; j += kThreads) s_top[j] = top[j];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t block_first = (uint64_t)blockIdx.x * (kThreads * kSampleIters);
#pragma clang loop unroll(disable)
  for (int it = 0; it < kSampleIters; ++it) {
    const uint64_t wave_first = block_first + (uint64_t)it * kThreads + (uint64_t)wave * 64;
    if (block_first + (uint64_t)it * kThreads >= n_samples) break;   // (uniform over the workgroup: the barriers below stay matched)
    const uint64_t i = wave_first + (uint64_t)lane;
    const bool live = i < n_samples;
    const uint32_t n_valid = wave_first >= n_samples ? 0u : (uint32_t)min((uint64_t)64, n_samples - wave_first);
    uint32_t t = 0;
    float u = 0.0f, v = 0.0f;
    f3 p = mk3(0.0f, 0.0f, 0.0f), nrm = p;
    if (live) {
      const Philox4 r = sample_random(seed, first + i);
      const uint64_t T = sample_target(r.r[0], r.r[1], W);
      if (LINEAR) {
        while (t + 1u < src.n_tris && !(C[t] > T)) ++t;
      } else {
        const uint64_t j = sample_upper_bound(s_top, 0, n_top, T);   // T < W = top[n_top - 1]: j < n_top
        const uint64_t lo = j << shift, hi = min((j + 1) << shift, (uint64_t)src.n_tris);
        // (C[hi - 1] = top[j] > T, so the search ends inside the chunk; the min only keeps a lane in bounds whatever the table holds)
        t = (uint32_t)min(shift ? sample_upper_bound(C, lo, hi, T) : j, (uint64_t)src.n_tris - 1);
      }
      sample_fold(r.r[2], r.r[3], &u, &v);
      f3 a, b, c, n;
      (void)load_triangle(src, t, &a, &b, &c);   // (indices were checked by k_tri_area before this launch)
      p = sample_point(a, b, c, u, v);
      if (out.normal) {
        const float A = tri_weight_area(a, b, c, &n);
        nrm = sample_normal(n, A);
      }
    }
    if (out.tri && live) out.tri[i] = t;
    if (out.point) {
      const float q[3] = {p.x, p.y, p.z};
      wave_store<3>(out.point + 3 * wave_first, q, s_stage[wave], lane, n_valid);
    }
    if (out.normal) {
      const float q[3] = {nrm.x, nrm.y, nrm.z};
      wave_store<3>(out.normal + 3 * wave_first, q, s_stage[wave], lane, n_valid);
    }
    if (out.uv) {
      const float q[2] = {u, v};
      wave_store<2>(out.uv + 2 * wave_first, q, s_stage[wave], lane, n_valid);
    }
  }
}

}  // namespace

void warm_sample(hipStream_t st) { hipLaunchKernelGGL(k_warm_sample, dim3(1), dim3(64), 0, st); }

uint32_t sample_top_shift(size_t n_tris) {
  uint32_t shift = 0;
  while (((n_tris + ((size_t)1 << shift) - 1) >> shift) > SAMPLE_TOP) ++shift;
  return shift;
}

size_t sample_table_bytes(size_t n_tris) { return (n_tris * 8 + 255) / 256 * 256 + SAMPLE_TOP * 8 + 256; }
size_t sample_scratch_bytes(size_t n_tris) {
  const size_t tiles = tiles_of(n_tris);
  return (n_tris * 4 + 255) / 256 * 256 + (tiles * 8 + 255) / 256 * 256 + 512;
}

int sample_table_carve(Arena& table, Arena& scratch, size_t n_tris, SampleTable* tb) {
  const size_t tiles = tiles_of(n_tris);
  tb->C = table.take<uint64_t>(n_tris);
  tb->top = table.take<uint64_t>(SAMPLE_TOP);
  tb->hdr = table.take<uint32_t>(4);
  tb->A = scratch.take<float>(n_tris);
  tb->tile_sum = scratch.take<uint64_t>(tiles);
  return (tb->C && tb->top && tb->hdr && tb->A && tb->tile_sum) ? 0 : -1;
}

int launch_sample_table(hipStream_t st, const SampleSrc& src, const SampleTable& tb, int* d_err) {
  const uint32_t n = src.n_tris, tiles = tiles_of(n), shift = sample_top_shift(n);
  const uint32_t n_top = (uint32_t)(((size_t)n + ((size_t)1 << shift) - 1) >> shift);
  M2S_HIP_CHECK(hipMemsetAsync(tb.hdr, 0, 16, st));
  hipLaunchKernelGGL(k_tri_area, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, st, src, tb.A, tb.hdr, d_err);
  hipLaunchKernelGGL(k_weight_sums, dim3(tiles), dim3(kThreads), 0, st, tb.A, n, tb.hdr, tb.tile_sum);
  hipLaunchKernelGGL(k_weight_scan_tiles, dim3(1), dim3(kThreads), 0, st, tb.tile_sum, tiles, tb.hdr);
  hipLaunchKernelGGL(k_weight_scan, dim3(tiles), dim3(kThreads), 0, st, tb.A, n, tb.hdr, tb.tile_sum, tb.C);
  hipLaunchKernelGGL(k_table_top, dim3((n_top + kThreads - 1) / kThreads), dim3(kThreads), 0, st, tb.C, n, shift, n_top, tb.hdr, tb.top);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_sample_surface(hipStream_t st, const SampleSrc& src, const SampleTable& tb, uint64_t W, uint64_t seed, uint64_t first, size_t n_samples,
                          int algorithm, const SampleOut& out) {
  if (n_samples == 0 || (!out.point && !out.tri && !out.uv && !out.normal)) return 0;
  const uint32_t shift = sample_top_shift(src.n_tris);
  const uint32_t n_top = (uint32_t)(((size_t)src.n_tris + ((size_t)1 << shift) - 1) >> shift);
  const uint32_t blocks = (uint32_t)((n_samples + (size_t)kThreads * kSampleIters - 1) / ((size_t)kThreads * kSampleIters));
  if (algorithm == 1)
    hipLaunchKernelGGL((k_sample<true>), dim3(blocks), dim3(kThreads), 0, st, src, tb.C, tb.top, shift, n_top, W, seed, first, (uint64_t)n_samples, out);
  else
    hipLaunchKernelGGL((k_sample<false>), dim3(blocks), dim3(kThreads), 0, st, src, tb.C, tb.top, shift, n_top, W, seed, first, (uint64_t)n_samples, out);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace m2s
