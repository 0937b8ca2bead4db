// query_order.hip — generic queries before the walk (gfx950): bounding box, Morton keys, sort, the packet table, the packets' centres
// and the gather into sorted order (prepare_query_walk).  Needs the queries only, so a one-shot call runs it beside the build.
#include "common.h"
#include "tuning.h"
#include "dist.hip.h"

namespace m2s {

namespace {

// ---- query ordering (generic path): Morton sort so that a packet is spatially compact ---------
__device__ __forceinline__ int ordf(float f) {
  int i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float unordf(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

// Bounding box of the queries (order-encoded ints): grid-stride partials per block, folded by a second
// one-block launch — no atomics on six hot addresses.
constexpr unsigned QB_BLOCKS = 1024;
__device__ __forceinline__ void qb_block_reduce(int lo[3], int hi[3], int* __restrict__ dst) {
  __shared__ int part[6][4];
  const int wv = threadIdx.x >> 6;
  for (int k = 0; k < 3; ++k) {
    int l = lo[k], h = hi[k];
    for (int off = 32; off > 0; off >>= 1) { l = min(l, __shfl_xor(l, off)); h = max(h, __shfl_xor(h, off)); }
    if ((threadIdx.x & 63) == 0) { part[k][wv] = l; part[3 + k][wv] = h; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    int v = part[k][0];
    for (int w = 1; w < 4; ++w) v = k < 3 ? min(v, part[k][w]) : max(v, part[k][w]);
    dst[k] = v;
  }
}
__global__ __launch_bounds__(256) void k_qbounds(const float* __restrict__ q, uint32_t n_q, int* __restrict__ partial) {
  int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_q; i += (size_t)gridDim.x * blockDim.x)
    for (int k = 0; k < 3; ++k) {
      const float v = q[3 * i + k];
      if (v == v && fabsf(v) < 3.0e38f) { const int o = ordf(v); lo[k] = min(lo[k], o); hi[k] = max(hi[k], o); }
    }
  qb_block_reduce(lo, hi, partial + 6 * blockIdx.x);
}
__global__ __launch_bounds__(256) void k_qbounds_final(const int* __restrict__ partial, uint32_t n_blocks, int* __restrict__ b) {
  int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  for (uint32_t j = threadIdx.x; j < n_blocks; j += 256)
    for (int k = 0; k < 3; ++k) { lo[k] = min(lo[k], partial[6 * j + k]); hi[k] = max(hi[k], partial[6 * j + 3 + k]); }
  qb_block_reduce(lo, hi, b);
}
// 30-bit Morton key of a query in the query bounding box (10 bits per axis: 1024^3 cells — far finer than a packet of 64 of
// any realistic query count, and a 32-bit key sorts in four radix passes instead of the eight of the 63-bit key used before:
// 0.83 -> 0.45 ms for 10 M queries).  Queries of one cell keep their input order among themselves.
constexpr int QKEY_BITS = 30;
__device__ __forceinline__ uint32_t expand10q(uint32_t v) {
  uint32_t x = v & 0x3ffu;
  x = (x | x << 16) & 0x030000ffu;
  x = (x | x << 8) & 0x0300f00fu;
  x = (x | x << 4) & 0x030c30c3u;
  x = (x | x << 2) & 0x09249249u;
  return x;
}
// `drop`: low key bits cleared.  The sort then runs over the bits [drop, 30) only — 10 M queries need 21 bits (2 M cells) to form their
// packets, three radix passes instead of four; queries of one finest cell stay in input order, which k_qcells treats like identical keys.
__global__ __launch_bounds__(256) void k_qkeys(const float* __restrict__ q, uint32_t n_q, const int* __restrict__ b,
                                               uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t drop) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_q) return;
  uint32_t c[3];
  for (int k = 0; k < 3; ++k) {
    const float lo = unordf(b[k]), hi = unordf(b[3 + k]);
    float u = (q[3 * (size_t)i + k] - lo) / (hi - lo);
    u = (u == u) ? fminf(fmaxf(u, 0.0f), 1.0f) : 0.0f;
    c[k] = min((uint32_t)(u * 1024.0f), 1023u);
  }
  keys[i] = (((expand10q(c[0]) << 2) | (expand10q(c[1]) << 1) | expand10q(c[2])) >> drop) << drop;
  vals[i] = i;
}
// Seed lattice for generic queries: QL^3 cells over the query bounding box (description kept on the device).
__global__ void k_qlattice(const int* __restrict__ b, GridParams* __restrict__ L) {
  if (threadIdx.x != 0) return;
  GridParams g{};
  for (int k = 0; k < 3; ++k) {
    const float lo = unordf(b[k]), hi = unordf(b[3 + k]);
    float cs = (hi - lo) / (float)QL;
    if (!(cs > 0.0f) || !(cs < 3.0e38f)) cs = 1.0f;
    g.n[k] = QL;
    g.size[k] = cs;
    g.first[k] = ((lo == lo && fabsf(lo) < 3.0e38f) ? lo : 0.0f) + 0.5f * cs;
  }
  g.xb = 0; g.xe = QL; g.nzw = 0; g.out_off = 0; g.chunk_log = 31; g.period = 0;
  *L = g;
}

__global__ __launch_bounds__(256) void k_qgather(const float* __restrict__ q, const uint32_t* __restrict__ perm,
                                                 uint32_t n_q, float4* __restrict__ sorted) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_q) return;
  const size_t s = perm[i];
  sorted[i] = make_float4(q[3 * s], q[3 * s + 1], q[3 * s + 2], 0.0f);
}

// Packets of the generic path.  64 CONSECUTIVE queries of the Morton order are a loose group (the run straddles cell
// boundaries of every level: bounding radius 1.6 x that of a cube holding 64 uniform points, r^2 2.9 x) and the wave-uniform
// walk pays for the union of what its 64 lanes need.  The packets are therefore the LEAVES OF THE BUCKET K-D TREE over the
// keys, capacity 64: the largest key-prefix cells holding at most 64 queries — aligned boxes of aspect <= 2, 46 queries on
// average for uniform points (1.38 x the packets, radius 0.88, r^2 0.78 of that cube's).  No tree is built: with
// w[j] = common prefix length of keys j and j + 64, query i sits in an over-full cell of prefix length b iff some window
// j in [i - 64, i] has w[j] >= b, so its leaf has prefix length m(i) + 1, m(i) = max of w over those windows, the same for
// every query of the leaf; i starts a packet iff it differs from i - 1 within that prefix.  More than 64 queries with
// identical keys (m = QKEY_BITS) are cut at multiples of 64.
__global__ __launch_bounds__(256) void k_qcells(const uint32_t* __restrict__ keys, uint32_t n, uint8_t* __restrict__ head) {
  __shared__ uint32_t sk[256 + 128];   // keys[base - 64, base + 320)
  __shared__ int sw[256 + 64];         // w[j], j in [base - 64, base + 256)
  const long long base = (long long)blockIdx.x * 256;
  for (uint32_t t = threadIdx.x; t < 384u; t += 256u) {
    const long long idx = base - 64 + t;
    sk[t] = (idx >= 0 && idx < (long long)n) ? keys[idx] : 0u;
  }
  __syncthreads();
  for (uint32_t t = threadIdx.x; t < 320u; t += 256u) {
    const long long j = base - 64 + t;
    const uint32_t x = sk[t] ^ sk[t + 64];
    sw[t] = (j >= 0 && j + 64 < (long long)n) ? (x == 0u ? QKEY_BITS : __clz((int)x) - (32 - QKEY_BITS)) : -1;
  }
  __syncthreads();
  const long long i = base + threadIdx.x;
  if (i >= (long long)n) return;
  int m = -1;
  for (uint32_t t = 0; t <= 64u; ++t) m = max(m, sw[threadIdx.x + t]);
  const uint32_t plen = (uint32_t)min(m + 1, QKEY_BITS);
  const uint32_t key = sk[threadIdx.x + 64], prev = sk[threadIdx.x + 63];
  bool h = i == 0 || (plen != 0u && ((key ^ prev) >> ((uint32_t)QKEY_BITS - plen)) != 0u);
  if (m >= QKEY_BITS) h |= (i & 63) == 0;                   // more than 64 queries in one cell of the finest level
  head[i] = h ? 1 : 0;
}
__global__ void k_qtable_mode(uint32_t* __restrict__ table, uint32_t n, uint32_t launched) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const bool over = table[0] > launched;                    // cannot be ruled out (63 levels of 1 + 64 splits): consecutive packets then
  table[1] = over ? 1u : 0u;
  if (over) table[0] = (n + 63u) / 64u;
}

// (centre, radius) of the bounding box of every packet's queries: one wave per packet.  The radius is rounded up; a packet
// with a non-finite coordinate gets radius inf (its cut list then keeps the whole tree).
// `raw` != nullptr: the kernel also brings the packet's queries into sorted order (sorted[i] = raw[perm[i]]; the packets partition the
// sorted range, so every query is written once) — the gather that k_qgather does in a pass of its own otherwise.
__global__ __launch_bounds__(256) void k_qpacket_bounds(float4* __restrict__ sorted, const uint32_t* __restrict__ table,
                                                        uint32_t n_q, uint32_t launched, float4* __restrict__ centres,
                                                        const float* __restrict__ raw, const uint32_t* __restrict__ perm) {
  const uint32_t packet = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (packet >= launched) return;
  uint32_t first, cnt;
  if (!query_packet_range(table, packet, n_q, &first, &cnt)) return;
  float4 v;
  if (raw != nullptr) {
    const size_t s = perm[first + min(lane, cnt - 1u)];
    v = make_float4(raw[3 * s], raw[3 * s + 1], raw[3 * s + 2], 0.0f);
    if (lane < cnt) sorted[first + lane] = v;
  } else {
    v = sorted[first + min(lane, cnt - 1u)];
  }
  float lo[3] = {v.x, v.y, v.z}, hi[3] = {v.x, v.y, v.z};
  bool bad = !(fabsf(v.x) < 3.0e37f) | !(fabsf(v.y) < 3.0e37f) | !(fabsf(v.z) < 3.0e37f);
  for (int o = 32; o >= 1; o >>= 1)
    for (int k = 0; k < 3; ++k) {
      lo[k] = fminf(lo[k], __shfl_xor(lo[k], o));
      hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o));
    }
  bad = __ballot(bad) != 0ull;
  if (lane != 0u) return;
  float c[3], r2 = 0.0f;
  for (int k = 0; k < 3; ++k) {
    c[k] = 0.5f * lo[k] + 0.5f * hi[k];
    const float h = fmaxf(hi[k] - c[k], c[k] - lo[k]);
    r2 = __builtin_fmaf(h, h, r2);
  }
  float r = sqrtf(r2) * 1.0001f + 1.0e-30f;
  if (bad) { c[0] = c[1] = c[2] = 0.0f; r = __builtin_inff(); }
  centres[packet] = make_float4(c[0], c[1], c[2], r);
}

}  // namespace

size_t query_workspace_bytes(size_t n_q) {
  size_t n = n_q ? n_q : 1, tmp = 0;
  (void)sort_pairs_u32(nullptr, tmp, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                            n, 0, 30, (hipStream_t)0);
  size_t sel = 0;
  (void)select_flagged_indices(nullptr, sel, (const uint8_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, (hipStream_t)0);
  return n * (8 + 8 + 4 + 4 + 16 + 1 + 4) + n * 16 + 256 + (n / 32 + 64) * (16 + 4 * CUT_WORDS) + tmp + sel + 21 * 256 + (size_t)64 * 64 * 64 * 44 + 8192 + 24 * 1024 + 256;
}

// Generic queries in two parts.  prepare_query_walk needs the queries only — bounding box, Morton keys, sort, packet table, the
// packets' centres and the gather into sorted order — so a one-shot call runs it on a side stream BESIDE the LBVH build (capi.hip:
// 0.8 ms of bandwidth-bound passes next to 0.24 ms of latency-bound launches for 10 M queries x 100 k triangles); launch_query_walk
// needs the tree: seed lattice, cut lists, walk.  launch_query_distance is both on one stream (persistent meshes, asynchronous calls).
int prepare_query_walk(Arena& ws, hipStream_t st, const float* d_queries, size_t n_q, size_t n_tris, int sign_src, int algorithm, QueryPlan* plan,
                       hipEvent_t after_lattice) {
  *plan = QueryPlan{};
  plan->n_q = n_q;
  if (n_q == 0 || algorithm == 1) return 0;
  const uint32_t nq = (uint32_t)n_q;
  const uint32_t packets = (nq + 63) / 64;
  // Morton order
  int* qb = ws.take<int>(8 + 6 * QB_BLOCKS);
  uint32_t* keys = ws.take<uint32_t>(n_q);
  uint32_t* keys2 = ws.take<uint32_t>(n_q);
  uint32_t* vals = ws.take<uint32_t>(n_q);
  uint32_t* perm = ws.take<uint32_t>(n_q);
  float4* sorted = ws.take<float4>(n_q);
  size_t tmp_bytes = 0;
  (void)sort_pairs_u32(nullptr, tmp_bytes, keys, keys2, vals, perm, n_q, 0, QKEY_BITS, st);
  void* tmp = ws.take<char>(tmp_bytes ? tmp_bytes : 1);
  if (!qb || !keys || !keys2 || !vals || !perm || !sorted || !tmp) {
    set_error("internal: query workspace too small");
    return M2S_ERR_HIP_INTERNAL;
  }
  // key bits that matter: cells of ~8 queries at the finest level, whole Morton triples, 12 ... 30
  uint32_t bits = 12;
  while (bits < (uint32_t)QKEY_BITS && (1ull << bits) * 8ull < (unsigned long long)n_q) bits += 3;
  const uint32_t drop = (uint32_t)QKEY_BITS - bits;
  const unsigned B = 256, nb = (nq + B - 1) / B;
  const unsigned qblocks = nb < QB_BLOCKS ? nb : QB_BLOCKS;
  hipLaunchKernelGGL(k_qbounds, dim3(qblocks), dim3(B), 0, st, d_queries, nq, qb + 8);
  hipLaunchKernelGGL(k_qbounds_final, dim3(1), dim3(B), 0, st, qb + 8, qblocks, qb);
  const bool seeds = n_tris && packets >= 8;
  if (seeds) {                                   // the seed lattice's description: QL^3 cells over the queries' bounding box
    GridParams* lat = ws.take<GridParams>(1);
    if (!lat) { set_error("internal: query workspace too small"); return M2S_ERR_HIP_INTERNAL; }
    hipLaunchKernelGGL(k_qlattice, dim3(1), dim3(64), 0, st, qb, lat);
    plan->lat = lat;
  }
  if (after_lattice) M2S_HIP_CHECK(hipEventRecord(after_lattice, st));
  hipLaunchKernelGGL(k_qkeys, dim3(nb), dim3(B), 0, st, d_queries, nq, qb, keys, vals, drop);
  M2S_HIP_CHECK(sort_pairs_u32(tmp, tmp_bytes, keys, keys2, vals, perm, n_q, drop, QKEY_BITS, st));
  // Sparse query sets take the lane walk (k_lane_q).  Measured crossover, uniform queries in the extended box (lane / packet walk,
  // RtreeBvh): blob-100k 100 k queries 1.36 / 3.65 ms, 1 M 2.70 / 3.45, 3 M 5.00 / 4.38, 10 M 12.3 / 6.7 (crossover ~2 M);
  // blob-1M 1 M 6.3 / 12.8 ms, 10 M 26.4 / 22.4 (~7 M).  Below it the packet walk lasts as long as its worst packet's chain of
  // dependent loads (2.7 ms), above it the lane walk's divergence costs more than the packets' union.  n* ~ 3500 T^0.55 fits both.
  // (End of round 4, leaf work queued and leaves of 4 - 8 for the packets — query_leaf_max: lane / packets, whole call: blob-100k 100 k queries 1.12 /
  // 1.53 ms, 300 k 1.47 / 1.46, 1 M 2.13 / 1.39, 10 M 10.9 / 3.60; blob-11k 30 k 0.72 / 0.66, 300 k 0.80 / 0.63: the crossover is at ~2.5 queries
  // per triangle now.)
  const bool lane_walk = query_walk_is_lane(n_q, n_tris, sign_src);
  // packets = leaves of the bucket k-d tree over the sorted keys (k_qcells); the launch has room for twice the consecutive
  // count, and k_qtable_mode falls back to consecutive packets should there be more
  const uint32_t* table = nullptr;
  uint32_t launched = packets;
  if (!lane_walk) {
    launched = nq / 32u + 64u;
    if (tuning().query_launch_tight != 0) launched = packets + 1u;   // test hook: forces the consecutive-packet fallback
    uint8_t* head = ws.take<uint8_t>(n_q);
    uint32_t* tb = ws.take<uint32_t>(n_q + 2);               // [0] count, [1] mode, then one start per head (at most n_q)
    size_t sel_bytes = 0;
    (void)select_flagged_indices(nullptr, sel_bytes, head, tb + 2, tb, n_q, st);
    void* sel_tmp = ws.take<char>(sel_bytes ? sel_bytes : 1);
    if (!head || !tb || !sel_tmp) { set_error("internal: query workspace too small"); return M2S_ERR_HIP_INTERNAL; }
    hipLaunchKernelGGL(k_qcells, dim3(nb), dim3(B), 0, st, keys2, nq, head);
    M2S_HIP_CHECK(select_flagged_indices(sel_tmp, sel_bytes, head, tb + 2, tb, n_q, st));
    hipLaunchKernelGGL(k_qtable_mode, dim3(1), dim3(1), 0, st, tb, nq, launched);
    table = tb;
  }
  // cut lists, one per packet (k_cut<false>): they need the packets' centres, and the kernel that finds those gathers the queries too
  const uint32_t qcut_min = tuning().query_cut_min;
  float4* centres = nullptr;
  if (table != nullptr && seeds && packets >= qcut_min) {
    centres = ws.take<float4>(launched);
    if (!centres) { set_error("internal: query workspace too small"); return M2S_ERR_HIP_INTERNAL; }
    hipLaunchKernelGGL(k_qpacket_bounds, dim3((launched + 3) / 4), dim3(256), 0, st, sorted, table, nq, launched, centres, d_queries, (const uint32_t*)perm);
  } else {
    hipLaunchKernelGGL(k_qgather, dim3(nb), dim3(B), 0, st, d_queries, perm, nq, sorted);
  }
  M2S_HIP_CHECK(hipGetLastError());
  plan->qb = qb; plan->perm = perm; plan->sorted = sorted; plan->table = table; plan->centres = centres;
  plan->launched = launched; plan->lane_walk = lane_walk; plan->seeds = seeds;
  return 0;
}

// m2s_warmup: this unit's code object, and the kernel functions of it that a first call uses (see warm_distance).
__global__ void k_warm_query_order() {}
void warm_query_order(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_query_order, dim3(1), dim3(64), 0, st);
  const void* fns[] = {
      (const void*)k_qbounds,
      (const void*)k_qbounds_final,
      (const void*)k_qkeys,
      (const void*)k_qgather,
      (const void*)k_qcells,
      (const void*)k_qtable_mode,
      (const void*)k_qpacket_bounds,
      (const void*)k_qlattice};
  hipFuncAttributes attr;
  for (const void* f : fns) (void)hipFuncGetAttributes(&attr, f);
  (void)hipGetLastError();
}

}  // namespace m2s
