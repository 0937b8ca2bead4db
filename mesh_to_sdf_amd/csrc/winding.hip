// winding.hip — generalized winding numbers per point (m2s_winding_numbers, m2s_grid_winding_numbers), gfx950.  DESIGN.md §4.9.
//
// w(p) = (1 / 4 pi) sum_t Omega_t(p), the signed solid angle of every triangle seen from p: 1 inside and 0 outside a closed, outward-wound
// mesh, degrading smoothly across holes; w >= 1/2 is the robust inside test.  Every point must account for every triangle, so the walk is
// a Barnes-Hut one (Barill et al. 2018): a subtree far enough from the point is replaced by the first-order expansion of its area vectors
// about their centroid (NodeMom, k_moments), a subtree of at most WIND_LEAF triangles is summed exactly from `corners`.
//
// One wave = 64 coherent points (a packet brick of the grid, or 64 consecutive queries of the Morton order), walking the stackless
// pre-order tree together: NodeMom and the node's `skip` arrive through scalar loads.  A lane that accepts a node adds its expansion and is
// muted until the walk's slot reaches that node's skip, so the other lanes may descend the same subtree; the wave skips a subtree when no
// lane needs it.  A lane's terms and their order depend only on its own point, the tree and beta — not on its wave-mates.
#include "common.h"
#include "geo.hip.h"
#include "walk.hip.h"

namespace m2s {

namespace {

// Subtrees of at most this many triangles are summed exactly (DESIGN.md §4.9 says why 8).
constexpr uint32_t WIND_LEAF = 8;
constexpr float INV_2PI = 0.15915494309189535f, INV_4PI = 0.07957747154594768f;

// ---- moments ---------------------------------------------------------------------------------------------------------------------
// Every subtree is a contiguous triangle range [slot_first[s], + (skip - s + 1) / 2), so a node is reduced directly from `corners`:
// O(T log T) triangle reads in all.  Sums are taken in f64 (a root of 1 M triangles is good to the f32 rounding of the result).
struct TriGeo {
  double ax, ay, az;   // area vector
  double cx, cy, cz;   // centroid
  double area;
  float v[9];
};
__device__ __forceinline__ TriGeo tri_geo(const float4* __restrict__ corners, uint32_t t) {
  const float4 q0 = corners[3 * (size_t)t], q1 = corners[3 * (size_t)t + 1], q2 = corners[3 * (size_t)t + 2];
  TriGeo g;
  g.v[0] = q0.x; g.v[1] = q0.y; g.v[2] = q0.z; g.v[3] = q0.w; g.v[4] = q1.x; g.v[5] = q1.y; g.v[6] = q1.z; g.v[7] = q1.w; g.v[8] = q2.x;
  const double ux = (double)q0.w - q0.x, uy = (double)q1.x - q0.y, uz = (double)q1.y - q0.z;
  const double vx = (double)q1.z - q0.x, vy = (double)q1.w - q0.y, vz = (double)q2.x - q0.z;
  g.ax = 0.5 * (uy * vz - uz * vy); g.ay = 0.5 * (uz * vx - ux * vz); g.az = 0.5 * (ux * vy - uy * vx);
  g.area = sqrt(g.ax * g.ax + g.ay * g.ay + g.az * g.az);
  g.cx = ((double)q0.x + q0.w + q1.z) / 3.0; g.cy = ((double)q0.y + q1.x + q1.w) / 3.0; g.cz = ((double)q0.z + q1.y + q2.x) / 3.0;
  return g;
}
struct MomSums {   // first pass: what fixes the centre; second pass: the moments about it
  double area = 0.0, wc[3] = {0.0, 0.0, 0.0}, c[3] = {0.0, 0.0, 0.0}, a[3] = {0.0, 0.0, 0.0};
  double m[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  float r2 = 0.0f;
};
__device__ __forceinline__ double wave_sum_d(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
template <uint32_t STRIDE>
__device__ __forceinline__ void mom_pass1(const float4* __restrict__ corners, uint32_t first, uint32_t cnt, uint32_t lane, MomSums& s) {
#pragma unroll 4
  for (uint32_t i = lane; i < cnt; i += STRIDE) {
    const TriGeo g = tri_geo(corners, first + i);
    s.area += g.area;
    s.wc[0] += g.area * g.cx; s.wc[1] += g.area * g.cy; s.wc[2] += g.area * g.cz;
    s.c[0] += g.cx; s.c[1] += g.cy; s.c[2] += g.cz;
    s.a[0] += g.ax; s.a[1] += g.ay; s.a[2] += g.az;
  }
}
template <uint32_t STRIDE>
__device__ __forceinline__ void mom_pass2(const float4* __restrict__ corners, uint32_t first, uint32_t cnt, uint32_t lane, float cx, float cy,
                                          float cz, MomSums& s) {
#pragma unroll 4
  for (uint32_t i = lane; i < cnt; i += STRIDE) {
    const TriGeo g = tri_geo(corners, first + i);
    const double dx = g.cx - cx, dy = g.cy - cy, dz = g.cz - cz;
    s.m[0] += g.ax * dx; s.m[1] += g.ax * dy; s.m[2] += g.ax * dz;
    s.m[3] += g.ay * dx; s.m[4] += g.ay * dy; s.m[5] += g.ay * dz;
    s.m[6] += g.az * dx; s.m[7] += g.az * dy; s.m[8] += g.az * dz;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float ex = g.v[3 * k] - cx, ey = g.v[3 * k + 1] - cy, ez = g.v[3 * k + 2] - cz;
      s.r2 = fmaxf(s.r2, ex * ex + ey * ey + ez * ez);
    }
  }
}
// The centre as it is stored (f32): the second pass and the walk both measure from these very bits.
__device__ __forceinline__ void mom_centre(const MomSums& s, uint32_t cnt, float* cx, float* cy, float* cz) {
  const bool weighted = s.area > 0.0 && s.area < 1.0e300;
  const double d = weighted ? s.area : (double)cnt;
  *cx = (float)((weighted ? s.wc[0] : s.c[0]) / d);
  *cy = (float)((weighted ? s.wc[1] : s.c[1]) / d);
  *cz = (float)((weighted ? s.wc[2] : s.c[2]) / d);
}
__device__ __forceinline__ void mom_store(NodeMom* __restrict__ moms, uint32_t slot, float cx, float cy, float cz, const MomSums& s) {
  NodeMom m;
  m.cx = cx; m.cy = cy; m.cz = cz;
  // outward rounding of the radius: the squared distances above carry a few ulps each; the floor keeps (beta r)^2 a normal number
  m.r = sqrtf(s.r2) * 1.00001f + 1.0e-18f;
  m.ax = (float)s.a[0]; m.ay = (float)s.a[1]; m.az = (float)s.a[2];
#pragma unroll
  for (int k = 0; k < 9; ++k) m.m[k] = (float)s.m[k];
  moms[slot] = m;
}

constexpr uint32_t MOM_THREAD_BELOW = 16;   // a lane per node up to this many triangles, a wave per node above (as k_node_ext splits)

__global__ __launch_bounds__(256) void k_moments(const NodeRec* __restrict__ nodes, const uint32_t* __restrict__ slot_first,
                                                 const float4* __restrict__ corners, uint32_t n_nodes, NodeMom* __restrict__ moms) {
  __shared__ uint32_t big_slot[256], big_first[256], big_cnt[256];
  __shared__ uint32_t n_big;
  if (threadIdx.x == 0) n_big = 0;
  __syncthreads();
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot < n_nodes) {
    const uint32_t cnt = (nodes[slot].skip - slot + 1u) >> 1, first = slot_first[slot];
    if (cnt <= MOM_THREAD_BELOW) {
      MomSums s;
      float cx, cy, cz;
      mom_pass1<1>(corners, first, cnt, 0u, s);
      mom_centre(s, cnt, &cx, &cy, &cz);
      mom_pass2<1>(corners, first, cnt, 0u, cx, cy, cz, s);
      mom_store(moms, slot, cx, cy, cz, s);
    } else {
      const uint32_t at = atomicAdd(&n_big, 1u);
      big_slot[at] = slot;
      big_first[at] = first;
      big_cnt[at] = cnt;
    }
  }
  __syncthreads();
  const uint32_t nb = n_big, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  for (uint32_t k = wave; k < nb; k += 4u) {
    const uint32_t first = big_first[k], cnt = big_cnt[k];
    MomSums s;
    float cx, cy, cz;
    mom_pass1<64>(corners, first, cnt, lane, s);
    s.area = wave_sum_d(s.area);
#pragma unroll
    for (int j = 0; j < 3; ++j) { s.wc[j] = wave_sum_d(s.wc[j]); s.c[j] = wave_sum_d(s.c[j]); s.a[j] = wave_sum_d(s.a[j]); }
    mom_centre(s, cnt, &cx, &cy, &cz);   // every lane holds the same sums
    mom_pass2<64>(corners, first, cnt, lane, cx, cy, cz, s);
#pragma unroll
    for (int j = 0; j < 9; ++j) s.m[j] = wave_sum_d(s.m[j]);
    for (int o = 32; o > 0; o >>= 1) s.r2 = fmaxf(s.r2, __shfl_xor(s.r2, o));
    if (lane == 0) mom_store(moms, big_slot[k], cx, cy, cz, s);
  }
}

// ---- the walk ----------------------------------------------------------------------------------------------------------------------
// Wave-uniform dword of a read-only array through the constant address space (walk.hip.h record_at_bytes says why).
__device__ __forceinline__ uint32_t word_at(const uint32_t* base, uint32_t index) {
  typedef const __attribute__((address_space(4))) uint32_t* const_words;
  return ((const_words)(uintptr_t)base)[index];
}
struct alignas(16) NodeHead { float mnx, mny, mnz; uint32_t skip; };   // the first half of a NodeRec: `tri` (re-marked per call) is not read
struct alignas(16) TriCorners { float ax, ay, az, bx, by, bz, cx, cy, cz, p0, p1, p2; };   // one 48-byte `corners` record
static_assert(sizeof(NodeHead) == 16 && sizeof(TriCorners) == 48, "record sizes");

// Solid angle of one triangle over 4 pi (Van Oosterom-Strackee): atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) / 2 pi with
// a, b, c relative to p.  The numerator is taken as a.n with n = (b - a) x (c - a), the raw normal — the same determinant, formed from the
// short edge vectors, so that it does not cancel for a far point.  n == 0 or a.n == 0 (p in the triangle's plane): no contribution.
__device__ __forceinline__ float tri_winding(f3 p, const TriCorners& t) {
  const float ux = t.bx - t.ax, uy = t.by - t.ay, uz = t.bz - t.az, vx = t.cx - t.ax, vy = t.cy - t.ay, vz = t.cz - t.az;
  const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  const bool flat = nx == 0.0f && ny == 0.0f && nz == 0.0f;
  const float ax = t.ax - p.x, ay = t.ay - p.y, az = t.az - p.z;
  const float bx = t.bx - p.x, by = t.by - p.y, bz = t.bz - p.z;
  const float cx = t.cx - p.x, cy = t.cy - p.y, cz = t.cz - p.z;
  const float num = ax * nx + ay * ny + az * nz;
  const float la = sqrtf(ax * ax + ay * ay + az * az), lb = sqrtf(bx * bx + by * by + bz * bz), lc = sqrtf(cx * cx + cy * cy + cz * cz);
  const float den = la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (bx * cx + by * cy + bz * cz) * la + (cx * ax + cy * ay + cz * az) * lb;
  const float w = atan2f(num, den) * INV_2PI;
  return (flat || num == 0.0f) ? 0.0f : w;   // a NaN point: num is NaN, the term is NaN
}

// Exact sum over the triangles [first, first + cnt) for the lanes in `on`, four records fetched per wait.
__device__ __forceinline__ void winding_exact(const DeviceMesh& mesh, f3 p, bool on, uint32_t first, uint32_t cnt, float& w) {
  const TriCorners* recs = reinterpret_cast<const TriCorners*>(mesh.corners);
  for (uint32_t k0 = 0; k0 < cnt; k0 += 4u) {
    TriCorners t[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) t[u] = record_at<TriCorners>(recs, first + min(k0 + u, cnt - 1u));
    // A use of both halves of every record right here: without it the compiler sinks each record's two loads into the branch that
    // evaluates it and the group pays four memory round trips, one after the other, instead of one.
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) asm volatile("" ::"s"(t[u].ax), "s"(t[u].cz));
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) {
      if (k0 + u >= cnt) break;   // wave-uniform
      const float term = tri_winding(p, t[u]);
      if (on) w += term;
    }
  }
}

// First-order expansion of a node seen from p: sum a . K(x) + <M, grad K(x)>, x = centre - p, K(x) = x / (4 pi |x|^3),
// grad K = (I / |x|^3 - 3 x x^T / |x|^5) / 4 pi, hence <M, grad K> = (tr M - 3 x^T M x / |x|^2) / (4 pi |x|^3).
__device__ __forceinline__ float node_expansion(const NodeMom& m, float x, float y, float z, float d2) {
  const float inv = __builtin_amdgcn_rsqf(d2), inv2 = inv * inv, k = inv * inv2 * INV_4PI;
  const float dip = m.ax * x + m.ay * y + m.az * z;
  const float tr = m.m[0] + m.m[4] + m.m[8];
  const float mx = m.m[0] * x + m.m[1] * y + m.m[2] * z, my = m.m[3] * x + m.m[4] * y + m.m[5] * z, mz = m.m[6] * x + m.m[7] * y + m.m[8] * z;
  const float quad = x * mx + y * my + z * mz;
  return (dip + (tr - 3.0f * quad * inv2)) * k;
}

template <bool ALL_PAIRS>
__device__ __forceinline__ float winding_of(const DeviceMesh& mesh, const NodeMom* moms, f3 p, bool valid, float beta) {
  float w = 0.0f;
  if (ALL_PAIRS) {
    winding_exact(mesh, p, valid, 0u, mesh.n_tris, w);
    return w;
  }
  const uint32_t end = mesh.n_nodes;
  uint32_t s = 0, muted_until = 0;   // a lane that accepted a node sits out until the walk leaves that node's subtree
  while (s < end) {
    const NodeMom m = record_at<NodeMom>(moms, s);
    const uint32_t skip = record_at<NodeHead>(reinterpret_cast<const NodeHead*>(mesh.nodes), 2u * s).skip;   // NodeRec = two NodeHead-sized halves
    const bool active = valid && s >= muted_until;
    const float x = m.cx - p.x, y = m.cy - p.y, z = m.cz - p.z, d2 = x * x + y * y + z * z, br = beta * m.r;
    const bool accept = active && d2 > br * br;   // beta = +inf, or a NaN point: never
    if (accept) { w += node_expansion(m, x, y, z, d2); muted_until = skip; }
    const bool need = active && !accept;
    if (__ballot(need) == 0ull) { s = skip; continue; }
    const uint32_t cnt = (skip - s + 1u) >> 1;
    if (cnt > WIND_LEAF) { s += 1u; continue; }
    winding_exact(mesh, p, need, word_at(mesh.slot_first, s), cnt, w);
    s = skip;
  }
  return w;
}

__device__ __forceinline__ void winding_store(const WindingOut& out, size_t i, float w, float d, float threshold) {
  if (out.w) out.w[i] = w;
  if (out.sdf) out.sdf[i] = w >= threshold ? -d : d;   // a NaN w: +d
}

template <bool ALL_PAIRS>
__global__ __launch_bounds__(64) void k_winding_grid(DeviceMesh mesh, const NodeMom* __restrict__ moms, GridParams g, float beta, float threshold,
                                                     const float* __restrict__ dist_in, uint64_t dist_off, WindingOut out) {
  const GridBrick vox = grid_lane_voxel(g, blockIdx.x, (int)threadIdx.x);
  if (!vox.brick_in_grid) return;   // padding of the last super-bricks: wave-uniform
  const f3 p = grid_point(g, vox);
  const size_t cell = ((size_t)vox.x * g.n[1] + vox.y) * g.n[2] + vox.z;
  const bool valid = vox.in_range;
  const float w = winding_of<ALL_PAIRS>(mesh, moms, p, valid, beta);
  if (valid) winding_store(out, cell - out.off, w, out.sdf ? dist_in[cell - dist_off] : 0.0f, threshold);
}

template <bool ALL_PAIRS>
__global__ __launch_bounds__(64) void k_winding_q(DeviceMesh mesh, const NodeMom* __restrict__ moms, const float* __restrict__ queries,
                                                  const uint32_t* __restrict__ perm, uint32_t n_q, float beta, float threshold,
                                                  const float* __restrict__ dist_in, WindingOut out) {
  const uint32_t j = blockIdx.x * 64u + threadIdx.x;
  const bool valid = j < n_q;
  const uint32_t i = valid ? (perm ? perm[j] : j) : 0u;
  const f3 p = valid ? mk3(queries[3 * (size_t)i], queries[3 * (size_t)i + 1], queries[3 * (size_t)i + 2]) : mk3(0.0f, 0.0f, 0.0f);
  const float w = winding_of<ALL_PAIRS>(mesh, moms, p, valid, beta);
  if (valid) winding_store(out, i, w, out.sdf ? dist_in[i] : 0.0f, threshold);
}

}  // namespace

int launch_winding_moments(hipStream_t st, const DeviceMesh& mesh, NodeMom* moms) {
  if (mesh.n_nodes == 0) return 0;
  hipLaunchKernelGGL(k_moments, dim3((mesh.n_nodes + 255u) / 256u), dim3(256), 0, st, mesh.nodes, mesh.slot_first, mesh.corners, mesh.n_nodes, moms);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_winding_grid(hipStream_t st, const DeviceMesh& mesh, const NodeMom* moms, const GridParams& g, float beta, float threshold,
                        const float* d_dist, uint64_t dist_off, int algorithm, const WindingOut& out) {
  const uint32_t packets = host_packet_bricks(g);
  if (packets == 0) return 0;
  M2S_REQUIRE_GRID_CONSTS(g);
  if (algorithm == 1) hipLaunchKernelGGL(k_winding_grid<true>, dim3(packets), dim3(64), 0, st, mesh, moms, g, beta, threshold, d_dist, dist_off, out);
  else hipLaunchKernelGGL(k_winding_grid<false>, dim3(packets), dim3(64), 0, st, mesh, moms, g, beta, threshold, d_dist, dist_off, out);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_winding_queries(hipStream_t st, const DeviceMesh& mesh, const NodeMom* moms, const float* d_queries, const uint32_t* perm, size_t n_q,
                           float beta, float threshold, const float* d_dist, int algorithm, const WindingOut& out) {
  if (n_q == 0) return 0;
  const uint32_t nq = (uint32_t)n_q, packets = (nq + 63u) / 64u;
  if (algorithm == 1) hipLaunchKernelGGL(k_winding_q<true>, dim3(packets), dim3(64), 0, st, mesh, moms, d_queries, perm, nq, beta, threshold, d_dist, out);
  else hipLaunchKernelGGL(k_winding_q<false>, dim3(packets), dim3(64), 0, st, mesh, moms, d_queries, perm, nq, beta, threshold, d_dist, out);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace m2s
