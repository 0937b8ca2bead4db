// closest.hip — nearest triangle and closest point per point (m2s_closest_points, m2s_grid_closest_points), gfx950.
//
// Second of two passes.  The first pass is the unsigned distance walk of distance.hip, unchanged: it leaves the exact
// d = sqrt(min d2) of every point in a buffer.  k_closest then knows how far the nearest triangle is and only has to find WHICH
// triangle attains that minimum — the lexicographic minimum (d2, input triangle index) of eval_triangle<MODE_NEAREST_NORMAL>, the tie
// rule the Rtree sign already uses — and where on it the closest point lies.
//
// One wave = 64 coherent points (a packet brick of the grid walk, or 64 consecutive queries in the Morton order the query walk sorts
// into), walking the stackless pre-order tree of oriented bounds together: node and pre-test records arrive through scalar loads, a
// subtree is entered when any lane's lower bound reaches its threshold.  The threshold of a lane is prune_bound of a d2 that is an upper
// bound of min d2, so it is at least the threshold the distance walk ends with: no triangle that attains the minimum can be pruned
// (the margin analysis of prune_bound, which covers ties).  No seeds, cut lists, groups or splits: the bound is exact from the start.
#include "common.h"
#include "geo.hip.h"
#include "walk.hip.h"

namespace m2s {

namespace {

constexpr uint32_t NO_TRIANGLE = 0xffffffffu;

// Upper bound of min d2 from the exact distance d = RN(sqrt(min d2)) of the first pass: d * d can round below min d2 (by a few ulps:
// the square root and the product each round by half an ulp), so it is raised by 2^-20 relative (8 ulps).  d = f32::MAX (no comparable
// triangle, or an overflowing distance) gives +inf: every node is entered, as it must be.
__device__ __forceinline__ float seed_d2(float d) {
  const float dd = d * d;
  return dd + dd * 0x1.0p-20f;
}

// Every triangle for every valid lane (m2s_opts.algorithm = 1, validation).
__device__ __forceinline__ void closest_all_pairs(const DeviceMesh& mesh, f3 p, bool valid, Best<MODE_NEAREST_NORMAL>& best, uint32_t& slot) {
  for (uint32_t s = 0; s < mesh.n_tris; ++s) {
    const TriRec tr = record_at<TriRec>(mesh.tris, s);
    if (valid) {
      const uint32_t before = best.idx;
      eval_triangle<MODE_NEAREST_NORMAL>(best, p, tr);
      if (best.idx != before) slot = s;
    }
  }
}
// The search of one wave.  `valid` lanes look for the lexicographic minimum (d2, index) below their threshold; `slot` is the record
// (sorted position) of the triangle that won, for the closest point afterwards.
template <bool ALL_PAIRS>
__device__ __forceinline__ void closest_search(const DeviceMesh& mesh, f3 p, float d, bool valid, Best<MODE_NEAREST_NORMAL>& best,
                                               uint32_t& slot) {
  if (ALL_PAIRS) {
    closest_all_pairs(mesh, p, valid, best, slot);
    return;
  }
  const float scale = fmaxf(mesh_scale(mesh), fmaxf(fabsf(p.x), fmaxf(fabsf(p.y), fabsf(p.z))));
  const float thr = prune_bound(seed_d2(d), 4.0e-6f * scale);   // the slack of the distance walks (k_lane, k_lane_q)
  constexpr uint32_t NB = (uint32_t)sizeof(NodeExt);
  const uint32_t end = mesh.n_nodes * NB;
  uint32_t off = 0;
  while (off < end) {
    const NodeExt nr = record_at_bytes<NodeExt>(mesh.ext, off);
    const bool reach = valid && !(ext_dist2(p, nr) > thr);   // a NaN bound (NaN point) is not a reason to prune
    if (__ballot(reach) == 0ull) { off = nr.skip; continue; }
    if (nr.tri < 0) { off += NB; continue; }
    const uint32_t cnt = (nr.skip - off + NB) / (2u * NB);   // a collapsed leaf holds its whole subtree's triangles
    for (uint32_t k = 0; k < cnt; ++k) {
      const uint32_t s = (uint32_t)nr.tri + k;
      const bool r = reach && !(planes_dist2(p, record_at<TriPlanes>(mesh.planes, s)) > thr);
      if (__ballot(r) == 0ull) continue;
      const TriRec tr = record_at<TriRec>(mesh.tris, s);
      if (r) {
        const uint32_t before = best.idx;
        eval_triangle<MODE_NEAREST_NORMAL>(best, p, tr);
        if (best.idx != before) slot = s;
      }
    }
    off = nr.skip;
  }
}

// Winner -> outputs: the index, closest_point_triangle (geo.rs:70-138, the arithmetic eval_triangle measured) and the distance as the
// distance walks finish it (f32::MAX when nothing was comparable).
__device__ __forceinline__ void closest_store(const DeviceMesh& mesh, f3 p, const Best<MODE_NEAREST_NORMAL>& best, uint32_t slot,
                                              const ClosestOut& out, size_t i) {
  f3 c = mk3(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
  if (best.idx != NO_TRIANGLE) {
    const TriRec tr = mesh.tris[slot];
    const TriEdges e = {mk3(tr.abx, tr.aby, tr.abz), mk3(tr.acx, tr.acy, tr.acz), mk3(tr.bcx, tr.bcy, tr.bcz)};
    c = closest_point_triangle(p, mk3(tr.ax, tr.ay, tr.az), mk3(tr.bx, tr.by, tr.bz), mk3(tr.cx, tr.cy, tr.cz), e, tr.cls);
  }
  if (out.tri) out.tri[i] = best.idx;
  if (out.point) { out.point[3 * i] = c.x; out.point[3 * i + 1] = c.y; out.point[3 * i + 2] = c.z; }
  if (out.dist) out.dist[i] = fminf(F32_MAX_C, sqrtf(best.d2));
}

// Grid: packet = one brick of the slab in the walk's order (grid_lane_voxel / grid_point: the walk's cell centres, bit for bit).
// dist_in holds the first pass's slab (cell index - dist_off); the outputs are indexed by cell index - out.off.
template <bool ALL_PAIRS>
__global__ __launch_bounds__(64) void k_closest_grid(DeviceMesh mesh, GridParams g, const float* __restrict__ dist_in, uint64_t dist_off,
                                                     ClosestOut out) {
  const GridBrick vox = grid_lane_voxel(g, blockIdx.x, (int)threadIdx.x);
  if (!vox.brick_in_grid) return;   // padding of the last super-bricks: wave-uniform
  const f3 p = grid_point(g, vox);
  const size_t cell = ((size_t)vox.x * g.n[1] + vox.y) * g.n[2] + vox.z;
  const bool valid = vox.in_range;
  const float d = valid ? dist_in[cell - dist_off] : 0.0f;
  Best<MODE_NEAREST_NORMAL> best;
  uint32_t slot = 0;
  closest_search<ALL_PAIRS>(mesh, p, d, valid, best, slot);
  if (valid) closest_store(mesh, p, best, slot, out, cell - out.off);
}

// Queries: packet = 64 consecutive positions of the Morton order (perm: sorted position -> query; nullptr = input order).
template <bool ALL_PAIRS>
__global__ __launch_bounds__(64) void k_closest_q(DeviceMesh mesh, const float* __restrict__ queries, const uint32_t* __restrict__ perm,
                                                  uint32_t n_q, const float* __restrict__ dist_in, ClosestOut out) {
  const uint32_t j = blockIdx.x * 64u + threadIdx.x;
  const bool valid = j < n_q;
  const uint32_t i = valid ? (perm ? perm[j] : j) : 0u;
  const f3 p = valid ? mk3(queries[3 * (size_t)i], queries[3 * (size_t)i + 1], queries[3 * (size_t)i + 2]) : mk3(0.0f, 0.0f, 0.0f);
  const float d = valid ? dist_in[i] : 0.0f;
  Best<MODE_NEAREST_NORMAL> best;
  uint32_t slot = 0;
  closest_search<ALL_PAIRS>(mesh, p, d, valid, best, slot);
  if (valid) closest_store(mesh, p, best, slot, out, i);
}

}  // namespace

int launch_closest_grid(hipStream_t st, const DeviceMesh& mesh, const GridParams& g, const float* d_dist, uint64_t dist_off, int algorithm,
                        const ClosestOut& out) {
  const uint32_t packets = host_packet_bricks(g);
  if (packets == 0) return 0;
  M2S_REQUIRE_GRID_CONSTS(g);
  if (algorithm == 1) hipLaunchKernelGGL(k_closest_grid<true>, dim3(packets), dim3(64), 0, st, mesh, g, d_dist, dist_off, out);
  else hipLaunchKernelGGL(k_closest_grid<false>, dim3(packets), dim3(64), 0, st, mesh, g, d_dist, dist_off, out);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_closest_queries(hipStream_t st, const DeviceMesh& mesh, const float* d_queries, const uint32_t* perm, size_t n_q, const float* d_dist,
                           int algorithm, const ClosestOut& out) {
  if (n_q == 0) return 0;
  const uint32_t nq = (uint32_t)n_q, packets = (nq + 63u) / 64u;
  if (algorithm == 1) hipLaunchKernelGGL(k_closest_q<true>, dim3(packets), dim3(64), 0, st, mesh, d_queries, perm, nq, d_dist, out);
  else hipLaunchKernelGGL(k_closest_q<false>, dim3(packets), dim3(64), 0, st, mesh, d_queries, perm, nq, d_dist, out);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace m2s
