// rays.hip — watertight ray casting against the mesh (m2s_cast_rays, m2s_mesh_cast_rays), gfx950.  DESIGN.md §4.10.
//
// One ray per lane.  Rays are incoherent (a lane's neighbours need other subtrees), so every lane walks the stackless pre-order tree
// on its own, as stab_count_lane does for the three axis rays of the Raycast sign: i = accepted && !leaf ? i + 1 : skip.  The walk
// reads the NodeRec boxes and `corners` only (+ one dword of a TriRec, the caller's triangle index, for a hit that may become the
// first), and takes the tree as it is: a node whose `tri` mark is set is a leaf of (skip - i + 1) / 2 triangles from `tri`, whatever
// leaf size the tree was last marked with.  The triangle test is ray.hip.h; algorithm 1 runs it over every triangle, and that form
// is the definition: the walk must return the same bits.
//
// ---- the box test: conservative bit for bit, by monotonicity alone ------------------------------------------------------------------
// What the walk may skip is decided in the ray's own sheared frame, with the triangle test's own operations.  No step of the argument
// is an error bound; each is "rounding is monotone" (x <= y implies fl(x) <= fl(y), for every IEEE operation in either operand).
//   1. The test maps a vertex v to  X(v) = fl(fl(v[kx] - o[kx]) - fl(Sx * fl(v[kz] - o[kz]))),  Y(v) likewise,  Z(v) = fl(Sz * fl(v[kz] - o[kz])).
//      X is non-decreasing in v[kx] and monotone in v[kz] (the direction is the sign of Sx).  A node's box [lo, hi] contains the vertices
//      of its subtree as `corners` holds them (a leaf box is the vertices' min / max moved OUTWARDS by the 1e-4 padding — where that is
//      below an ulp the box is the bare min / max, which still contains them — and an inner box is an exact min / max of boxes).  Hence
//        Xlo = fl(fl(lo[kx] - o[kx]) - max(fl(Sx * zl), fl(Sx * zh))),  Xhi = fl(fl(hi[kx] - o[kx]) - min(..)),   zl, zh = fl(lo / hi[kz] - o[kz]),
//      bound the COMPUTED X of every vertex below the node: Xlo <= X(v) <= Xhi.  The same for Y, and Zlo = min(fl(Sz zl), fl(Sz zh)) <=
//      Z(v) <= Zhi.  Nothing is owed to the shear, the translation or the padding.
//   2. So for a triangle below the node, with xl / xh, yl / yh, zl / zh the min / max of its three computed points (ray.hip.h):
//      Xlo <= xl, xh <= Xhi, ..., and the largest |coordinate| of the node's rectangle is at least the triangle's, hence
//      mxy(node) = fl(2^-20 * that) >= mxy(triangle), and mz(node) >= mz(triangle) likewise.
//   3. The node is skipped when  Xlo > mxy(node)  — then xl >= Xlo > mxy(node) >= mxy(triangle): the definition's XY clause calls that a
//      miss — or Xhi < -mxy(node), or the same in Y;  when fl(Zhi + mz(node)) < t_min  — a hit has t <= fl(zh + mz) <= fl(Zhi + mz(node)) by
//      the Z clause, so it is below the range;  or when fl(Zlo - mz(node)) > limit  — a hit has t >= fl(zl - mz) >= fl(Zlo - mz(node)) >
//      limit.  limit is t_max, or the best t so far when only the first hit is wanted: the comparison is STRICT, so a triangle that ties
//      the best t with a lower index is still evaluated.
//   NaNs (infinite boxes, overflowing differences) fail every comparison: the node is accepted.
// Every triangle the definition reports in range therefore lies below accepted nodes only, on every ray, and walk and all pairs
// return the same bits whatever leaf size the tree is marked with.
//
// ---- why the definition has the two clauses, and what they cost it -------------------------------------------------------------------
// (u = 2^-24.)  Without them the margins would have to cover what the triangle test does after step 1, and cannot:
//   XY.  U = fl(Cx By) - fl(Cy Bx): the subtraction of two floats has the exact sign, and rounding is monotone, so a computed edge
//     function has the sign of the exact one (of the computed 2-D points) or is ZERO; it is never of the wrong sign.  A hit of the bare
//     test is therefore either a hit of the exact 2-D triangle — then the origin lies in it, hence in the rectangle, margin 0 — or one
//     where an exact non-zero edge function rounded to zero: fl(Cx By) == fl(Cy Bx), so |cross(C, B)| <= 2u |C||B|, the origin sees the
//     edge BC under an angle below 2u.  With the origin's foot on the edge that puts it within u |BC| / 2 of the edge; with the foot
//     beyond an end by r it needs an altitude h of the 2-D triangle with h <= 2u (r + |BC|) (the origin must also stay inside the cone of
//     the opposite vertex, so its offset from the edge's line is at least r h / |BC|).  L = the largest |coordinate| of the rectangle
//     bounds |B|, |C| and r by 2 sqrt(2) L.  The clause's 2^-20 = 16 u of L keeps every such hit of a triangle whose 2-D altitudes exceed
//     8 u L — eight ulps of its distance from the ray: on those the clause changes nothing.  Below that the image is degenerate: the ray
//     lies in the triangle's plane (common: any ray in a plane of symmetry of the mesh), or the triangle is a sliver below the resolution
//     of its coordinates; U, V, W are all rounding noise and the bare test reports hits at distances of order L from the three points
//     (measured: a strip along a blob's meridians under radial rays, axis 0.5 to 0.97 L outside the rectangle).  Two points of ANY
//     rectangle can be in line with the origin, so no box test bounds those short of visiting every node, and which of them a walk met
//     would depend on how the tree is marked.  The clause removes exactly them.  It does not open the mesh: a ray through a shared edge
//     or vertex has the axis ON the rectangle of every triangle that includes it.  (Degenerate triangles, two equal vertices, never hit:
//     two edge functions are exact negatives of each other and the third is 0.)
//   Z.  For a hit U, V, W have one sign, so t = fl(fl(fl(fl(U Az) + fl(V Bz)) + fl(W Cz)) / det) is a rounded weighted mean of Az, Bz, Cz
//     with weights of one sign: the products and the two additions of the numerator err by at most 3.1 u sum |w z|, det = fl(fl(U + V) + W)
//     by 2 u (no cancellation), the division by u, so |t - mean| <= 7 u max |z| and the mean lies in [zl, zh]: the clause's 2^-21 = 8 u of
//     max |z| changes nothing — unless products underflow (coordinates below 1e-19), where the absolute error 2^-150 of a product,
//     divided by a tiny det, is unbounded.  The clause cuts those off.
#include "common.h"
#include "geo.hip.h"
#include "ray.hip.h"

namespace m2s {

void warm_rays(hipStream_t st);

namespace {

__global__ void k_warm_rays() {}

enum : int { RAYS_ALL = 0 /* every hit in range: count wanted */, RAYS_FIRST = 1 /* prune against the best t */, RAYS_ANY = 2 /* occluded only */ };

__device__ __forceinline__ bool ray_box_accept(const RaySetup& r, f3 o, const NodeRec& nr, float t_min, float limit) {
  const f3 lo = sub3(mk3(nr.mnx, nr.mny, nr.mnz), o), hi = sub3(mk3(nr.mxx, nr.mxy, nr.mxz), o);
  const float zl = axis3(lo, r.kz), zh = axis3(hi, r.kz);
  const float sx0 = r.Sx * zl, sx1 = r.Sx * zh, sy0 = r.Sy * zl, sy1 = r.Sy * zh, z0 = r.Sz * zl, z1 = r.Sz * zh;
  const float Xlo = axis3(lo, r.kx) - fmaxf(sx0, sx1), Xhi = axis3(hi, r.kx) - fminf(sx0, sx1);
  const float Ylo = axis3(lo, r.ky) - fmaxf(sy0, sy1), Yhi = axis3(hi, r.ky) - fminf(sy0, sy1);
  const float Zlo = fminf(z0, z1), Zhi = fmaxf(z0, z1);
  const float mxy = RAY_XY_REL * fmaxf(fmaxf(fabsf(Xlo), fabsf(Xhi)), fmaxf(fabsf(Ylo), fabsf(Yhi)));
  const float mz = RAY_Z_REL * fmaxf(fabsf(Zlo), fabsf(Zhi));
  return !(Xlo > mxy) && !(Xhi < -mxy) && !(Ylo > mxy) && !(Yhi < -mxy) && !(Zhi + mz < t_min) && !(Zlo - mz > limit);
}

struct RayBest {
  float t = __builtin_inff(), u = __builtin_nanf(""), v = __builtin_nanf("");
  uint32_t tri = 0xffffffffu, count = 0;
};

// Triangle `slot` of the sorted arrays against one ray.  The first hit is the smallest t, the lowest caller's index on exact ties.
template <int KIND>
__device__ __forceinline__ void ray_eval(const DeviceMesh& mesh, const RaySetup& r, f3 o, float t_min, float t_max, uint32_t slot, RayBest& best) {
  const float4 c0 = mesh.corners[3 * (size_t)slot], c1 = mesh.corners[3 * (size_t)slot + 1], c2 = mesh.corners[3 * (size_t)slot + 2];
  float t, u, v;
  if (!ray_triangle_in_range(r, o, mk3(c0.x, c0.y, c0.z), mk3(c0.w, c1.x, c1.y), mk3(c1.z, c1.w, c2.x), t_min, t_max, &t, &u, &v)) return;
  best.count += 1u;
  if (KIND == RAYS_ANY || t > best.t) return;
  const uint32_t index = mesh.tris[slot].index;
  if (t < best.t || index < best.tri) { best.t = t; best.u = u; best.v = v; best.tri = index; }
}

template <bool ALL_PAIRS, int KIND>
__global__ __launch_bounds__(256) void k_rays(DeviceMesh mesh, const float* __restrict__ org, const float* __restrict__ dir, uint32_t n_rays,
                                              float t_min, float t_max, RayOut out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rays) return;
  const f3 o = mk3(org[3 * (size_t)i], org[3 * (size_t)i + 1], org[3 * (size_t)i + 2]);
  const RaySetup r = ray_setup(o, mk3(dir[3 * (size_t)i], dir[3 * (size_t)i + 1], dir[3 * (size_t)i + 2]));
  RayBest best;
  if (r.valid) {
    if (ALL_PAIRS) {
      // (not unrolled: left to itself the compiler unrolls the occlusion-only form, whose body only counts, to 136 VGPRs)
#pragma clang loop unroll(disable)
      for (uint32_t k = 0; k < mesh.n_tris; ++k) {
        ray_eval<KIND>(mesh, r, o, t_min, t_max, k, best);
        if (KIND == RAYS_ANY && best.count != 0u) break;
      }
    } else {
      uint32_t node = 0;
      while (node < mesh.n_nodes) {
        const NodeRec nr = mesh.nodes[node];
        const float limit = KIND == RAYS_FIRST ? fminf(t_max, best.t) : t_max;
        if (!ray_box_accept(r, o, nr, t_min, limit)) { node = nr.skip; continue; }
        if (nr.tri < 0) { node += 1u; continue; }
        const uint32_t cnt = (nr.skip - node + 1u) >> 1;
#pragma clang loop unroll(disable)
        for (uint32_t k = 0; k < cnt; ++k) ray_eval<KIND>(mesh, r, o, t_min, t_max, (uint32_t)nr.tri + k, best);
        if (KIND == RAYS_ANY && best.count != 0u) break;   // the only output is "anything in the way"
        node = nr.skip;
      }
    }
  }
  if (out.t) out.t[i] = best.t;
  if (out.tri) out.tri[i] = best.tri;
  if (out.uv) { out.uv[2 * (size_t)i] = best.u; out.uv[2 * (size_t)i + 1] = best.v; }
  if (out.count) out.count[i] = best.count;
  if (out.occluded) out.occluded[i] = best.count != 0u ? 1 : 0;
}

template <bool ALL_PAIRS>
void launch_kind(hipStream_t st, int kind, uint32_t blocks, const DeviceMesh& mesh, const float* org, const float* dir, uint32_t n, float t_min,
                 float t_max, const RayOut& out) {
  if (kind == RAYS_ALL) hipLaunchKernelGGL((k_rays<ALL_PAIRS, RAYS_ALL>), dim3(blocks), dim3(256), 0, st, mesh, org, dir, n, t_min, t_max, out);
  else if (kind == RAYS_FIRST) hipLaunchKernelGGL((k_rays<ALL_PAIRS, RAYS_FIRST>), dim3(blocks), dim3(256), 0, st, mesh, org, dir, n, t_min, t_max, out);
  else hipLaunchKernelGGL((k_rays<ALL_PAIRS, RAYS_ANY>), dim3(blocks), dim3(256), 0, st, mesh, org, dir, n, t_min, t_max, out);
}

}  // namespace

void warm_rays(hipStream_t st) { hipLaunchKernelGGL(k_warm_rays, dim3(1), dim3(64), 0, st); }

int launch_cast_rays(hipStream_t st, const DeviceMesh& mesh, const float* d_org, const float* d_dir, size_t n_rays, float t_min, float t_max,
                     int algorithm, const RayOut& out) {
  if (n_rays == 0) return 0;
  const uint32_t n = (uint32_t)n_rays, blocks = (n + 255u) / 256u;
  // what has to be found: every hit (count), the first one (t, triangle, uv), or any one (occluded alone)
  const int kind = out.count ? RAYS_ALL : ((out.t || out.tri || out.uv) ? RAYS_FIRST : RAYS_ANY);
  if (algorithm == 1) launch_kind<true>(st, kind, blocks, mesh, d_org, d_dir, n, t_min, t_max, out);
  else launch_kind<false>(st, kind, blocks, mesh, d_org, d_dir, n, t_min, t_max, out);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace m2s
