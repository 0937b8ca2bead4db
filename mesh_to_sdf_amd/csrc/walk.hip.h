// walk.hip.h — the pieces of the nearest-triangle walks that more than one translation unit needs:
// record loads, the grid's point source, the per-lane search state with its tie rule, the pruning
// threshold and the lower bounds of a node and of a leaf triangle.  Included by distance.hip (the
// distance walks), its sibling units (dist.hip.h) and closest.hip (the closest-point pass); every definition is inline and lives in
// an anonymous namespace, so each translation unit keeps its own copy and inlines it as before.
#pragma once
#include "common.h"
#include "geo.hip.h"

namespace m2s {

namespace {

constexpr float F32_MAX_C = 3.402823466e+38f;

// Record `index` of a read-only array through a 32-bit BYTE offset: a wave-uniform offset then goes straight into
// the scalar load's offset operand (no 64-bit address arithmetic in the walk loops).  Arrays stay below 4 GiB:
// 96 B x n_tris with n_tris < 2^25 (checked by the build).
// The records are read through the CONSTANT address space: the mesh arrays are never written while a walk runs, and only for a
// constant-address-space load does the compiler keep a wave-uniform address on the scalar unit (s_load) whatever else the kernel
// does — a global-address-space load falls back to the vector unit as soon as the kernel stores or performs an atomic anywhere
// before it ("may be clobbered"), which is what the suspension path of the split walk does (first version: every node record
// through global_load, walk 7.9 -> 17.2 ms).
template <class T>
__device__ __forceinline__ T record_at_bytes(const void* base, uint32_t byte_offset) {
  static_assert(sizeof(T) % 16 == 0 && alignof(T) >= 16, "records are whole 16-byte words");
  // builtin vectors (they load from any address space), declared 16-byte aligned: one s_load_dwordx16 / x8 / x4 each
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  typedef uint32_t u32x8 __attribute__((ext_vector_type(8), aligned(16)));
  typedef uint32_t u32x16 __attribute__((ext_vector_type(16), aligned(16)));
  typedef const __attribute__((address_space(4))) char* const_bytes;
  const const_bytes q = (const_bytes)(uintptr_t)base + byte_offset;
  constexpr unsigned N16 = sizeof(T) / 64, R16 = sizeof(T) % 64, N8 = R16 / 32, N4 = (R16 % 32) / 16;
  union { T rec; unsigned char raw[sizeof(T)]; } u;
#pragma unroll
  for (unsigned k = 0; k < N16; ++k) { const u32x16 v = *(const __attribute__((address_space(4))) u32x16*)(q + 64 * k); __builtin_memcpy(u.raw + 64 * k, &v, 64); }
#pragma unroll
  for (unsigned k = 0; k < N8; ++k) { const u32x8 v = *(const __attribute__((address_space(4))) u32x8*)(q + 64 * N16 + 32 * k); __builtin_memcpy(u.raw + 64 * N16 + 32 * k, &v, 32); }
#pragma unroll
  for (unsigned k = 0; k < N4; ++k) { const u32x4 v = *(const __attribute__((address_space(4))) u32x4*)(q + 64 * N16 + 32 * N8 + 16 * k); __builtin_memcpy(u.raw + 64 * N16 + 32 * N8 + 16 * k, &v, 16); }
  return u.rec;
}
template <class T>
__device__ __forceinline__ T record_at(const T* base, uint32_t index) {
  return record_at_bytes<T>(base, index * (uint32_t)sizeof(T));
}

// The 96-byte triangle records of the exact evaluation are read through the VECTOR path although their address
// is wave-uniform: a uniform-address vector load is a broadcast out of the 32 KB vector L1, lands in VGPRs, waits
// on the in-order vmcnt — and keeps the 16 KB scalar cache for the node records (and the 64-byte pre-test planes)
// of the walk.  Measured on 512^3 x blob-100k: both leaf records scalar 14.9 ms (kernel), both vector 14.05,
// planes scalar + triangle vector 13.67, the other way round 14.36.  The index is laundered through a VGPR so that
// the compiler does not turn the load back into a scalar one.
template <class T>
__device__ __forceinline__ T record_at_vec(const T* base, uint32_t uniform_index) {
  uint32_t vi;
  asm("v_mov_b32_e32 %0, %1" : "=v"(vi) : "s"(uniform_index));
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + (size_t)vi * sizeof(T));
}

// ---- point sources -------------------------------------------------------------------------
struct GridBrick {
  uint32_t x, y, z;
  uint32_t bx, by, bz;
  bool in_range;
  bool brick_in_grid;
};

// Brick sequence number -> brick coordinates.  Bricks are walked in 8x8x8 super-bricks (z fastest inside
// and between them), so that consecutive packets of an XCD keep touching the same part of the BVH while
// its 4 MiB L2 still holds it; a plain z-y-x sweep returns to a node only after a whole z column.
// A thin x-slab uses super-bricks that are 4, 2 or 1 bricks wide in x instead (common.h super_brick_xlog).  The width's log and the
// super-brick counts are the call's constants, resolved on the host (GridParams::sb_xl, sy, sz: common.h set_super_brick_magic).
__device__ __forceinline__ uint32_t div_magic(uint32_t n, uint32_t d, uint32_t magic) {
  return magic ? __umulhi(n, magic) : n / d;   // common.h set_super_brick_magic
}
__device__ __forceinline__ void brick_coords(const GridParams& g, uint32_t brick, uint32_t* bx, uint32_t* by, uint32_t* bz) {
  const uint32_t sy = g.sy, sz = g.sz, xl = g.sb_xl;
  const uint32_t sb = brick >> (6 + xl), in = brick & ((64u << xl) - 1u);   // super-brick index, position inside (padded grid)
  const uint32_t t = div_magic(sb, sz, g.sz_magic), sbz = sb - t * sz;
  const uint32_t sbx = div_magic(t, sy, g.sy_magic), sby = t - sbx * sy;
  *bx = (sbx << xl) + (in >> 6);
  *by = sby * 8 + ((in >> 3) & 7u);
  *bz = sbz * 8 + (in & 7u);
}
__device__ __forceinline__ GridBrick grid_lane_voxel(const GridParams& g, uint32_t brick, int lane) {
  uint32_t bx, by, bz;
  brick_coords(g, brick, &bx, &by, &bz);
  GridBrick v;
  const uint32_t lx = g.bl[0], ly = g.bl[1], lz = g.bl[2], l = (uint32_t)lane;   // z in the low bits: the fastest axis
  const uint32_t layers = g.xe - g.xb, xv = (bx << lx) + (l >> (ly + lz));   // layer of the (virtual) slab
  v.y = (by << ly) + ((l >> lz) & ((1u << ly) - 1u));
  v.z = (bz << lz) + (l & ((1u << lz) - 1u));
  v.in_range = xv < layers && v.y < g.n[1] && v.z < g.n[2];
  v.brick_in_grid = ((bx << lx) < layers) && ((by << ly) < g.n[1]) && ((bz << lz) < g.n[2]);
  v.bx = bx; v.by = by; v.bz = bz;
  v.x = slab_x(g, min(xv, layers - 1u));
  v.y = min(v.y, g.n[1] - 1);
  v.z = min(v.z, g.n[2] - 1);
  return v;
}
__device__ __forceinline__ f3 grid_point(const GridParams& g, const GridBrick& v) {
  return {cell_center(g.first[0], g.size[0], v.x), cell_center(g.first[1], g.size[1], v.y),
          cell_center(g.first[2], g.size[2], v.z)};  // grid.rs:135-141
}
__device__ __forceinline__ uint32_t grid_brick_count(const GridParams& g) {
  return bricks_along(g.xe - g.xb, g.bl[0]) * bricks_along(g.n[1], g.bl[1]) * bricks_along(g.n[2], g.bl[2]);
}

// Bricks in plain z-y-x order, no padding to super-bricks (k_brute_split: every packet costs the same, order is irrelevant).
__device__ __forceinline__ GridBrick grid_lane_voxel_plain(const GridParams& g, uint32_t brick, int lane) {
  const uint32_t nby = g.nby, nbz = g.nbz;
  const uint32_t bz = brick % nbz, t = brick / nbz, by = t % nby, bx = t / nby;
  GridBrick v;
  const uint32_t lx = g.bl[0], ly = g.bl[1], lz = g.bl[2], l = (uint32_t)lane;
  const uint32_t layers = g.xe - g.xb, xv = (bx << lx) + (l >> (ly + lz));
  v.y = (by << ly) + ((l >> lz) & ((1u << ly) - 1u));
  v.z = (bz << lz) + (l & ((1u << lz) - 1u));
  v.in_range = xv < layers && v.y < g.n[1] && v.z < g.n[2];
  v.brick_in_grid = true;
  v.bx = bx; v.by = by; v.bz = bz;
  v.x = slab_x(g, min(xv, layers - 1u));
  v.y = min(v.y, g.n[1] - 1);
  v.z = min(v.z, g.n[2] - 1);
  return v;
}

// XCD-aware work order: the dispatcher places block b on XCD b % 8.  Each XCD works through runs of 2^XCD_RUN_LOG consecutive
// packets (its private L2 keeps seeing the same part of the BVH), and the runs are dealt out round-robin — XCD x takes the runs
// x, x+8, x+16, ...: every XCD still works through whole super-bricks, and no XCD is handed the expensive eighth of the grid, as
// one contiguous eighth per XCD did (matters most for the thin multi-GPU pieces, which have few runs).
#ifndef M2S_XCD_RUN_LOG
#define M2S_XCD_RUN_LOG 8
#endif
constexpr uint32_t XCD_RUN_LOG = M2S_XCD_RUN_LOG;   // 7 is as fast, 8 re-fetches less (L2 misses 363 -> 263 MB on the headline)
__device__ __forceinline__ uint32_t xcd_remap(uint32_t b) {
  const uint32_t i = b >> 3, x = b & 7u;
  return ((((i >> XCD_RUN_LOG) << 3) + x) << XCD_RUN_LOG) | (i & ((1u << XCD_RUN_LOG) - 1u));
}

// ---- per-lane search state -----------------------------------------------------------------
template <int MODE>
struct Best {
  float d2 = __builtin_inff();      // min d2 over all triangles
  float d2pos = __builtin_inff();   // MODE_NORMAL_FOLD: min d2 over triangles with positive signed distance
  uint32_t idx = 0xffffffffu;       // MODE_NEAREST_NORMAL: triangle achieving d2 (lowest index on ties)
  bool pos = false;                 // MODE_NEAREST_NORMAL: its sign
  bool nan = false;
};

template <int MODE>
__device__ __forceinline__ void eval_triangle(Best<MODE>& best, f3 p, const TriRec& tr) {
  const f3 a = mk3(tr.ax, tr.ay, tr.az), b = mk3(tr.bx, tr.by, tr.bz), c = mk3(tr.cx, tr.cy, tr.cz);
  const TriEdges e = {mk3(tr.abx, tr.aby, tr.abz), mk3(tr.acx, tr.acy, tr.acz), mk3(tr.bcx, tr.bcy, tr.bcz)};
  const uint32_t cls = tr.cls, index = tr.index;
  if (MODE == MODE_UNSIGNED) {
    const float d2 = point_triangle_dist2(p, a, b, c, e, cls);
    best.d2 = fminf(best.d2, d2);  // f32::min drops a NaN operand (default.rs:47)
  } else {
    bool positive;
    const float d2 = point_triangle_dist2_signed_n(p, a, b, c, e, cls, mk3(tr.nrx, tr.nry, tr.nrz), &positive);
    if (MODE == MODE_NORMAL_FOLD) {
      best.nan |= !(d2 == d2);  // the reference panics: "NaN distance" (lib.rs:257)
      best.d2 = fminf(best.d2, d2);
      if (positive) best.d2pos = fminf(best.d2pos, d2);
    } else {
      if (d2 < best.d2 || (d2 == best.d2 && index < best.idx)) { best.d2 = d2; best.idx = index; best.pos = positive; }
    }
  }
}

// eval_triangle for the leaf triangles of the packet walk.  `reach` = this lane's pre-test bound reaches the triangle;
// a lane without it cannot be improved (that is what the pre-test's margin guarantees) and is left alone.  If every lane
// that is reached lies in a VERTEX region of the triangle (geo.rs:97-111 — 40 % of the evaluations on the benchmark: the
// fan of triangles around a voxel's nearest vertex, all at exactly the same distance), the closest point is that vertex
// and the edge / interior half of the computation (selects, the division, the reconstruction) is skipped for the wave.
// Same arithmetic for the lanes that count, so the result is bit-identical.
template <int MODE>
__device__ __forceinline__ void eval_triangle_leaf(Best<MODE>& best, f3 p, const TriRec& tr, bool reach) {
  if (MODE == MODE_NEAREST_NORMAL || tr.cls != TRI_REGULAR) { eval_triangle<MODE>(best, p, tr); return; }
  const f3 a = mk3(tr.ax, tr.ay, tr.az), b = mk3(tr.bx, tr.by, tr.bz), c = mk3(tr.cx, tr.cy, tr.cz);
  const f3 ab = mk3(tr.abx, tr.aby, tr.abz), ac = mk3(tr.acx, tr.acy, tr.acz);
  const RegularHead h = closest_point_regular_head(p, a, b, c, ab, ac);
  const bool vertex = h.rA | h.rB | h.rC;
  f3 q;
  bool valid = true;
  if (__ballot(reach & !vertex) == 0ull) {
    q = closest_point_regular_vertex(h, a, b, c);
    valid = vertex;                      // the other lanes are not reached: nothing to learn for them
  } else {
    q = closest_point_regular_tail(h, a, b, c, ab, ac, mk3(tr.bcx, tr.bcy, tr.bcz));
  }
  const f3 d = sub3(p, q);
  float d2 = dot3(d, d);
  if (MODE == MODE_UNSIGNED) {
    d2 = valid ? d2 : __builtin_inff();
    best.d2 = fminf(best.d2, d2);  // f32::min drops a NaN operand (default.rs:47)
  } else {   // MODE_NORMAL_FOLD
    const bool positive = dot3(d, mk3(tr.nrx, tr.nry, tr.nrz)) > 0.0f;
    best.nan |= valid & !(d2 == d2);  // the reference panics: "NaN distance" (lib.rs:257)
    d2 = valid ? d2 : __builtin_inff();
    best.d2 = fminf(best.d2, d2);
    if (positive) best.d2pos = fminf(best.d2pos, d2);
  }
}

template <int MODE>
__device__ __forceinline__ float finish(const Best<MODE>& best, bool negate_unsigned) {
  if (MODE == MODE_UNSIGNED) {
    const float d = fminf(F32_MAX_C, sqrtf(best.d2));   // fold starts from f32::MAX (default.rs:45)
    return negate_unsigned ? -d : d;
  }
  if (MODE == MODE_NORMAL_FOLD) return normal_fold_result(best.d2, best.d2pos);
  const float d = sqrtf(best.d2);
  return best.pos ? d : -d;                              // rtree.rs:118-123
}

// Pruning threshold in d2 space for the current best: a node or a triangle is looked at while its lower bound is <= (d (1 + PRUNE_REL) +
// slack)^2, with `slack` absolute (~67 ulp of the coordinate scale, + the approx_eq window of 1e-6 in Normal mode).
// What the relative part has to cover ("The pruning margin"; u = 2^-24): a triangle T may only be skipped if its
// COMPUTED distance could neither beat nor tie (Normal: approx_eq, 2 ulp) the final minimum.  With delta the true distance of T and B a
// computed lower bound of something that contains T:  B <= delta (1 + e_B) + a_B  and  computed d_T >= delta (1 - e_T) - a_T, where the
// absolute parts a_B, a_T (coordinate cancellation: <= ~16 u x scale together) are what `slack` is for, and the relative parts are
//   e_T <= 4 u     dot3 of the difference vector and the square root of the final comparison
//   e_B <= 7 u     ext_dist2 beyond 6.4 node radii (closer in, the 2e-6 x radius widening of the stored slab and the 1e-6 |v|^2 taken off the
//                  lateral term are larger than its rounding), planes_dist2 / box_dist2 likewise, + 1 u for the approximate square root here
//   2 u            the approx_eq tie window of the Normal fold (float-cmp ulps = 2)
// together < 14 u = 8.3e-7.  PRUNE_REL = 4e-6 is 4.8 times that.  (Rounds 1-4 used 2e-5: config 5's walk 78.6 -> 75.7 ms at 2e-6; far from
// a flat sheet the candidates within the margin are a disc of radius sqrt(2 m) D.)
constexpr float PRUNE_REL = 4.0e-6f;
__device__ __forceinline__ float prune_bound(float best_d2, float slack) {
  const float d = __builtin_amdgcn_sqrtf(best_d2);
  const float r = __builtin_fmaf(d, 1.0f + PRUNE_REL, slack);
  return r * r;
}

__device__ __forceinline__ float box_dist2(f3 p, float mnx, float mny, float mnz, float mxx, float mxy, float mxz) {
  const float dx = fmaxf(fmaxf(mnx - p.x, p.x - mxx), 0.0f);
  const float dy = fmaxf(fmaxf(mny - p.y, p.y - mxy), 0.0f);
  const float dz = fmaxf(fmaxf(mnz - p.z, p.z - mxz), 0.0f);
  return __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz));
}

// Lower bound (squared) of the distance from p to anything inside the node's disc-shaped slab
// (common.h NodeExt).  Every rounding is taken towards a SMALLER bound; FMAs are fine here.
__device__ __forceinline__ float ext_dist2(f3 p, const NodeExt& e) {
  const float vx = p.x - e.cx, vy = p.y - e.cy, vz = p.z - e.cz;
  const float t = __builtin_fmaf(e.nz, vz, __builtin_fmaf(e.ny, vy, e.nx * vx));
  const float v2 = __builtin_fmaf(vz, vz, __builtin_fmaf(vy, vy, vx * vx));
  // l^2 = v2 - t^2 cancels when p sits over the disc centre: shave a few ulps of v2 off first
  const float l2 = __builtin_fmaf(-1.0e-6f, v2, __builtin_fmaf(-t, t, v2));
  // l2 < 0 (rounding) gives sqrt = NaN and fmaxf(NaN - R, 0) = 0: still a valid lower bound
  const float lat = fmaxf(__builtin_amdgcn_sqrtf(l2) - e.R, 0.0f);
  const float s = fmaxf(fabsf(t - e.mid) - e.half, 0.0f);
  return __builtin_fmaf(s, s, lat * lat);
}

// Leaf pre-test (common.h TriPlanes): squared lower bound of the distance from p to the triangle itself.
__device__ __forceinline__ float planes_dist2(f3 p, const TriPlanes& t) {
  const float h = __builtin_fmaf(t.nz, p.z, __builtin_fmaf(t.ny, p.y, t.nx * p.x)) - t.dn;
  const float e0 = __builtin_fmaf(t.m0z, p.z, __builtin_fmaf(t.m0y, p.y, t.m0x * p.x)) - t.o0;
  const float e1 = __builtin_fmaf(t.m1z, p.z, __builtin_fmaf(t.m1y, p.y, t.m1x * p.x)) - t.o1;
  const float e2 = __builtin_fmaf(t.m2z, p.z, __builtin_fmaf(t.m2y, p.y, t.m2x * p.x)) - t.o2;
  const float e = fmaxf(fmaxf(e0, e1), fmaxf(e2, 0.0f));
  return __builtin_fmaf(h, h, e * e);
}

}  // namespace

}  // namespace m2s
