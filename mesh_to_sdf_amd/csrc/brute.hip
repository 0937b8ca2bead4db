// brute.hip — all pairs, no tree (gfx950): every point against every triangle with the triangle records staged through LDS in tiles.
// k_brute is AccelerationMethod::None and the on-device cross-check of the walks; k_brute_split / k_brute_split_q cut the triangles into
// chunks as well, for problems so small that the tree is not worth building.  Same arithmetic as the walks (geo.hip.h, walk.hip.h).
#include <algorithm>

#include "common.h"
#include "geo.hip.h"
#include "tuning.h"
#include "walk.hip.h"
#include "dist.hip.h"

namespace m2s {

namespace {

constexpr int TILE = 128;  // triangles per LDS tile in k_brute (12 KiB)

// ---- k_brute --------------------------------------------------------------------------------
template <bool GRID, int MODE, int SIGN>
__global__ __launch_bounds__(256) void k_brute(DeviceMesh mesh, GridParams g, const float* __restrict__ queries,
                                               uint32_t n_q, const uint32_t* __restrict__ plane,
                                               float* __restrict__ out, int* __restrict__ err, uint32_t n_packets, PeerOut peers) {
  __shared__ TriRec tile[TILE];
  const int lane = threadIdx.x & 63;
  const uint32_t packet = blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool active = packet < n_packets;

  f3 p = {0, 0, 0};
  size_t out_index = 0;
  bool store = false;
  GridBrick vox{};
  if (active) {
    if (GRID) {
      vox = grid_lane_voxel(g, packet, lane);
      p = grid_point(g, vox);
      out_index = ((size_t)vox.x * g.n[1] + vox.y) * g.n[2] + vox.z - (size_t)g.out_off;
      store = vox.in_range;
    } else {
      const uint32_t i = min(packet * 64u + lane, n_q - 1);
      p = mk3(queries[3 * (size_t)i], queries[3 * (size_t)i + 1], queries[3 * (size_t)i + 2]);
      out_index = i;
      store = packet * 64u + lane < n_q;
    }
  }

  Best<MODE> best;
  uint32_t hits[3] = {0, 0, 0};
  for (uint32_t t0 = 0; t0 < mesh.n_tris; t0 += TILE) {
    const uint32_t nt = min((uint32_t)TILE, mesh.n_tris - t0);
    __syncthreads();
    {  // 128 records x 96 B = 768 float4; 256 threads x 3
      const float4* src = reinterpret_cast<const float4*>(mesh.tris + t0);
      float4* dst = reinterpret_cast<float4*>(tile);
      for (uint32_t i = threadIdx.x; i < nt * 6; i += 256) dst[i] = src[i];
    }
    __syncthreads();
    for (uint32_t k = 0; k < nt; ++k) {
      const TriRec& tr = tile[k];
      const f3 a = mk3(tr.ax, tr.ay, tr.az), b = mk3(tr.bx, tr.by, tr.bz), c = mk3(tr.cx, tr.cy, tr.cz);
      eval_triangle<MODE>(best, p, tr);
      if (MODE == MODE_UNSIGNED && SIGN == SIGN_XRAY_ALL) {
        float t;
        hits[0] += ray_triangle_aligned<0>(p, a, b, c, &t) ? 1u : 0u;   // default.rs:35-37: every triangle
      }
      if (MODE == MODE_UNSIGNED && SIGN == SIGN_RAYS3) {
        f3 mn, mx;
        triangle_bounding_box(a, b, c, &mn, &mx);
        float t;
        hits[0] += (ray_meets_box<0>(p, mn, mx) & ray_triangle_aligned<0>(p, a, b, c, &t)) ? 1u : 0u;
        hits[1] += (ray_meets_box<1>(p, mn, mx) & ray_triangle_aligned<1>(p, a, b, c, &t)) ? 1u : 0u;
        hits[2] += (ray_meets_box<2>(p, mn, mx) & ray_triangle_aligned<2>(p, a, b, c, &t)) ? 1u : 0u;
      }
    }
  }

  bool negate = false;
  if (MODE == MODE_UNSIGNED) {
    if (SIGN == SIGN_GRID_PLANE && active) {
      const size_t w = ((size_t)vox.x * g.n[1] + vox.y) * g.nzw + (vox.z >> 5);
      negate = (plane[w] >> (vox.z & 31u)) & 1u;
    } else if (SIGN == SIGN_XRAY_ALL) {
      negate = hits[0] & 1u;                                            // default.rs:65-72
    } else if (SIGN == SIGN_RAYS3) {
      negate = ((hits[0] & 1u) + (hits[1] & 1u) + (hits[2] & 1u)) > 1u;
    }
  }
  if (MODE == MODE_NORMAL_FOLD && best.nan && store) atomicOr(err, ERRF_NAN);
  const float result = finish<MODE>(best, negate);
  if (store) out[out_index] = result;
  if (GRID && store)
    for (uint32_t i = 0; i < peers.n; ++i) peers.p[i][out_index + (size_t)g.out_off] = result;
}

// ---- k_brute_split: tiny problems without a tree -------------------------------------------------------------------
// The reference's own criterion shapes include a 16^3 grid over an 11 k-triangle mesh (benches/generate_grid_sdf.rs:8-34): 4 096
// voxels are 64 waves, each lane walks the tree alone, and the call lasts as long as its slowest lane's chain of dependent loads
// (0.7 ms) on top of a 0.17 ms build.  All voxels x all triangles is only 46 M evaluations there — 0.1 ms if the whole chip takes
// part, and no tree is needed at all.  k_brute gives a block ALL triangles (16 blocks for 16^3); here the triangles are cut into
// chunks as well: block (x, y) evaluates voxel block x against triangle chunk y and folds its minima into per-voxel words with
// atomic minima (non-negative floats order like their bit patterns; min is associative and commutative: bit-identical to k_brute
// and to every walk), k_brute_finish turns them into signed distances.  Chosen for cells x triangles <= M2S_BRUTE_MAX.
template <int MODE>
__global__ __launch_bounds__(256) void k_brute_split(DeviceMesh mesh, GridParams g, uint32_t* __restrict__ acc, int* __restrict__ err,
                                                     uint32_t n_packets, uint32_t tiles_per_chunk) {
  __shared__ TriRec tile[TILE];
  const int lane = threadIdx.x & 63;
  const uint32_t packet = blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool active = packet < n_packets;
  f3 p = {0, 0, 0};
  bool store = false;
  if (active) {
    const GridBrick vox = grid_lane_voxel_plain(g, packet, lane);
    p = grid_point(g, vox);
    store = vox.in_range;
  }
  Best<MODE> best;
  const uint32_t t_begin = blockIdx.y * tiles_per_chunk * TILE, t_end = min(mesh.n_tris, t_begin + tiles_per_chunk * TILE);
  for (uint32_t t0 = t_begin; t0 < t_end; t0 += TILE) {
    const uint32_t nt = min((uint32_t)TILE, t_end - t0);
    __syncthreads();
    {
      const float4* src = reinterpret_cast<const float4*>(mesh.tris + t0);
      float4* dst = reinterpret_cast<float4*>(tile);
      for (uint32_t i = threadIdx.x; i < nt * 6; i += 256) dst[i] = src[i];
    }
    __syncthreads();
    for (uint32_t k = 0; k < nt; ++k) eval_triangle<MODE>(best, p, tile[k]);
  }
  if (!active || !store) return;
  const size_t slot = ((size_t)packet * 64u + lane) * 2u;
  atomicMin(&acc[slot], __float_as_uint(best.d2));
  if (MODE == MODE_NORMAL_FOLD) {
    atomicMin(&acc[slot + 1], __float_as_uint(best.d2pos));
    if (best.nan) atomicOr(err, ERRF_NAN);
  }
}
template <int MODE, int SIGN>
__global__ __launch_bounds__(256) void k_brute_finish(GridParams g, const uint32_t* __restrict__ plane, const uint32_t* __restrict__ acc,
                                                      float* __restrict__ out, uint32_t n_packets, PeerOut peers) {
  const int lane = threadIdx.x & 63;
  const uint32_t packet = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (packet >= n_packets) return;
  const GridBrick vox = grid_lane_voxel_plain(g, packet, lane);
  if (!vox.in_range) return;
  const size_t slot = ((size_t)packet * 64u + lane) * 2u;
  Best<MODE> best;
  best.d2 = __uint_as_float(acc[slot]);
  best.d2pos = __uint_as_float(acc[slot + 1]);
  bool negate = false;
  if (MODE == MODE_UNSIGNED && SIGN == SIGN_GRID_PLANE) {
    const size_t w = ((size_t)vox.x * g.n[1] + vox.y) * g.nzw + (vox.z >> 5);
    negate = (plane[w] >> (vox.z & 31u)) & 1u;
  }
  const float result = finish<MODE>(best, negate);
  const size_t out_index = ((size_t)vox.x * g.n[1] + vox.y) * g.n[2] + vox.z - (size_t)g.out_off;
  out[out_index] = result;
  for (uint32_t i = 0; i < peers.n; ++i) peers.p[i][out_index + (size_t)g.out_off] = result;
}

// ---- k_brute_split_q: small query sets without a tree ---------------------------------------------------------------
// The crate's documented use is a handful of query points (lib.rs:13-31, examples/demo.rs:29-54): for those the LBVH build (0.16 -
// 0.24 ms), the query sort and a lane walk that lasts as long as its slowest lane's chain of dependent loads (~1 ms) are all
// overhead — queries x triangles is a few 10^7 evaluations, 0.1 - 0.3 ms if the whole chip takes part.  As k_brute_split: block
// (x, y) evaluates query block x against triangle chunk y and folds into per-query words with atomics — minima for the distances
// (non-negative floats order like their bits), a 64-bit (d2, index, !positive) key for the Rtree rule (lowest index on ties, as
// the walks and k_brute take it), XOR for the three ray parities (the parity of a sum is the XOR of the parities) — and
// k_brute_finish_q turns the words into signed distances.  Per query: [0] d2, [1] d2 of the positive side (Normal fold) or the
// hit parities (bits 0..2: +X, +Y, +Z), [2..3] the key.  Same arithmetic per pair as everywhere else: bit-identical.
__global__ __launch_bounds__(256) void k_brute_q_init(uint32_t* __restrict__ acc, uint32_t n_q, uint32_t second) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_q) return;
  reinterpret_cast<uint4*>(acc)[i] = make_uint4(0x7f800000u, second, 0xffffffffu, 0xffffffffu);   // +inf, +inf or no hits, "no triangle"
}
template <int MODE, int SIGN>
__global__ __launch_bounds__(256) void k_brute_split_q(DeviceMesh mesh, const float* __restrict__ queries, uint32_t n_q, uint32_t* __restrict__ acc,
                                                       int* __restrict__ err, uint32_t tiles_per_chunk) {
  __shared__ TriRec tile[TILE];
  const uint32_t i_raw = blockIdx.x * 256u + threadIdx.x, i = min(i_raw, n_q - 1u);
  const f3 p = mk3(queries[3 * (size_t)i], queries[3 * (size_t)i + 1], queries[3 * (size_t)i + 2]);
  Best<MODE> best;
  uint32_t hits[3] = {0, 0, 0};
  const uint32_t t_begin = blockIdx.y * tiles_per_chunk * TILE, t_end = min(mesh.n_tris, t_begin + tiles_per_chunk * TILE);
  for (uint32_t t0 = t_begin; t0 < t_end; t0 += TILE) {
    const uint32_t nt = min((uint32_t)TILE, t_end - t0);
    __syncthreads();
    {
      const float4* src = reinterpret_cast<const float4*>(mesh.tris + t0);
      float4* dst = reinterpret_cast<float4*>(tile);
      for (uint32_t k = threadIdx.x; k < nt * 6; k += 256) dst[k] = src[k];
    }
    __syncthreads();
    for (uint32_t k = 0; k < nt; ++k) {
      const TriRec& tr = tile[k];
      eval_triangle<MODE>(best, p, tr);
      if (MODE == MODE_UNSIGNED && SIGN == SIGN_RAYS3) {               // the candidate rule of bvh.rs:119 / rtree_bvh.rs:149: the triangle's own padded box
        const f3 a = mk3(tr.ax, tr.ay, tr.az), b = mk3(tr.bx, tr.by, tr.bz), c = mk3(tr.cx, tr.cy, tr.cz);
        f3 mn, mx;
        triangle_bounding_box(a, b, c, &mn, &mx);
        float t;
        hits[0] += (ray_meets_box<0>(p, mn, mx) & ray_triangle_aligned<0>(p, a, b, c, &t)) ? 1u : 0u;
        hits[1] += (ray_meets_box<1>(p, mn, mx) & ray_triangle_aligned<1>(p, a, b, c, &t)) ? 1u : 0u;
        hits[2] += (ray_meets_box<2>(p, mn, mx) & ray_triangle_aligned<2>(p, a, b, c, &t)) ? 1u : 0u;
      }
    }
  }
  if (i_raw >= n_q) return;
  uint32_t* w = acc + 4 * (size_t)i;
  if (MODE == MODE_NEAREST_NORMAL) {
    if (best.idx != 0xffffffffu)
      atomicMin(reinterpret_cast<unsigned long long*>(w + 2), ((unsigned long long)__float_as_uint(best.d2) << 32) | ((unsigned long long)best.idx << 1) | (best.pos ? 0ull : 1ull));
    return;
  }
  atomicMin(&w[0], __float_as_uint(best.d2));
  if (MODE == MODE_NORMAL_FOLD) {
    atomicMin(&w[1], __float_as_uint(best.d2pos));
    if (best.nan) atomicOr(err, ERRF_NAN);
  } else if (SIGN == SIGN_RAYS3) {
    const uint32_t par = (hits[0] & 1u) | ((hits[1] & 1u) << 1) | ((hits[2] & 1u) << 2);
    if (par) atomicXor(&w[1], par);
  }
}
template <int MODE, int SIGN>
__global__ __launch_bounds__(256) void k_brute_finish_q(const uint32_t* __restrict__ acc, uint32_t n_q, float* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_q) return;
  const uint4 w = reinterpret_cast<const uint4*>(acc)[i];
  Best<MODE> best;
  bool negate = false;
  if (MODE == MODE_NEAREST_NORMAL) {
    best.d2 = __uint_as_float(w.w);                                    // high word of the key; "no triangle" reads as NaN, as a walk over nothing would not
    best.pos = (w.z & 1u) == 0u;
    if (w.w == 0xffffffffu && w.z == 0xffffffffu) { best.d2 = __builtin_inff(); best.pos = false; }
  } else {
    best.d2 = __uint_as_float(w.x);
    if (MODE == MODE_NORMAL_FOLD) best.d2pos = __uint_as_float(w.y);
    else if (SIGN == SIGN_RAYS3) negate = ((w.y & 1u) + ((w.y >> 1) & 1u) + ((w.y >> 2) & 1u)) > 1u;   // bvh.rs:131-141, rtree_bvh.rs:161-171
  }
  out[i] = finish<MODE>(best, negate);
}
template <bool GRID, int MODE, int SIGN>
void launch_brute(hipStream_t st, const DeviceMesh& mesh, const GridParams& g, const float* q, uint32_t n_q,
                  const uint32_t* plane, float* out, int* err, uint32_t n_packets, const PeerOut& peers = PeerOut{}) {
  hipLaunchKernelGGL((k_brute<GRID, MODE, SIGN>), dim3((n_packets + 3) / 4), dim3(256), 0, st, mesh, g, q, n_q, plane,
                     out, err, n_packets, peers);
}

}  // namespace

// Tiny problems take k_brute_split: at most 2^22 cells and cells x triangles <= 1e8 + 3000 x triangles (M2S_BRUTE_MAX overrides the
// product's limit).  Measured (tools/exp_tiny.py, whole calls, brute / build + walk): blob-11k 16^3
// 0.34 / 0.92 ms, 20^3 0.58 / 0.96, 24^3 0.92 / 0.83; blob-100k 8^3 0.41 / 2.21, 12^3 1.08 / 2.55, 16^3 2.21 / 2.22; blob-6k 16^3 0.20 / 0.74,
// 32^3 1.10 / 0.61 — brute force runs at 178 G point-triangle pairs per second (half the chip's fp32 issue rate), the walks of such
// grids as long as their slowest lane's chain of dependent loads, which grows with the mesh.
// Round 6 (packet groups, one-workgroup seed flood: the walks of small problems got faster), whole one-shot calls, brute / build + walk
// (tools/exp_tiny.py, profiles/r06_tiny.txt): suzanne (968 triangles) 16^3 Raycast 0.120 / 0.125 ms, 24^3 0.151 / 0.127, Normal 24^3 0.097 / 0.132, 32^3
// 0.136 / 0.128; blob-11k 12^3 Raycast 0.190 / 0.276, 16^3 0.323 / 0.232, Normal 16^3 0.204 / 0.231, 20^3 0.347 / 0.252; blob-100k 8^3 0.40 / 1.17,
// 12^3 Raycast 1.05 / 0.94, Normal 0.66 / 0.93.  Brute force costs 0.08 ms + pairs / 1.9e11 per s with the Raycast planes (0.06 + pairs / 3e11 for
// Normal), the walk 0.12 ms + 1e-5 ms per triangle: the limits below are where they cross (rounds 2 - 5: 1e8 + 3 000 per triangle for both).
bool grid_is_tiny(const GridParams& g, size_t n_tris, int algorithm, bool raycast, const Tuning& tn) {
  if (algorithm != 0 || n_tris == 0 || slab_is_empty(g) || g.chunk_log < 31u) return false;
  const double automatic = raycast ? 7.6e6 + 1.9e3 * (double)n_tris : 1.8e7 + 3.0e3 * (double)n_tris;
  const double limit = tn.brute_max >= 0.0 ? tn.brute_max : automatic;
  const double cells = (double)(g.xe - g.xb) * g.n[1] * g.n[2];
  return cells <= 4194304.0 && cells * (double)n_tris <= limit;
}
bool grid_is_tiny(const GridParams& g, size_t n_tris, int algorithm, bool raycast) { return grid_is_tiny(g, n_tris, algorithm, raycast, tuning()); }

// What a grid walk does on the path GridWalkChoice::ALL_PAIRS_SPLIT (tiny problems): `acc` holds two words per voxel of the slab's `real`
// bricks, preset to +inf.  `plane`: the sign planes, or nullptr (no sign, or the Normal fold).
int launch_grid_brute_split(hipStream_t st, const DeviceMesh& mesh, const GridParams& g, int mode, const uint32_t* plane, uint32_t* acc, uint32_t real,
                            float* d_out, int* d_err, const PeerOut& pz) {
  for_grid_form(mode, plane != nullptr, [&](auto form) {
    constexpr int MODE = decltype(form)::MODE, SIGN = decltype(form)::SIGN;
    // ~4 blocks per CU over (voxel blocks x triangle chunks); a chunk is a whole number of 128-triangle tiles
    const uint32_t vblocks = (real + 3) / 4, tiles = (mesh.n_tris + TILE - 1) / TILE;
    const uint32_t chunks = std::max(1u, std::min(tiles, (1024u + vblocks - 1) / vblocks));
    const uint32_t tiles_per_chunk = (tiles + chunks - 1) / chunks, ychunks = (tiles + tiles_per_chunk - 1) / tiles_per_chunk;
    hipLaunchKernelGGL((k_brute_split<MODE>), dim3(vblocks, ychunks), dim3(256), 0, st, mesh, g, acc, d_err, real, tiles_per_chunk);
    hipLaunchKernelGGL((k_brute_finish<MODE, SIGN>), dim3(vblocks), dim3(256), 0, st, g, plane, (const uint32_t*)acc, d_out, real, pz);
  });
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}
// ... and on the path ALL_PAIRS (algorithm 1): k_brute over the `packets` bricks of the launch order.
int launch_grid_brute(hipStream_t st, const DeviceMesh& mesh, const GridParams& g, int mode, const uint32_t* plane, float* d_out, int* d_err,
                      uint32_t packets, const PeerOut& pz) {
  for_grid_form(mode, plane != nullptr, [&](auto form) {
    launch_brute<true, decltype(form)::MODE, decltype(form)::SIGN>(st, mesh, g, nullptr, 0, plane, d_out, d_err, packets, pz);
  });
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}
// Generic queries, algorithm 1: every query against every triangle, in input order (None(Raycast) takes its +X ray against all triangles here).
int launch_query_brute(hipStream_t st, const DeviceMesh& mesh, const float* d_queries, uint32_t nq, int mode, int sign_src, float* d_out, int* d_err) {
  GridParams g{};
  const uint32_t packets = (nq + 63) / 64;
  if (mode == MODE_UNSIGNED && sign_src == SIGN_XRAY_ALL) launch_brute<false, MODE_UNSIGNED, SIGN_XRAY_ALL>(st, mesh, g, d_queries, nq, nullptr, d_out, d_err, packets);
  else for_query_form(mode, sign_src, [&](auto form) {
    launch_brute<false, decltype(form)::MODE, decltype(form)::SIGN>(st, mesh, g, d_queries, nq, nullptr, d_out, d_err, packets);
  });
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

// Small query sets take k_brute_split_q: queries x triangles <= 1.2e8, 6e7 with the three ray tests per pair (M2S_BRUTE_MAX overrides; 0:
// never).  Measured (tools/exp_small_queries.py, whole one-shot calls, all pairs / build + walk): 11 k triangles x 1 ... 1 000 queries
// 0.085 - 0.15 / 0.25 - 0.70 ms, x 10 000 0.47 (0.83 with rays) / 0.55 (0.66); 100 k triangles x 64 0.13 - 0.22 / 1.0 - 1.3 ms, x 1 000
// 0.46 (0.81) / 0.74 (0.94), x 10 000 3.2 (5.8) / 0.9 (1.0): 240 G pairs/s for the distance alone, 135 G with the rays.
bool query_is_tiny(size_t n_q, size_t n_tris, int algorithm, int sign_src) {
  if (algorithm != 0 || n_tris == 0 || n_q == 0 || sign_src == SIGN_XRAY_ALL) return false;
  const double limit = tuning().brute_max >= 0.0 ? tuning().brute_max : (sign_src == SIGN_RAYS3 ? 6.0e7 : 1.2e8);
  return (double)n_q * (double)n_tris <= limit;
}
int launch_query_brute_split(Arena& ws, hipStream_t st, const DeviceMesh& mesh, const float* d_queries, size_t n_q, int mode, int sign_src,
                             float* d_out, int* d_err) {
  const uint32_t nq = (uint32_t)n_q;
  uint32_t* acc = ws.take<uint32_t>(4 * n_q);
  if (!acc) { set_error("internal: query workspace too small"); return M2S_ERR_HIP_INTERNAL; }
  const uint32_t qblocks = (nq + 255u) / 256u, tiles = (mesh.n_tris + TILE - 1) / TILE;
  // ~4 blocks per CU over (query blocks x triangle chunks); a chunk is a whole number of 128-triangle tiles
  const uint32_t chunks = std::max(1u, std::min(tiles, (1024u + qblocks - 1) / qblocks));
  const uint32_t tiles_per_chunk = (tiles + chunks - 1) / chunks, ychunks = (tiles + tiles_per_chunk - 1) / tiles_per_chunk;
  const dim3 grid(qblocks, ychunks);
  hipLaunchKernelGGL(k_brute_q_init, dim3(qblocks), dim3(256), 0, st, acc, nq, mode == MODE_NORMAL_FOLD ? 0x7f800000u : 0u);
  for_query_form(mode, sign_src, [&](auto form) {
    constexpr int MODE = decltype(form)::MODE, SIGN = decltype(form)::SIGN;
    hipLaunchKernelGGL((k_brute_split_q<MODE, SIGN>), grid, dim3(256), 0, st, mesh, d_queries, nq, acc, d_err, tiles_per_chunk);
    hipLaunchKernelGGL((k_brute_finish_q<MODE, SIGN>), dim3(qblocks), dim3(256), 0, st, (const uint32_t*)acc, nq, d_out);
  });
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

// m2s_warmup: this unit's code object (see warm_distance; none of its kernels is on the list of those a first call uses).
__global__ void k_warm_brute() {}
void warm_brute(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_brute, dim3(1), dim3(64), 0, st);
}

}  // namespace m2s
