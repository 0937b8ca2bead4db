// dist.hip.h — what more than one translation unit of a distance call needs (distance.hip: the walks and their policy; seeds.hip,
// cut.hip, brute.hip, query_order.hip, peer_push.hip: the other stages): the cut-list format that k_cut writes and k_packet reads, the
// packet table and seed lattice of generic queries, the (mode, sign) dispatch and the brick counts of a slab.  As in walk.hip.h every
// definition lives in an anonymous namespace, so each unit keeps its own copy and inlines it as before.
#pragma once
#include "common.h"
#include "walk.hip.h"

namespace m2s {

namespace {

// ---- cut lists ------------------------------------------------------------------------------
// A third of a packet's node tests fall on nodes much larger than the packet (512^3 x blob-100k: 46 of 158 on nodes
// wider than 28 voxels, 69 on nodes wider than 14), and neighbouring packets repeat them with the same outcome.
// k_cut walks that top part of the tree ONCE per block of 2^log bricks per axis, against a bound that holds for every
// voxel of the block, and leaves at most CUT_MAX pre-order ranges [start, end) of NodeExt byte offsets per block: the
// subtrees that can still matter there.  k_packet then walks those ranges instead of starting at the root.
// A subtree is dropped only if   bound(block centre, subtree) - r_block  >  D + margins,   where D bounds the
// distance of every voxel of the block to the seed triangle of its own packet (which k_packet evaluates first):
// such a subtree cannot hold a triangle nearer than, or tied with, any voxel's final minimum.
#ifndef M2S_CUT_MAX
#define M2S_CUT_MAX 15   // 7: 12.0 ms, 15: 11.7 ms (512^3 x blob-100k)
#endif
// A list is ONE 64-byte record (round 2: 128 B of (start, end) byte offsets — 268 MB of lists for a 537 MB output):
//   word 0        number of ranges
//   word 1 + k    low S bits: start of range k (node record index), S = bits needed for the tree's node count; the other 32 - S bits:
//                 its length as a small float — 5 bits of exponent e, M = 27 - S bits of mantissa m: m << e records, the smallest
//                 such value that is >= the true length
// Lengths below 2^M records are exact and longer ones exceed the truth by less than 2^-(M-1) (100 k triangles: M = 9, 0.4 %; 1 M: M = 6,
// 3 %; the 2^25-triangle limit: M = 1): a superset of the subtrees, which a walk may always take, and one that hardly costs — a first
// form with 6-bit power-of-two lengths walked up to twice a long range: 14 % more node tests and 4.8 % more time on 512^3 x blob-1M
// (same box: 26.60 against 25.37 ms; the headline 8.40 against 8.43 ms).  A range that
// reaches into the next one is walked there twice (harmless: a minimum).  k_cut writes a word when its range closes, as before (ranges
// kept in LDS or scratch until the end and written as one record cost k_cut 20-35 %: five waves per SIMD, or scratch traffic).
__host__ __device__ __forceinline__ uint32_t cut_start_bits(uint32_t n_nodes) {
  uint32_t b = 1;
  while (b < 27u && (1u << b) < n_nodes) ++b;
  return b;
}
// length code: 5 bits of exponent e above M bits of mantissa, len = mantissa << e (explicit leading bit: no special case in the walk's
// decode, which runs once per range of every packet on the scalar unit)
__host__ __device__ __forceinline__ uint32_t cut_decode_len(uint32_t code, uint32_t M) { return (code & ((1u << M) - 1u)) << (code >> M); }
__host__ __device__ __forceinline__ uint32_t cut_encode_len(uint32_t len, uint32_t M) { // smallest representable value >= len (len >= 1)
  if (len < (1u << M)) return len;                                                      // exact, e = 0
  uint32_t e = (32u - (uint32_t)__builtin_clz(len)) - M;                                // len >> e lies in [2^(M-1), 2^M)
  uint32_t mant = (len + (1u << e) - 1u) >> e;
  if (mant == (1u << M)) { mant >>= 1; ++e; }
  return (e << M) | mant;
}
constexpr uint32_t CUT_MAX = M2S_CUT_MAX, CUT_WORDS = M2S_CUT_MAX + 1;
static_assert(M2S_CUT_MAX <= 15, "the range count has four bits");
struct CutList {
  const uint32_t* lists;   // CUT_WORDS words per block, nullptr: walk the whole tree
  uint32_t log, ny, nz;    // bricks per block per axis = 2^log; blocks along y and z
  uint32_t bx_off;         // grid: this launch covers a piece of the slab the seed lattice and the lists were built for,
                           // starting bx_off bricks into it along x (a multiple of 2^log)
  const float4* centres;   // generic queries: (centre, radius) of every packet's bounding box (k_qpacket_bounds); one list per packet
  uint32_t start_bits;     // S of the list words: cut_start_bits of the tree's node count, resolved once on the host (cut_list_for); 0: not set
};
// The lists of a tree of n_nodes records: the ONE place that fills a CutList (no lists: `lists` null, nothing is decoded).
inline CutList cut_list_for(uint32_t n_nodes, const uint32_t* lists, uint32_t log, uint32_t ny, uint32_t nz, uint32_t bx_off, const float4* centres) {
  return {lists, log, ny, nz, bx_off, centres, cut_start_bits(n_nodes)};
}
// The coarse level of two-level lists (cut.hip k_cut, LEVEL 1): CUTC_S sub-lists of at most CUTC_MAX ranges per block of 4 x 4 x 4 bricks.
constexpr uint32_t CUTC_S_LOG = 3, CUTC_S = 1u << CUTC_S_LOG, CUTC_WORDS = 8, CUTC_MAX = CUTC_WORDS - 1;   // 64 words = 256 B per block
static_assert(CUTC_S * CUTC_WORDS == 64, "a fine wave fetches its block's coarse record with one load, lane = word");

// Generic queries: the sorted queries [first, first + cnt) of packet k (table of launch_query_distance / k_qcells).
__device__ __forceinline__ bool query_packet_range(const uint32_t* __restrict__ table, uint32_t packet, uint32_t n_q,
                                                   uint32_t* first, uint32_t* cnt) {
  uint32_t f = packet * 64u, c = 64u;
  if (table != nullptr) {
    const uint32_t count = table[0];
    if (packet >= count) return false;
    if (table[1] == 0u) {
      f = table[2u + packet];
      c = (packet + 1u < count ? table[3u + packet] : n_q) - f;
    }
  }
  if (f >= n_q) return false;
  *first = f;
  *cnt = min(c, n_q - f);
  return true;
}
// Cell of the generic path's seed lattice that holds x (k_qlattice).
__device__ __forceinline__ uint32_t query_lattice_coord(const GridParams& L, int k, float q) {
  float f = (q - L.first[k]) / L.size[k] + 0.5f;
  f = (f == f) ? fminf(fmaxf(f, 0.0f), (float)(L.n[k] - 1)) : 0.0f;
  return min((uint32_t)f, L.n[k] - 1);
}
__device__ __forceinline__ uint32_t query_lattice_cell(const GridParams& L, float x, float y, float z) {
  return (query_lattice_coord(L, 0, x) * L.n[1] + query_lattice_coord(L, 1, y)) * L.n[2] + query_lattice_coord(L, 2, z);
}
// The same cell for a point that is the same in every lane, its index formed on the scalar unit.  (Formed on the vector unit the
// multiply-adds are 64-bit ones whose unused upper half the compiler pairs with any register at hand — in k_packet the one the list
// word is being loaded into, which put the wait for that load in front of the seed's loads.)
__device__ __forceinline__ uint32_t query_lattice_cell_uniform(const GridParams& L, float x, float y, float z) {
  const uint32_t cx = __builtin_amdgcn_readfirstlane(query_lattice_coord(L, 0, x)), cy = __builtin_amdgcn_readfirstlane(query_lattice_coord(L, 1, y)),
                 cz = __builtin_amdgcn_readfirstlane(query_lattice_coord(L, 2, z));
  return (cx * L.n[1] + cy) * L.n[2] + cz;
}
constexpr uint32_t QL = 64;   // generic queries: QL^3 cells of the seed lattice over the query bounding box (query_order.hip k_qlattice)

// The (mode, sign) of a call as compile-time constants for a generic lambda: f(WalkForm<MODE, SIGN>{}).  The grid walks exist in three forms,
// the query walks in four — every kernel of distance.hip and brute.hip that takes <MODE, SIGN> is instantiated for these and no others (launch_brute<false>
// alone has a fifth, SIGN_XRAY_ALL: launch_query_brute).  The Normal fold and the nearest normal carry their own sign: no planes, no rays.
template <int M, int S>
struct WalkForm { static constexpr int MODE = M, SIGN = S; };
template <class F>
void for_grid_form(int mode, bool planes, F&& f) {
  if (mode == MODE_UNSIGNED && planes) f(WalkForm<MODE_UNSIGNED, SIGN_GRID_PLANE>{});
  else if (mode == MODE_UNSIGNED) f(WalkForm<MODE_UNSIGNED, SIGN_NONE>{});
  else f(WalkForm<MODE_NORMAL_FOLD, SIGN_NONE>{});
}
template <class F>
void for_query_form(int mode, int sign_src, F&& f) {
  if (mode == MODE_UNSIGNED && sign_src == SIGN_RAYS3) f(WalkForm<MODE_UNSIGNED, SIGN_RAYS3>{});
  else if (mode == MODE_UNSIGNED) f(WalkForm<MODE_UNSIGNED, SIGN_NONE>{});
  else if (mode == MODE_NORMAL_FOLD) f(WalkForm<MODE_NORMAL_FOLD, SIGN_NONE>{});
  else f(WalkForm<MODE_NEAREST_NORMAL, SIGN_NONE>{});
}

// Packet bricks of the slab [g.xb, g.xe) per axis and in all: the real ones, those of the whole grid (all g.n[0] layers; the crossovers
// that must not depend on how a caller cuts the grid into slabs count these) and the launch's — padded to whole super-bricks.
struct BrickCounts { uint32_t nb[3]; uint64_t real, grid; uint32_t padded; };
static bool slab_is_empty(const GridParams& g) { return g.xe <= g.xb || g.n[1] == 0 || g.n[2] == 0; }
BrickCounts brick_counts(const GridParams& g) {
  BrickCounts c;
  c.nb[0] = bricks_along(g.xe - g.xb, g.bl[0]), c.nb[1] = bricks_along(g.n[1], g.bl[1]), c.nb[2] = bricks_along(g.n[2], g.bl[2]);
  c.real = (uint64_t)c.nb[0] * c.nb[1] * c.nb[2];
  c.grid = (uint64_t)bricks_along(g.n[0], g.bl[0]) * c.nb[1] * c.nb[2];
  const uint32_t xl = super_brick_xlog(c.nb[0], g.xl_cap);
  c.padded = ((c.nb[0] + (1u << xl) - 1u) >> xl) * ((c.nb[1] + 7) >> 3) * ((c.nb[2] + 7) >> 3) * (64u << xl);
  return c;
}
static size_t cut_blocks(const GridParams& g, uint32_t log) {
  const BrickCounts bc = brick_counts(g);
  return (size_t)bricks_along(bc.nb[0], log) * bricks_along(bc.nb[1], log) * bricks_along(bc.nb[2], log);
}

}  // namespace

}  // namespace m2s
