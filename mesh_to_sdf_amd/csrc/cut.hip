// cut.hip — the cut lists of a distance call (gfx950): k_cut walks the top of the tree once per block of packet bricks (grids, in one
// level or two) or per packet of sorted queries and leaves the pre-order ranges that k_packet (distance.hip) then walks instead of
// starting at the root.  The list format is in dist.hip.h.
#include <algorithm>

#include "common.h"
#include "geo.hip.h"
#include "tuning.h"
#include "walk.hip.h"
#include "dist.hip.h"
#include "cut_size.hip.h"

namespace m2s {

namespace {

// ---- k_cut: one wave per 4 x 4 x 4 bricks, lane = brick, one cut list per brick (see CutList) ---------------
// The 64 bricks of a wave are neighbours, so they visit nearly the same top of the tree: the wave walks it ONCE, like
// k_packet does (wave-uniform position, node records through scalar loads, a subtree left when no lane keeps it), one
// test per lane per node; a lane that has dropped or emitted a subtree sits out until the walk has left it (`resume`).
//
// What a brick may drop.  Brick: centre q, every voxel centre v = q + w with |w| <= r.  k_packet evaluates the brick's seed
// triangle T first, so voxel v ends with a minimum <= dist(v, T) <= |v - s|, s = the point of T closest to q, a = q - s,
// D = |a|, e = a / D.  Subtree X lies inside its convex disc-slab C_X; c = the point of C_X closest to q, L = |q - c|,
// n = (q - c) / L, and convexity gives dist(v, C_X) >= n . (v - c) = L + n . w.  X holds nothing within (or tied with) any
// voxel's minimum if   L + n . w > |a + w|   for all |w| <= r.  Two sufficient conditions, either drops X:
//   sphere     L - r > D + r                                                       (1-Lipschitz; the only test so far)
//   gradient   L - D > |n - e| r + r^2 / (2 D)          from |a + w| <= D + e . w + |w|^2 / (2 D)
// The sphere test wastes 2 r = 5 cells: far from the surface (D = 64 cells) it keeps every triangle of a cap of ~25
// cells radius, so the lists had to stay coarse and the packets walked the rest voxel by voxel — 64 lanes repeating
// nearly the same decision (84 % of the packets of 512^3 x blob-100k are farther than 16 cells from the surface and
// they are the expensive ones: 129 node tests at D >= 64 cells against 45 next to the surface).  The gradient test sees
// that all voxels of the brick look at X from (almost) the same direction as at their seed: its slack is
// |n - e| r ~ (lateral offset / D) r, a few tenths of a cell, so the lists can go down to subtrees of a few triangles.
// All margins are far above f32 rounding (relative 1e-4 on lengths, sqrt(2e-5) on |n - e|), always towards keeping.
//
// Earlier versions (512^3 x blob-100k / the 64-layer slab of an 8-GPU rank; lists per block of 2 x 2 x 2 bricks, sphere
// test): one lane per block, per-lane record fetches: 0.27 / 0.24 ms; eight lanes per block: 0.40 / 0.15 ms; one wave per
// eight blocks with scalar record loads: 0.22 / 0.07 ms.
// GRID = false (generic queries): "brick" = packet of sorted queries, lane = packet, 64 consecutive packets (neighbours in
// the Morton order) per wave; centre and radius from `centres` (k_qpacket_bounds), the seed from the lattice cell of the
// centre (as k_packet<false> does), `nbx` = the number of wave slots the packet walk was launched with.
// Two levels (round 6; grids only).  Of a fine wave's node visits on 512^3 x blob-100k 44 % fall on nodes larger than the wave's own block
// of 4 x 4 x 4 bricks (16 % on nodes larger than four blocks; 1024^3 x sheet-100k: 61 % / 29 %; counted, profiles/r06_kcut_visits.txt),
// and its 63 neighbours inside a 64^3-voxel region repeat them with the same outcome.  LEVEL 1 walks that top ONCE per region: lane =
// a block of 4 x 4 x 4 bricks (the same tests with the block's radius; witness triangle = the seed of the brick at the block's centre —
// any triangle bounds the final minimum from above), one wave per 4 x 4 x 4 blocks AND per one of CUTC_S subtrees of the tree's top
// (a single wave per region would be a chain of ~300 dependent visits on a launch of a few hundred waves: as long as what it saves),
// and leaves CUTC_S sub-lists of <= CUTC_MAX ranges per block.  LEVEL 2 is the fine walk started from its block's ranges instead of
// the root.  A subtree the coarse level drops holds nothing a voxel of the block can need, whatever the fine level's own seeds say,
// so the fine lists can only get shorter; the packets' results cannot change (parity suite, soaks).
// A lane condition as the wave's 64-bit mask, and this lane's bit of such a mask as a condition again: neither costs a vector instruction.
__device__ __forceinline__ unsigned long long wave_mask(bool lane_condition) { return __builtin_amdgcn_ballot_w64(lane_condition); }
__device__ __forceinline__ bool lane_of(unsigned long long mask) { return __builtin_amdgcn_inverse_ballot_w64(mask); }
template <bool GRID, int LEVEL = 0>
__global__ __launch_bounds__(64) void k_cut(DeviceMesh mesh, GridParams g, const uint32_t* __restrict__ seeds, uint32_t seed_shift,
                                            uint32_t seed_ny, uint32_t seed_nz, uint32_t nbx, uint32_t nby, uint32_t nbz,
                                            uint32_t* __restrict__ lists, float emit_near, float emit_far, uint32_t wave_cap,
                                            const float4* __restrict__ centres, const uint32_t* __restrict__ table,
                                            const GridParams* __restrict__ seed_lattice, uint32_t start_bits, const uint32_t* __restrict__ coarse = nullptr) {
  static_assert(GRID || LEVEL == 0, "the two-level form is the grid's");
  // LEVEL 1: the "bricks" of this launch are blocks of 4 x 4 x 4 packet bricks (nbx, nby, nbz count blocks), eight waves per 4 x 4 x 4 of them
  constexpr uint32_t UL = LEVEL == 1 ? 2u : 0u;               // log2 packet bricks per lane unit and axis
  constexpr uint32_t NMAX = LEVEL == 1 ? CUTC_MAX : CUT_MAX;  // ranges per list
  constexpr uint32_t OUT_WORDS = LEVEL == 1 ? CUTC_WORDS : CUT_WORDS;
  const uint32_t nsy = (nby + 3u) >> 2, nsz = (nbz + 3u) >> 2;
  const uint32_t sb = LEVEL == 1 ? blockIdx.x >> CUTC_S_LOG : blockIdx.x;   // 4 x 4 x 4 units
  const uint32_t sub = LEVEL == 1 ? blockIdx.x & (CUTC_S - 1u) : 0u;        // LEVEL 1: which subtree of the top
  const uint32_t sz = sb % nsz, sy = (sb / nsz) % nsy, sx = sb / (nsz * nsy);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t bk[3] = {4u * sx + (lane >> 4), 4u * sy + ((lane >> 2) & 3u), 4u * sz + (lane & 3u)};
  const uint32_t pk = blockIdx.x * 64u + lane;               // !GRID: this lane's packet
  bool in_grid = bk[0] < nbx && bk[1] < nby && bk[2] < nbz;
  float r = 0.0f, qq[3];
  if (GRID) {
    // first cell of the unit in the grid (a brick never straddles two chunks of an interleaved slab: capi.hip checks; a block
    // does not either where the coarse level is used: prepare_grid_walk)
    const uint32_t cell0[3] = {slab_x(g, bk[0] << (g.bl[0] + UL)), bk[1] << (g.bl[1] + UL), bk[2] << (g.bl[2] + UL)};
    for (int k = 0; k < 3; ++k) {
      const float hb = 0.5f * (float)((1u << (g.bl[k] + UL)) - 1u) * fabsf(g.size[k]);   // half extent between voxel centres
      r = __builtin_fmaf(hb, hb, r);
      qq[k] = g.first[k] + ((float)cell0[k] + 0.5f * (float)((1u << (g.bl[k] + UL)) - 1u)) * g.size[k];
    }
    r = sqrtf(r) * 1.0001f;
  } else {
    in_grid = pk < nbx && pk < table[0];
    const float4 c = centres[in_grid ? pk : 0u];
    qq[0] = c.x; qq[1] = c.y; qq[2] = c.z;
    r = c.w;                                                 // already rounded up; NaN / inf (non-finite queries): nothing is dropped
    if (!(r < 3.0e37f)) r = __builtin_inff();
  }
  const f3 q = mk3(qq[0], qq[1], qq[2]);
  const float scale = fmaxf(mesh_centre_scale(mesh), fmaxf(fabsf(q.x), fmaxf(fabsf(q.y), fabsf(q.z))) + r);
  // 16 x the packet walk's own slack, which is 4e-6 * vscale + 2.5e-6 with the scale of the VERTICES (common.h mesh_scale): the first
  // term is the larger one unless the vertices exceed the box centres and the unit by 0.625, as those of long triangles about the origin do
  const float vscale = fmaxf(mesh_scale(mesh), scale);
  const float abs_margin = fmaxf(6.4e-5f * scale + 4.0e-5f, 6.4e-5f * vscale);
  float R2 = -1.0f, R = 0.0f, D = 0.0f;                      // unit outside the grid: never keeps anything
  f3 e = mk3(0.0f, 0.0f, 0.0f);
  float grad_c0 = __builtin_inff(), grad_c1 = 0.0f;          // gradient test: drop if L * (1 - 1e-4) - grad_c0 > grad_c1 * |n - e|
  if (in_grid) {
    uint32_t sidx;
    if (!GRID) sidx = query_lattice_cell(*seed_lattice, q.x, q.y, q.z);
    else if (LEVEL == 1) {                                    // the brick at the block's centre (seed lattice: one point per brick)
      const uint32_t lx = bricks_along(g.xe - g.xb, g.bl[0]);
      const uint32_t b0 = min((bk[0] << 2) + 2u, lx - 1u), b1 = min((bk[1] << 2) + 2u, seed_ny - 1u), b2 = min((bk[2] << 2) + 2u, seed_nz - 1u);
      sidx = (b0 * seed_ny + b1) * seed_nz + b2;
    } else sidx = ((bk[0] >> seed_shift) * seed_ny + (bk[1] >> seed_shift)) * seed_nz + (bk[2] >> seed_shift);
    const uint32_t slot = min(seeds[sidx], mesh.n_tris - 1);
    const TriRec& t = mesh.tris[slot];
    const f3 a = mk3(t.ax, t.ay, t.az), bq = mk3(t.bx, t.by, t.bz), c = mk3(t.cx, t.cy, t.cz);
    const TriEdges ed = {mk3(t.abx, t.aby, t.abz), mk3(t.acx, t.acy, t.acz), mk3(t.bcx, t.bcy, t.bcz)};
    const f3 s = closest_point_triangle(q, a, bq, c, ed, t.cls);
    const f3 av = sub3(q, s);
    const float d2 = dot3(av, av);
    D = (d2 == d2) ? sqrtf(d2) : __builtin_inff();
    // sphere: the packet walk keeps a node while bound <= d * (1 + PRUNE_REL) + slack: stay well above that
    R = (D * 1.0001f + 2.0f * r) * 1.0003f + abs_margin;
    R2 = R * R;                                              // inf: nothing is dropped
    if (D > r && D < 3.0e37f) {                              // (valid for any D > 0; useless when r^2 / 2D is large)
      const float inv = 1.0f / D;
      e = mk3(av.x * inv, av.y * inv, av.z * inv);
      grad_c0 = D * 1.0003f + (r * r * 0.5f * inv) * 1.01f + abs_margin;
      grad_c1 = r * 1.001f;
    }
  }
  const float grad_c1sq = grad_c1 * grad_c1 * 1.000001f;     // the test compares squares (no root per node): rounded up
  const float emit_radius = fmaxf(emit_near * r, R * emit_far);

  constexpr uint32_t NB = (uint32_t)sizeof(NodeExt);
  uint32_t* out = lists + ((size_t)(in_grid ? (GRID ? (bk[0] * nby + bk[1]) * nbz + bk[2] : pk) : 0u)) * (LEVEL == 1 ? CUTC_S * CUTC_WORDS : OUT_WORDS)
                  + sub * CUTC_WORDS;
  const uint32_t cut_S = start_bits;   // cut_start_bits(mesh.n_nodes), resolved by the launch
  auto cut_word = [cut_S](uint32_t start, uint32_t stop) {   // records [start, stop) -> list word (see CUT_WORDS)
    return start | (cut_encode_len(stop - start, 27u - cut_S) << cut_S);
  };
  // The walk's own positions (off, end, the lanes' resume) are byte offsets, as the records' `skip` is; the ranges a lane collects
  // (last_start, last_end) are RECORD indices, divided once on the scalar unit where a range is emitted, so that a list word needs no
  // per-lane division by the record size.
  uint32_t n = 0, last_start = 0, last_end = 0, resume = 0;   // per lane
  uint32_t off = 0, end = mesh.n_nodes * NB, steps = 0;       // wave-uniform
  if (LEVEL == 1) {
    // this wave's subtree: CUTC_S_LOG levels down from the root, left or right by the bits of `sub`.  A leaf met on the way belongs to
    // the wave whose remaining bits are zero; the others have nothing to walk.
    for (uint32_t lv = 0; lv < CUTC_S_LOG && off < end; ++lv) {
      const NodeExt* nr = reinterpret_cast<const NodeExt*>(reinterpret_cast<const char*>(mesh.ext) + off);
      const uint32_t rest = sub & ((1u << (CUTC_S_LOG - lv)) - 1u);
      if (__builtin_amdgcn_readfirstlane(nr->tri) >= 0) { if (rest != 0u) end = off; break; }
      const uint32_t left = off + NB;
      const uint32_t right = __builtin_amdgcn_readfirstlane(reinterpret_cast<const NodeExt*>(reinterpret_cast<const char*>(mesh.ext) + left)->skip);
      const uint32_t skip = __builtin_amdgcn_readfirstlane(nr->skip);
      if ((sub >> (CUTC_S_LOG - 1u - lv)) & 1u) { off = right; end = skip; } else { off = left; end = right; }
    }
  }
  // LEVEL 2: the block's coarse record, lane = word; ranges are taken from it one by one
  uint32_t cw = 0, c_sub = 0, c_k = 0, c_cnt = 0;
  if (LEVEL == 2) {
    cw = coarse[(size_t)sb * (CUTC_S * CUTC_WORDS) + lane];
    off = end = 0;
    c_cnt = (uint32_t)__builtin_amdgcn_readlane((int)cw, 0);
  }
#ifdef M2S_STATS_BUILD
  // M2S_STATS: where a wave's node visits go — on nodes larger than the wave's own block of 4 x 4 x 4 bricks (what a coarser level
  // of lists could decide once for several waves) or below
  uint32_t st_visits = 0, st_above1 = 0, st_above4 = 0;
  const float st_block = (LEVEL == 1 ? 1.0f : 4.0f) * __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, r)));
#endif
  for (;;) {
    if (LEVEL == 2) {
      while (c_k >= c_cnt) {                                  // next non-empty sub-list
        if (++c_sub >= CUTC_S) break;
        c_k = 0;
        c_cnt = (uint32_t)__builtin_amdgcn_readlane((int)cw, (int)(c_sub * CUTC_WORDS));
      }
      if (c_sub >= CUTC_S) break;
      const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)cw, (int)(c_sub * CUTC_WORDS + 1u + c_k));
      ++c_k;
      const uint32_t first = w & ((1u << cut_S) - 1u);
      const uint32_t len = ((w >> cut_S) & ((1u << (27u - cut_S)) - 1u)) << (w >> 27);
      off = max(first * NB, off);                             // (a rounded-up range may reach into the next one: never walk back)
      end = min(first + len, mesh.n_nodes) * NB;
    }
  while (off < end) {
    off = __builtin_amdgcn_readfirstlane(off);
    ++steps;
    const NodeExt nr = *reinterpret_cast<const NodeExt*>(reinterpret_cast<const char*>(mesh.ext) + off);
#ifdef M2S_STATS_BUILD
    {
      const float ext = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, fmaxf(nr.R, nr.half))));
      ++st_visits;
      st_above1 += ext > st_block ? 1u : 0u;
      st_above4 += ext > 4.0f * st_block ? 1u : 0u;
    }
#endif
    // The lanes' conditions live as 64-bit wave masks in scalar registers from the compare that forms them (the ballot of ONE compare is
    // that compare's own result) and are combined there with AND / OR / ANDN2; a lane's state changes under the final mask (lane_of).
    // Kept as per-lane booleans they were turned into 0 / 1 values and back (v_cndmask + v_cmp) at every ballot of a combined
    // condition and in the loop's tail: some twenty vector instructions of every visit held no arithmetic of the brick.
    const unsigned long long active = wave_mask(off >= resume);   // bricks that have not dropped / emitted an ancestor
    // closest point of the disc-slab to q:  q - c = ax * n_s + lat * l / |l|   (common.h NodeExt, ext_dist2)
    const float vx = q.x - nr.cx, vy = q.y - nr.cy, vz = q.z - nr.cz;
    const float t = __builtin_fmaf(nr.nz, vz, __builtin_fmaf(nr.ny, vy, nr.nx * vx));
    const float v2 = __builtin_fmaf(vz, vz, __builtin_fmaf(vy, vy, vx * vx));
    const float l2 = fmaxf(__builtin_fmaf(-1.0e-6f, v2, __builtin_fmaf(-t, t, v2)), 0.0f);
    const float inv_ell = __builtin_amdgcn_rsqf(l2);                  // one transcendental for ell and 1 / ell (inf at l2 = 0: guarded below)
    const float ell = l2 > 0.0f ? l2 * inv_ell : 0.0f;
    const float lat = fmaxf(ell - nr.R, 0.0f);
    const float dt = t - nr.mid;
    const float ax = copysignf(fmaxf(fabsf(dt) - nr.half, 0.0f), dt);
    const float L2 = __builtin_fmaf(ax, ax, lat * lat);
    unsigned long long kept = active & wave_mask(!(L2 > R2));    // sphere test; NaN keeps the node
    if (kept == 0ull) { off = nr.skip; continue; }
    {
      // gradient test (lanes without it carry grad_c0 = inf: never dropped).  rcp / rsq instead of IEEE divisions: their
      // 1-ulp error is nothing beside the 2e-5 added under the root
      const float ne_s = __builtin_fmaf(nr.nz, e.z, __builtin_fmaf(nr.ny, e.y, nr.nx * e.x));            // n_s . e
      const float ve = __builtin_fmaf(vz, e.z, __builtin_fmaf(vy, e.y, vx * e.x));                       // (q - c0) . e
      const float le = ve - t * ne_s;                                                                    // l . e
      const float lat_dir = lat > 0.0f ? lat * inv_ell : 0.0f;       // lat > 0 means ell > R >= 0
      const float num = __builtin_fmaf(ax, ne_s, lat_dir * le);                                          // (q - c) . e
      const float inv_L = __builtin_amdgcn_rsqf(L2);
      const float cosne = fminf(num * inv_L, 1.0f);                                                      // n . e (NaN / inf if L == 0: kept)
      const float nme2 = fmaxf(2.0f - 2.0f * cosne, 0.0f) + 2.0e-5f;                                     // >= |n - e|^2
      const float A = __builtin_fmaf(L2 * inv_L, 0.9999f, -grad_c0);                                     // L (1 - 1e-4) - c0
      kept &= ~(wave_mask(A > 0.0f) & wave_mask(A * A > grad_c1sq * nme2));                              // drop if A > c1 |n - e|, without the root; false on NaN
    }
    if (kept == 0ull) { off = nr.skip; continue; }
    // Where many triangles are (nearly) equidistant — towards the medial axis, e.g. deep inside a round body — the brick-level
    // test keeps a large part of the tree however far it descends: past wave_cap visits (cut_params) the wave's bricks emit what
    // they meet next as it is and leave the rest to the packet's per-voxel tests (which are 200 times sharper there).
    // (a saturated list — NMAX ranges — only grows its last range over every gap from here on: nothing finer can be said)
    // The leaf mark and the cap are the wave's, the size test's left side too (cut_size.hip.h): one compare per lane each for the size
    // and the saturated list.
    const unsigned long long emit_all = ((nr.tri >= 0) | (steps >= wave_cap)) ? ~0ull : 0ull;
    const unsigned long long emitted = kept & (emit_all | wave_mask(cut_small_enough(nr.R, nr.half, emit_radius)) | wave_mask(n == NMAX));
    const unsigned long long open = kept & ~emitted;          // bricks that still have to look inside
    if (lane_of(emitted)) {
      // keep this subtree: the records [at, to).  Adjacent subtrees merge; past NMAX ranges the last one grows over the gap
      const uint32_t at = off / NB, to = nr.skip / NB;        // (wave-uniform: one multiply-high each on the scalar unit)
      if (n > 0 && (last_end == at || n == NMAX)) last_end = to;
      else {
        if (n > 0) out[n] = cut_word(last_start, last_end);
        ++n; last_start = at; last_end = to;
      }
    }
    if (lane_of(active & ~open)) resume = nr.skip;            // dropped or emitted: done with this subtree either way
    off = open != 0ull ? off + NB : nr.skip;
  }
    if (LEVEL != 2) break;
  }
#ifdef M2S_STATS_BUILD
  if (mesh.stats != nullptr && lane == 0u) {
    unsigned long long* sc = mesh.stats + (LEVEL == 1 ? 112 : 104);
    atomicAdd(&sc[0], 1ull);
    atomicAdd(&sc[1], (unsigned long long)st_visits);
    atomicAdd(&sc[2], (unsigned long long)st_above1);
    atomicAdd(&sc[3], (unsigned long long)st_above4);
    atomicMax(&sc[4], (unsigned long long)st_visits);
  }
#endif
  if (!in_grid) return;
  if (LEVEL == 1) {                                           // an empty sub-list is fine: the other subtrees hold what the block needs
    if (n > 0) out[n] = cut_word(last_start, last_end);
    out[0] = n;
    return;
  }
  if (n == 0) { n = 1; last_start = 0; last_end = mesh.n_nodes; }    // cannot happen with finite input; never walk nothing
  out[n] = cut_word(last_start, last_end);
  out[0] = n;
}

}  // namespace

// What k_cut is launched with, for grids and for queries.
struct CutParams { float emit_near, emit_far; uint32_t wave_cap; };   // emission radius of a list entry: emit_near brick radii next to the surface, emit_far of the distance far from it
static CutParams cut_params(uint32_t n_tris, const Tuning& tn) {
  // A wave that has visited wave_cap nodes lets its bricks emit whatever they meet next: the long union walks of the
  // regions with many near-ties (deep inside a round body) are the tail of the launch — on the 64-layer slab of an 8-GPU
  // rank, 4 waves per SIMD, they WERE its duration (0.39 -> 0.19 ms; 512^3: flat between 300 and 450, 200 costs the
  // packets 0.5 ms) — and what they still decide so deep in the tree the packets decide almost as cheaply.
  uint32_t depth = 1;
  while ((1ull << depth) < (unsigned long long)n_tris + 1ull) ++depth;
  // (emit_far 1/32: re-tuned at the end of round 3 (1/16 before): headline 9.19 -> 9.11 ms, 1024^3 x sheet-100k 92.95 -> 89.33 ms)
  // (k_cut once also counted the nodes each brick had opened and let a brick past a budget of 100 000 emit what it met.  A brick opens at
  // most one node per visit, so its count never exceeds the wave's visits, and the cap — at most 99 999 whatever M2S_CUT_WAVE_CAP or
  // M2S_CUT_COARSE_CAP asks for: tuning.cpp — is always met first: the term could never decide and is gone.)
  return {tn.cut_near, tn.cut_far, tn.cut_wave_cap ? tn.cut_wave_cap : std::max(120u, 20u * depth)};
}

// k_cut over the slab [g.xb, g.xe): one list of CUT_WORDS words per packet brick into `lists`, from the seed lattice the walk will use.
// `coarse` (cut_blocks(g, 2) x CUTC_S x CUTC_WORDS words) set: in two levels.
void launch_grid_cut(hipStream_t st, const DeviceMesh& mesh, const GridParams& g, const uint32_t* seed1, uint32_t sh1, uint32_t s1ny, uint32_t s1nz,
                     uint32_t* lists, uint32_t* coarse) {
  const Tuning& tn = tuning();
  const CutParams cp = cut_params(mesh.n_tris, tn);
  const BrickCounts bc = brick_counts(g);
  const uint32_t nbx = bc.nb[0], nby = bc.nb[1], nbz = bc.nb[2];
  const uint32_t cbx = bricks_along(nbx, 2), cby = bricks_along(nby, 2), cbz = bricks_along(nbz, 2);   // blocks of 4 x 4 x 4 bricks = fine waves
  const size_t waves = cut_blocks(g, 2);
  const uint32_t S = cut_start_bits(mesh.n_nodes);   // the list words' start field: once per call, for k_cut and (CutList) the walk
  if (coarse != nullptr) {
    const size_t groups = cut_blocks(g, 4);   // 4 x 4 x 4 blocks
    const uint32_t coarse_cap = tn.cut_coarse_cap ? tn.cut_coarse_cap : cp.wave_cap;
    hipLaunchKernelGGL((k_cut<true, 1>), dim3((unsigned)(groups * CUTC_S)), dim3(64), 0, st, mesh, g, seed1, sh1, s1ny, s1nz, cbx, cby, cbz, coarse, 1.0f, cp.emit_far,
                       coarse_cap, (const float4*)nullptr, (const uint32_t*)nullptr, (const GridParams*)nullptr, S, (const uint32_t*)nullptr);
    hipLaunchKernelGGL((k_cut<true, 2>), dim3((unsigned)waves), dim3(64), 0, st, mesh, g, seed1, sh1, s1ny, s1nz, nbx, nby, nbz, lists, cp.emit_near, cp.emit_far, cp.wave_cap,
                       (const float4*)nullptr, (const uint32_t*)nullptr, (const GridParams*)nullptr, S, (const uint32_t*)coarse);
  } else
  hipLaunchKernelGGL((k_cut<true, 0>), dim3((unsigned)waves), dim3(64), 0, st, mesh, g, seed1, sh1, s1ny, s1nz, nbx, nby, nbz, lists, cp.emit_near, cp.emit_far, cp.wave_cap,
                     (const float4*)nullptr, (const uint32_t*)nullptr, (const GridParams*)nullptr, S, (const uint32_t*)nullptr);
}

// k_cut<false> for the packets of a query set: one list per packet of the `launched` the walk will be launched with.
void launch_query_cut(hipStream_t st, const DeviceMesh& mesh, const uint32_t* seeds, uint32_t launched, uint32_t* lists, const float4* centres,
                      const uint32_t* table, const GridParams* d_lat) {
  GridParams g{};
  const CutParams cp = cut_params(mesh.n_tris, tuning());
  hipLaunchKernelGGL((k_cut<false, 0>), dim3((launched + 63) / 64), dim3(64), 0, st, mesh, g, seeds, 0u, 0u, 0u, launched, 1u, 1u, lists,
                     cp.emit_near, cp.emit_far, cp.wave_cap, centres, table, d_lat, cut_start_bits(mesh.n_nodes));
}

// Test hook (capi.hip m2s_debug_cut_code): the list word k_cut writes for the range [start, start + len) of a tree of n_nodes records,
// and the (first, end) records k_packet reads back from it.
void cut_word_roundtrip(uint32_t n_nodes, uint32_t start, uint32_t len, uint32_t* word, uint32_t* first, uint32_t* end) {
  const uint32_t S = cut_start_bits(n_nodes);
  const uint32_t w = start | (cut_encode_len(len, 27u - S) << S);
  *word = w;
  const uint32_t f = w & ((1u << S) - 1u);
  const uint32_t l = ((w >> S) & ((1u << (27u - S)) - 1u)) << (w >> 27);                // as k_packet decodes it
  *first = f;
  *end = std::min(f + l, n_nodes);
}

// Test hook (capi.hip m2s_debug_walk_consts): the start bits the host resolves for a tree of n_nodes records, as every launch gets them.
uint32_t cut_list_start_bits(uint32_t n_nodes) { return cut_list_for(n_nodes, nullptr, 0, 0, 0, 0, nullptr).start_bits; }

// m2s_warmup: this unit's code object, and the kernel functions of it that a first call uses (see warm_distance).
__global__ void k_warm_cut() {}
void warm_cut(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_cut, dim3(1), dim3(64), 0, st);
  const void* fns[] = {
      (const void*)k_cut<true, 0>,
      (const void*)k_cut<true, 1>,
      (const void*)k_cut<true, 2>,
      (const void*)k_cut<false, 0>};
  hipFuncAttributes attr;
  for (const void* f : fns) (void)hipFuncGetAttributes(&attr, f);
  (void)hipGetLastError();
}

}  // namespace m2s
