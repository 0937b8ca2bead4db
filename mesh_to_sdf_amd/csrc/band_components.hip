// band_components.hip — m2s_band_components / m2s_band_select: the connected components of a resident band's active cells (labels in list
// order, and per component its first cell, cell count, negative-cell count and bounding box), and a band with some components erased,
// gfx950.  The contract is include/m2s.h's (to the bit); tests/band_components_model.py restates it in numpy.  Nothing sized per grid
// point exists: the labelling works on 4 bytes per active cell, the selection on the index words plus the kept cells.
//
// m2s_band_components is a lock-free union-find over the list places ("ranks") r of the active cells, with parent[r] <= r throughout.
//   k_cc_init     parent[r] = r.
//   k_cc_hook     band_walk.hip.h's walk: lane t owns bit t of a word and knows (i, j, k).  For each active cell it looks up the ranks of
//                 the backward half of its stencil (3, 9 or 13 neighbours with a smaller L; mask word, word_off, popcount below, as
//                 band_filter.hip's bf_slot; a step off the grid finds nothing) and unites the cell with each active one: find both
//                 roots, hook the larger under the smaller by a compare-and-swap on parent[larger], retry from the new roots on failure.
//                 A find strictly descends, so it ends; a failed swap means another lane hooked that root.  A component's root is
//                 therefore its smallest rank whatever the order of execution, which is what makes the result deterministic.
//                 Every edge is united, also those that three others imply (L ~ L - 1, M ~ M - 1, L - 1 ~ M - 1): leaving them out was
//                 built, measured slower and taken out again.
//                 parent is read and written at agent scope: a stale value is an older ancestor, never a wrong one, and the
//                 compare-and-swap decides.  Finds halve their paths: they write an ancestor over a non-root, which stays a non-root.
//   k_cc_flatten  parent[r] = find(r), and per tile of 4096 ranks the number of roots.
//   k_scan_tiles  scan.hip.h's scan of the tile sums; the total is the component count, read by the host.
//   k_cc_number   each root's number = the roots before it: ranks ascend with L, so this is the raster numbering.
//   k_cc_label    the walk again, for (i, j, k): labels, and the statistics by 64-bit atomic adds and 32-bit atomic min / max.  A wave
//                 keeps per-lane partial statistics while the words it takes carry one label and flushes them (a wave reduction, eight
//                 atomics) when the label changes; a word with several labels falls back to atomics per lane.
// m2s_band_select is two walks in the shape of band_csg.hip.
//   k_sel_mask    the result's mask word (the kept cells), its sign word and the unit counts.  A word with inactive-inside bits runs the
//                 row search of the header: lane t looks in its own word first, then in the following / preceding words up to its row's
//                 end (at most nz / 64 + 1 word loads per direction), and asks whether the nearest active cell on each side is kept.
//                 A word with no active cell at all (a solid's interior; rows of 64 points or more) is searched once, by the lane
//                 that loaded it, 64 words at a time per wave: its points share their nearest cells.
//   k_scan_tiles  the group sums; the total is the result's cell count.
//   k_sel_emit    the result's word_off, and the kept values moved to their places.
// All stores are plain vector stores or vector atomics; the ballot loops are wave-uniform; every other loop is bounded by the
// invariant parent[r] <= r or by a row's length.
#include "../../include/m2s.h"
#include "band_handle.h"
#include "band_walk.hip.h"
#include "capi_internal.h"
#include "common.h"
#include "scan.hip.h"

#include <algorithm>
#include <cstring>

namespace m2s {
namespace {

constexpr int kCcScanThreads = 1024;                        // the one workgroup that scans the sums
constexpr int kSelGroup = 16;                               // units per scanned sum, as band_csg.hip
constexpr uint32_t kCcNone = 0xffffffffu;

__device__ __forceinline__ uint32_t cc_load(const uint32_t* parent, uint32_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cc_store(uint32_t* parent, uint32_t x, uint32_t v) {
  __hip_atomic_store(parent + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x's tree as far as this lane can see.  Every step goes to a smaller rank.  HALVE: x's parent becomes its grandparent.
template <bool HALVE>
__device__ __forceinline__ uint32_t cc_find(uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = cc_load(parent, x);
    if (p >= x) return x;   // p == x: a root (p > x never happens; it would end the descent too)
    const uint32_t gp = cc_load(parent, p);
    if (gp >= p) return p;
    if (HALVE) cc_store(parent, x, gp);
    x = gp;
  }
}

__device__ __forceinline__ void cc_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = cc_find<true>(parent, a);
    b = cc_find<true>(parent, b);
    if (a == b) return;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    a = old;   // hi was hooked by another lane meanwhile: below hi, so the retry descends
    b = lo;
  }
}

// The rank of the grid point M (inside the grid) if it is active, else kCcNone.
__device__ __forceinline__ uint32_t cc_rank(const BandDev& X, uint64_t M) {
  const uint64_t w = M >> 6;
  const int b = (int)(M & 63);
  const uint64_t m = X.mask[w];
  if (!((m >> b) & 1ull)) return kCcNone;
  const uint64_t r = X.word_off[w] + (uint64_t)__popcll(m & walk_below(b));
  return r < X.n ? (uint32_t)r : kCcNone;
}

__global__ void __launch_bounds__(256) k_cc_init(uint32_t* __restrict__ parent, uint64_t n) {
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (uint64_t)gridDim.x * 256) parent[r] = (uint32_t)r;
}

// AXES: the axes a step may differ on: 1, 2 or 3 for connectivity 6, 18 or 26.
template <int AXES>
__global__ void __launch_bounds__(kWalkThreads) k_cc_hook(BandDev X, WalkGrid g, uint32_t* parent) {
  WALK_UNIT_HEAD(kWalkSteps, g.n_words)
  for (int step = 0; step < kWalkSteps; ++step) {
    WALK_STEP_HEAD(g.n_words)
    const uint64_t m = in_range ? X.mask[w] : 0;
    const uint64_t wo = m ? X.word_off[w] : 0;
    WalkIjk base{0, 0, 0};
    if (m) base = walk_base(w << 6, g);
    uint64_t todo = __ballot(m != 0);
    while (todo) {   // wave-uniform
      const int j = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const uint64_t mj = walk_lane(m, j), woj = walk_lane(wo, j);
      const WalkIjk p = walk_step(walk_bcast(base, j), (uint32_t)lane, g);
      const uint64_t L = ((wb + (uint64_t)j) << 6) + (uint64_t)lane;
      const uint64_t r = woj + (uint64_t)__popcll(mj & walk_below(lane));
      if (((mj >> lane) & 1ull) && r < X.n) {   // an active point is inside the grid
#pragma unroll
        for (int di = -1; di <= 0; ++di)
#pragma unroll
          for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
            for (int dk = -1; dk <= 1; ++dk) {
              const bool backward = di < 0 || (di == 0 && (dj < 0 || (dj == 0 && dk < 0)));
              if (!backward || (di != 0) + (dj != 0) + (dk != 0) > AXES) continue;   // decided when compiled
              const bool on = (di == 0 || p.i > 0) && (dj < 0 ? p.j > 0 : (dj > 0 ? p.j + 1 < g.ny : true)) &&
                              (dk < 0 ? p.k > 0 : (dk > 0 ? p.k + 1 < g.nz : true));
              if (!on) continue;
              const uint64_t M = (uint64_t)((int64_t)L + di * (int64_t)g.si + dj * (int64_t)g.sj + dk);
              const uint32_t q = cc_rank(X, M);
              if (q != kCcNone) cc_unite(parent, (uint32_t)r, q);
            }
      }
    }
  }
}

// parent[r] = its root, and the roots of each tile of kScanTile ranks.
__global__ void __launch_bounds__(kTileThreads) k_cc_flatten(uint32_t* parent, uint64_t n, uint64_t* __restrict__ tile_sum) {
  uint64_t s = 0, all;
#pragma unroll 4
  for (int k = 0; k < kScanItems; ++k) {
    const uint64_t r = (uint64_t)blockIdx.x * kScanTile + (uint64_t)k * kTileThreads + threadIdx.x;
    if (r < n) {
      const uint32_t root = cc_find<false>(parent, (uint32_t)r);
      if (root != (uint32_t)r) cc_store(parent, (uint32_t)r, root);
      else ++s;
    }
  }
  (void)block_exclusive_scan<kTileThreads>(s, &all);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
}

// labels[root] = the roots before it.  tile_off: the scanned tile sums.
__global__ void __launch_bounds__(kTileThreads) k_cc_number(const uint32_t* __restrict__ parent, uint64_t n, const uint64_t* __restrict__ tile_off,
                                                          uint32_t* __restrict__ labels) {
  const uint64_t first = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems;
  uint32_t roots = 0;
  uint64_t s = 0, all;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    const uint64_t r = first + k;
    if (r < n && parent[r] == (uint32_t)r) {
      roots |= 1u << k;
      ++s;
    }
  }
  uint64_t run = tile_off[blockIdx.x] + block_exclusive_scan<kTileThreads>(s, &all);
#pragma unroll
  for (int k = 0; k < kScanItems; ++k)
    if ((roots >> k) & 1u) labels[first + k] = (uint32_t)run++;
}

__global__ void __launch_bounds__(256) k_cc_clear(m2s_band_component* __restrict__ comps, uint64_t count) {
  for (uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x; c < count; c += (uint64_t)gridDim.x * 256) {
    m2s_band_component x;
    x.first_cell = x.n_cells = x.n_negative = 0;
    x.lo[0] = x.lo[1] = x.lo[2] = 0xffffffffu;
    x.hi[0] = x.hi[1] = x.hi[2] = 0;
    comps[c] = x;
  }
}

// A wave's partial statistics of the label `cur`: per lane until they are flushed.
struct CcStats {
  uint32_t cnt, neg, lo[3], hi[3];
  __device__ __forceinline__ void reset() {
    cnt = neg = 0;
    lo[0] = lo[1] = lo[2] = 0xffffffffu;
    hi[0] = hi[1] = hi[2] = 0;
  }
  __device__ __forceinline__ void add(const WalkIjk& p, bool negative) {
    const uint32_t c[3] = {(uint32_t)p.i, (uint32_t)p.j, (uint32_t)p.k};   // a grid has fewer than 2^36 points: an axis fits 32 bits
    ++cnt;
    neg += negative ? 1u : 0u;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = c[a] < lo[a] ? c[a] : lo[a];
      hi[a] = c[a] > hi[a] ? c[a] : hi[a];
    }
  }
};
__device__ __forceinline__ void cc_publish(m2s_band_component* c, uint32_t cnt, uint32_t neg, const uint32_t (&lo)[3], const uint32_t (&hi)[3]) {
  atomicAdd((unsigned long long*)&c->n_cells, (unsigned long long)cnt);
  if (neg) atomicAdd((unsigned long long*)&c->n_negative, (unsigned long long)neg);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    atomicMin(&c->lo[a], lo[a]);
    atomicMax(&c->hi[a], hi[a]);
  }
}
// Every lane takes part.  cur: wave-uniform.
__device__ __forceinline__ void cc_flush(m2s_band_component* comps, uint32_t cur, CcStats& s, int lane) {
  if (cur != kCcNone) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s.cnt += __shfl_xor(s.cnt, o, 64);
      s.neg += __shfl_xor(s.neg, o, 64);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const uint32_t l = __shfl_xor(s.lo[a], o, 64), h = __shfl_xor(s.hi[a], o, 64);
        s.lo[a] = l < s.lo[a] ? l : s.lo[a];
        s.hi[a] = h > s.hi[a] ? h : s.hi[a];
      }
    }
    if (lane == 0 && s.cnt) cc_publish(comps + cur, s.cnt, s.neg, s.lo, s.hi);
  }
  s.reset();
}

// labels[r] = the number of r's root (k_cc_number wrote the roots'), and, with comps, the statistics.  count: the components there are.
__global__ void __launch_bounds__(kWalkThreads) k_cc_label(BandDev X, WalkGrid g, const uint32_t* __restrict__ parent, uint32_t* labels,
                                                         m2s_band_component* comps, uint64_t count) {
  WALK_UNIT_HEAD(kWalkSteps, g.n_words)
  uint32_t cur = kCcNone;
  CcStats acc;
  acc.reset();
  for (int step = 0; step < kWalkSteps; ++step) {
    WALK_STEP_HEAD(g.n_words)
    const uint64_t m = in_range ? X.mask[w] : 0;
    const uint64_t wo = m ? X.word_off[w] : 0;
    WalkIjk base{0, 0, 0};
    if (m) base = walk_base(w << 6, g);
    uint64_t todo = __ballot(m != 0);
    while (todo) {   // wave-uniform
      const int j = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const uint64_t mj = walk_lane(m, j), woj = walk_lane(wo, j);
      const WalkIjk p = walk_step(walk_bcast(base, j), (uint32_t)lane, g);
      const uint64_t L = ((wb + (uint64_t)j) << 6) + (uint64_t)lane;
      const uint64_t r = woj + (uint64_t)__popcll(mj & walk_below(lane));
      bool act = ((mj >> lane) & 1ull) && r < X.n;
      uint32_t lab = kCcNone;
      bool negative = false;
      if (act) {
        const uint32_t root = parent[r];
        lab = labels[root <= (uint32_t)r ? root : (uint32_t)r];
        if (root != (uint32_t)r) labels[r] = lab;
        else if (comps && lab < count) comps[lab].first_cell = L;   // the root is its component's smallest L
        negative = X.dist[r] < 0.0f;
        act = lab < count;   // always, when the index is sound
      }
      if (!comps) continue;   // wave-uniform
      const uint64_t am = __ballot(act);
      if (!am) continue;
      const uint32_t lab0 = (uint32_t)__builtin_amdgcn_readlane((int)lab, __ffsll((unsigned long long)am) - 1);
      if (__ballot(act && lab != lab0) == 0) {   // one label in the word: the usual case
        if (lab0 != cur) {
          cc_flush(comps, cur, acc, lane);
          cur = lab0;
        }
        if (act) acc.add(p, negative);
      } else if (act) {
        CcStats one;
        one.reset();
        one.add(p, negative);
        cc_publish(comps + lab, one.cnt, one.neg, one.lo, one.hi);
      }
    }
  }
  if (comps) cc_flush(comps, cur, acc, lane);
}

// ---- m2s_band_select ----

__device__ __forceinline__ bool sel_keep(const uint32_t* __restrict__ labels, const uint8_t* __restrict__ keep, uint64_t n_keep, uint64_t r) {
  const uint32_t lab = labels[r];
  return (uint64_t)lab < n_keep && keep[lab] != 0;
}
// Whether the active bit b of word w2 (mask m2) of X is kept.
__device__ __forceinline__ bool sel_keep_at(const BandDev& X, const uint32_t* __restrict__ labels, const uint8_t* __restrict__ keep, uint64_t n_keep,
                                            uint64_t w2, uint64_t m2, int b) {
  const uint64_t at = X.word_off[w2] + (uint64_t)__popcll(m2 & walk_below(b));
  return at < X.n && sel_keep(labels, keep, n_keep, at);
}
// The bits 0 .. b of a word.
__device__ __forceinline__ uint64_t sel_upto(uint64_t b) { return ((1ull << b) << 1) - 1ull; }

struct SelArgs {
  const uint32_t* __restrict__ labels;
  const uint8_t* __restrict__ keep;
  uint64_t n_keep;
};
// The nearest active cell of a row beyond word w: in the words w + 1 .. w_last (L1: the row's last point), or w - 1 .. w_first (L0: its
// first).  At most nz / 64 + 1 word loads.  -> 0: none, 1: it is kept, 2: it is dropped.
__device__ __forceinline__ int sel_search_up(const BandDev& X, const SelArgs& a, uint64_t w, uint64_t w_last, uint64_t L1) {
  while (w < w_last) {
    ++w;
    const uint64_t m2 = X.mask[w];
    const uint64_t cand = w == w_last ? (m2 & sel_upto(L1 & 63)) : m2;
    if (cand) return sel_keep_at(X, a.labels, a.keep, a.n_keep, w, m2, __ffsll((unsigned long long)cand) - 1) ? 1 : 2;
  }
  return 0;
}
__device__ __forceinline__ int sel_search_down(const BandDev& X, const SelArgs& a, uint64_t w, uint64_t w_first, uint64_t L0) {
  while (w > w_first) {
    --w;
    const uint64_t m2 = X.mask[w];
    const uint64_t cand = w == w_first ? (m2 & ~walk_below((int)(L0 & 63))) : m2;
    if (cand) return sel_keep_at(X, a.labels, a.keep, a.n_keep, w, m2, 63 - __clzll((long long)cand)) ? 1 : 2;
  }
  return 0;
}
// The rule: cleared iff a side has an active cell and no side's nearest one is kept.
__device__ __forceinline__ bool sel_clear(int up, int down) { return (up | down) != 0 && up != 1 && down != 1; }

// A word with no active cell whose rows hold 64 points or more, by the lane that loaded it: the points of a row in it share their
// nearest cells, and the word holds the end of one row and the start of the next at most.  -> the inactive-inside bits to clear.
__device__ __forceinline__ uint64_t sel_clear_word(const BandDev& X, const SelArgs& a, const WalkGrid& g, uint64_t w, uint64_t loose) {
  const WalkIjk b = walk_base(w << 6, g);
  const uint64_t L0 = (w << 6) - b.k, L1 = L0 + g.nz - 1;
  const uint64_t w_last = L1 >> 6;
  const uint64_t first = w == w_last ? sel_upto(L1 & 63) : ~0ull;   // the bits of the row the word starts in
  uint64_t clear = 0;
  if (loose & first) {
    const int up = sel_search_up(X, a, w, w_last, L1), down = sel_search_down(X, a, w, L0 >> 6, L0);
    if (sel_clear(up, down)) clear |= loose & first;
  }
  if (loose & ~first) {   // the next row starts in this word: nothing below, and it reaches beyond the word
    const uint64_t N1 = L1 + g.nz;
    if (sel_clear(sel_search_up(X, a, w, N1 >> 6, N1), 0)) clear |= loose & ~first;
  }
  return clear;
}

// counters[0] += the inactive-inside points cleared.
__global__ void __launch_bounds__(kWalkThreads) k_sel_mask(BandDev X, WalkGrid g, SelArgs a, uint64_t* __restrict__ out_mask,
                                                         uint64_t* __restrict__ out_inside, uint32_t* __restrict__ unit_cnt,
                                                         uint64_t* __restrict__ group_sum, uint64_t* __restrict__ counters) {
  WALK_UNIT_HEAD(kWalkSteps, g.n_words)
  uint64_t cnt = 0, n_cleared = 0;
  for (int step = 0; step < kWalkSteps; ++step) {
    WALK_STEP_HEAD(g.n_words)
    const uint64_t m = in_range ? X.mask[w] : 0;
    const uint64_t in = in_range && X.inside ? X.inside[w] : 0;
    const uint64_t wo = m ? X.word_off[w] : 0;
    uint64_t loose = in & ~m & walk_valid(w, in_range, g.total);   // inactive and inside
    uint64_t rm = 0, rs = loose;
    if (loose && !m && g.nz >= 64) {   // the solid's interior: one lane per word
      const uint64_t cleared = sel_clear_word(X, a, g, w, loose);
      rs = loose & ~cleared;
      n_cleared += (uint64_t)__popcll(cleared);
      loose = 0;
    }
    WalkIjk base{0, 0, 0};
    if (loose) base = walk_base(w << 6, g);
    uint64_t todo = __ballot((m | loose) != 0);
    while (todo) {   // wave-uniform
      const int j = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const uint64_t mj = walk_lane(m, j), woj = walk_lane(wo, j), loosej = walk_lane(loose, j);
      const uint64_t W = wb + (uint64_t)j;
      bool kept = false, negative = false;
      if ((mj >> lane) & 1ull) {
        const uint64_t r = woj + (uint64_t)__popcll(mj & walk_below(lane));
        if (r < X.n) {
          kept = sel_keep(a.labels, a.keep, a.n_keep, r);
          negative = X.dist[r] < 0.0f;
        }
      }
      const uint64_t km = __ballot(kept), sm = __ballot(kept && negative);
      uint64_t cleared = 0;
      if (loosej) {   // wave-uniform: lane t owns bit t, looks in its own word first and then along its row
        bool clear = false;
        if ((loosej >> lane) & 1ull) {
          const WalkIjk p = walk_step(walk_bcast(base, j), (uint32_t)lane, g);
          const uint64_t L = (W << 6) + (uint64_t)lane;
          const uint64_t L0 = L - p.k, L1 = L0 + g.nz - 1;   // the row's first and last point
          const uint64_t w_first = L0 >> 6, w_last = L1 >> 6;
          int up, down;
          uint64_t cand = lane == 63 ? 0 : (mj & ~sel_upto((uint64_t)lane));
          if (W == w_last) cand &= sel_upto(L1 & 63);
          if (cand) up = ((km >> (__ffsll((unsigned long long)cand) - 1)) & 1ull) ? 1 : 2;
          else up = sel_search_up(X, a, W, w_last, L1);
          cand = mj & walk_below(lane);
          if (W == w_first) cand &= ~walk_below((int)(L0 & 63));
          if (cand) down = ((km >> (63 - __clzll((long long)cand))) & 1ull) ? 1 : 2;
          else down = sel_search_down(X, a, W, w_first, L0);
          clear = sel_clear(up, down);
        }
        cleared = __ballot(clear);
      }
      if (lane == j) {
        rm = km;
        rs = sm | (loosej & ~cleared);
        n_cleared += (uint64_t)__popcll(cleared);
      }
    }
    if (in_range) {
      out_mask[w] = rm;
      out_inside[w] = rs;
    }
    cnt += (uint64_t)__popcll(rm);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_cleared += __shfl_xor(n_cleared, o, 64);
  if (lane == 0 && n_cleared) atomicAdd((unsigned long long*)counters, (unsigned long long)n_cleared);
  walk_publish<kSelGroup>(cnt, lane, unit, unit_cnt, group_sum);
}

// group_base: the scanned group sums.  cap: the floats out_dist holds.
__global__ void __launch_bounds__(kWalkThreads) k_sel_emit(BandDev X, uint64_t n_words, const uint64_t* __restrict__ out_mask,
                                                         const uint32_t* __restrict__ unit_cnt, const uint64_t* __restrict__ group_base,
                                                         uint64_t* __restrict__ out_word_off, float* __restrict__ out_dist, uint64_t cap) {
  WALK_UNIT_HEAD(kWalkSteps, n_words)
  uint64_t base = walk_unit_base<kSelGroup>(lane, unit, unit_cnt, group_base);
  for (int step = 0; step < kWalkSteps; ++step) {
    WALK_STEP_HEAD(n_words)
    const uint64_t rm = in_range ? out_mask[w] : 0;
    const uint64_t off = walk_word_off((uint64_t)__popcll(rm), lane, base);
    if (in_range) out_word_off[w] = off;
    const uint64_t m = rm ? X.mask[w] : 0;
    const uint64_t wo = rm ? X.word_off[w] : 0;
    uint64_t todo = __ballot(rm != 0);
    while (todo) {   // wave-uniform
      const int j = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const uint64_t rmj = walk_lane(rm, j), offj = walk_lane(off, j), mj = walk_lane(m, j), woj = walk_lane(wo, j);
      const uint64_t pos = offj + (uint64_t)__popcll(rmj & walk_below(lane));
      if (((rmj >> lane) & 1ull) && pos < cap) out_dist[pos] = X.dist[walk_rank(mj, woj, lane, X.n)];
    }
  }
}

int bad_connectivity(int c) { return c != M2S_CONNECT_6 && c != M2S_CONNECT_18 && c != M2S_CONNECT_26; }

}  // namespace

// m2s_warmup: the first launch of a kernel of this translation unit makes the runtime load its code object (all its kernels).
__global__ void k_warm_band_components() {}
void warm_band_components(hipStream_t st) { hipLaunchKernelGGL(k_warm_band_components, dim3(1), dim3(64), 0, st); }

}  // namespace m2s

using namespace m2s;

extern "C" {

int m2s_band_components(const m2s_band* band, const m2s_band_components_opts* copts, const m2s_opts* opts, uint32_t* labels_out,
                        m2s_band_component* components_out, uint64_t capacity, uint64_t* n_components_out) {
  clear_error();
  if (!band) return fail(M2S_ERR_BAD_ARG, "band is NULL");
  if (!n_components_out) return fail(M2S_ERR_BAD_ARG, "n_components_out is NULL");
  if (copts && copts->struct_size != sizeof(m2s_band_components_opts))
    return fail(M2S_ERR_BAD_ARG, "m2s_band_components_opts.struct_size is not sizeof(m2s_band_components_opts)");
  const int connectivity = copts ? copts->connectivity : (int)M2S_CONNECT_6;
  if (bad_connectivity(connectivity)) return fail(M2S_ERR_BAD_ARG, "connectivity = %d: must be 6, 18 or 26", connectivity);
  int rc = band_opts_args(opts, "m2s_band_components");
  if (rc) return rc;
  m2s_opts o;
  rc = band_call_opts(band, opts, &o);
  if (rc) return rc;
  o.synchronous = 1;
  const uint64_t n = band->n;
  if (n >= 0xffffffffull) return fail(M2S_ERR_BAD_ARG, "%llu cells: labels and parents are 32-bit", (unsigned long long)n);
  if (n == 0) {
    *n_components_out = 0;
    return M2S_OK;
  }
  CallCtx c;
  DeviceState* st = nullptr;
  rc = resolve_ctx(&o, &c, &st);
  if (rc) return rc;
  const bool host = c.mem_kind == M2S_MEM_HOST;
  const bool stats = components_out != nullptr, want = stats || labels_out != nullptr;
  const WalkGrid g = walk_grid_of(band->grid.cell_count, band->total, band->n_words);
  const uint64_t n_units = (g.n_words + kWalkUnit - 1) / kWalkUnit;   // below 2^22: a grid has fewer than 2^36 cells
  const unsigned blocks = (unsigned)((n_units + kWalkWaves - 1) / kWalkWaves);
  const uint32_t n_tiles = tiles_of(n);
  rc = ensure_capacity(*st, 4096 + align_up((size_t)n_tiles * 8));
  if (rc) return rc;
  Arena ws{st->base, st->cap, 0};
  uint64_t* d_total = ws.take<uint64_t>(4);
  uint64_t* tile_sum = ws.take<uint64_t>(n_tiles);
  if (!d_total || !tile_sum) return fail(M2S_ERR_HIP, "internal: workspace");
  // parent, and the labels where the caller's are not device memory (or not wanted, with statistics that need them)
  const bool own_labels = want && (host || !labels_out);
  const size_t b_parent = align_up(n * 4);
  char* tmp = nullptr;
  char* tmp2 = nullptr;   // the statistics of a host caller: sized once the count is known
  auto drop = [&](int code) {
    (void)hipFree(tmp2);
    (void)hipFree(tmp);
    return code;
  };
  auto hip_fail = [&](hipError_t e) { return drop(fail(M2S_ERR_HIP, "HIP error: %s", hipGetErrorString(e))); };
  hipError_t e = hipMalloc((void**)&tmp, b_parent + (own_labels ? b_parent : 0));
  if (e != hipSuccess) return hip_fail(e);
  uint32_t* parent = reinterpret_cast<uint32_t*>(tmp);
  uint32_t* labels = own_labels ? reinterpret_cast<uint32_t*>(tmp + b_parent) : labels_out;
  const BandDev X = dev_of(band);
  hipStream_t s = c.stream;
  if (c.timings) e = hipEventRecord(st->ev[0], s);
  if (e != hipSuccess) return hip_fail(e);
  hipLaunchKernelGGL(k_cc_init, dim3(blocks_for(n)), dim3(256), 0, s, parent, n);
  if (connectivity == M2S_CONNECT_6) hipLaunchKernelGGL((k_cc_hook<1>), dim3(blocks), dim3(kWalkThreads), 0, s, X, g, parent);
  else if (connectivity == M2S_CONNECT_18) hipLaunchKernelGGL((k_cc_hook<2>), dim3(blocks), dim3(kWalkThreads), 0, s, X, g, parent);
  else hipLaunchKernelGGL((k_cc_hook<3>), dim3(blocks), dim3(kWalkThreads), 0, s, X, g, parent);
  hipLaunchKernelGGL(k_cc_flatten, dim3(n_tiles), dim3(kTileThreads), 0, s, parent, n, tile_sum);
  hipLaunchKernelGGL((k_scan_tiles<kCcScanThreads, uint64_t>), dim3(1), dim3(kCcScanThreads), 0, s, tile_sum, (uint64_t)n_tiles, d_total);
  if (want) hipLaunchKernelGGL(k_cc_number, dim3(n_tiles), dim3(kTileThreads), 0, s, (const uint32_t*)parent, n, (const uint64_t*)tile_sum, labels);
  e = hipGetLastError();
  uint64_t count = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&count, d_total, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);   // the count decides whether the statistics fit
  if (e != hipSuccess) return hip_fail(e);
  *n_components_out = count;
  if (stats && capacity < count)
    return drop(fail(M2S_ERR_BAD_ARG, "capacity = %llu below the band's %llu components", (unsigned long long)capacity, (unsigned long long)count));
  if (want) {
    m2s_band_component* comps = components_out;
    if (stats && host) {
      e = hipMalloc((void**)&tmp2, align_up(count * sizeof(m2s_band_component)));
      if (e != hipSuccess) return hip_fail(e);
      comps = reinterpret_cast<m2s_band_component*>(tmp2);
    }
    if (stats) hipLaunchKernelGGL(k_cc_clear, dim3(blocks_for(count)), dim3(256), 0, s, comps, count);
    hipLaunchKernelGGL(k_cc_label, dim3(blocks), dim3(kWalkThreads), 0, s, X, g, (const uint32_t*)parent, labels, stats ? comps : nullptr, count);
    e = hipGetLastError();
    if (e == hipSuccess && host && labels_out) e = hipMemcpyAsync(labels_out, labels, n * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && host && stats) e = hipMemcpyAsync(components_out, comps, count * sizeof(m2s_band_component), hipMemcpyDeviceToHost, s);
  }
  if (e == hipSuccess && c.timings) e = hipEventRecord(st->ev[1], s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(e);
  if (c.timings) {
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, st->ev[0], st->ev[1]);
    memset(c.timings, 0, sizeof(*c.timings));
    c.timings->distance_ms = ms;
    c.timings->total_ms = ms;
    c.timings->n_units = n;
  }
  return drop(M2S_OK);
}

int m2s_band_select(const m2s_band* band, const uint32_t* labels, const uint8_t* keep, uint64_t n_keep, const m2s_band_field_opts* fopts,
                    const m2s_opts* opts, m2s_band** out, m2s_band_select_info* info_out) {
  clear_error();
  if (!out) return fail(M2S_ERR_BAD_ARG, "out is NULL");
  *out = nullptr;
  if (!band) return fail(M2S_ERR_BAD_ARG, "band is NULL");
  if (!labels) return fail(M2S_ERR_BAD_ARG, "labels is NULL");
  if (!keep && n_keep > 0) return fail(M2S_ERR_BAD_ARG, "keep is NULL with n_keep = %llu", (unsigned long long)n_keep);
  int rc = band_field_opts_args(fopts);
  if (rc) return rc;
  if (info_out && info_out->struct_size != sizeof(m2s_band_select_info))
    return fail(M2S_ERR_BAD_ARG, "m2s_band_select_info.struct_size is not sizeof(m2s_band_select_info)");
  rc = band_opts_args(opts, "m2s_band_select");
  if (rc) return rc;
  m2s_opts o;
  rc = band_call_opts(band, opts, &o);
  if (rc) return rc;
  o.synchronous = 1;
  CallCtx c;
  DeviceState* st = nullptr;
  rc = resolve_ctx(&o, &c, &st);
  if (rc) return rc;
  const bool host = c.mem_kind == M2S_MEM_HOST;
  const uint64_t n = band->n;
  const WalkGrid g = walk_grid_of(band->grid.cell_count, band->total, band->n_words);
  const uint64_t n_words = g.n_words;
  const uint64_t cap = std::max<uint64_t>(1, n);                      // the bound of the result's cells: at least one float
  const uint64_t n_units = (n_words + kWalkUnit - 1) / kWalkUnit;     // below 2^22: a grid has fewer than 2^36 cells
  const unsigned blocks = (unsigned)((n_units + kWalkWaves - 1) / kWalkWaves);
  const uint64_t n_groups = (n_units + kSelGroup - 1) / kSelGroup;
  char* tmp = nullptr;   // a host caller's labels and keep
  BandBlock res;
  auto drop = [&](int code) {
    (void)hipFree(tmp);
    res.free();
    return code;
  };
  auto hip_fail = [&](hipError_t e) { return drop(fail(M2S_ERR_HIP, "HIP error: %s", hipGetErrorString(e))); };
  rc = ensure_capacity(*st, 4096 + 256 + align_up((size_t)n_units * 4) + align_up((size_t)n_groups * 8));
  if (rc) return rc;
  Arena ws{st->base, st->cap, 0};
  uint64_t* d_hdr = ws.take<uint64_t>(4);   // [0] the result's cells, [1] n_sign_cleared
  uint32_t* unit_cnt = ws.take<uint32_t>(n_units);
  uint64_t* group_sum = ws.take<uint64_t>(n_groups);
  if (!d_hdr || !unit_cnt || !group_sum) return fail(M2S_ERR_HIP, "internal: workspace");
  hipStream_t s = c.stream;
  hipError_t e = res.alloc(n_words, cap);
  if (e != hipSuccess) return hip_fail(e);
  const uint32_t* d_labels = labels;
  const uint8_t* d_keep = keep;
  if (host) {
    const size_t b_labels = align_up(cap * 4);
    e = hipMalloc((void**)&tmp, b_labels + align_up(std::max<uint64_t>(1, n_keep)));
    if (e == hipSuccess && n) e = hipMemcpyAsync(tmp, labels, n * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && n_keep) e = hipMemcpyAsync(tmp + b_labels, keep, n_keep, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return hip_fail(e);
    d_labels = reinterpret_cast<const uint32_t*>(tmp);
    d_keep = reinterpret_cast<const uint8_t*>(tmp + b_labels);
  }
  const BandDev X = dev_of(band);
  if (c.timings) e = hipEventRecord(st->ev[0], s);
  if (e == hipSuccess) e = hipMemsetAsync(d_hdr, 0, 32, s);
  if (e == hipSuccess) e = hipMemsetAsync(res.dist, 0, 4, s);   // an empty result still has one defined float
  if (e == hipSuccess) e = hipMemsetAsync(group_sum, 0, n_groups * 8, s);
  if (e != hipSuccess) return hip_fail(e);
  hipLaunchKernelGGL(k_sel_mask, dim3(blocks), dim3(kWalkThreads), 0, s, X, g, SelArgs{d_labels, d_keep, n_keep}, res.mask, res.inside, unit_cnt,
                     group_sum, d_hdr + 1);
  hipLaunchKernelGGL((k_scan_tiles<kCcScanThreads, uint64_t>), dim3(1), dim3(kCcScanThreads), 0, s, group_sum, n_groups, d_hdr);
  hipLaunchKernelGGL(k_sel_emit, dim3(blocks), dim3(kWalkThreads), 0, s, X, n_words, (const uint64_t*)res.mask, (const uint32_t*)unit_cnt,
                     (const uint64_t*)group_sum, res.word_off, res.dist, cap);
  e = hipGetLastError();
  if (e == hipSuccess && c.timings) e = hipEventRecord(st->ev[1], s);
  uint64_t hdr[2] = {0, 0};
  if (e == hipSuccess) e = hipMemcpyAsync(hdr, d_hdr, 16, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(e);
  if (hdr[0] > n) return drop(fail(M2S_ERR_HIP, "internal: the result has %llu cells, above the input's %llu", (unsigned long long)hdr[0], (unsigned long long)n));
  if (c.timings) {
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, st->ev[0], st->ev[1]);
    memset(c.timings, 0, sizeof(*c.timings));
    c.timings->seed_ms = ms;
    c.timings->total_ms = ms;
    c.timings->n_units = hdr[0];
  }
  (void)hipFree(tmp);
  tmp = nullptr;
  if (info_out) {
    info_out->reserved = 0;
    info_out->n_cells = hdr[0];
    info_out->n_dropped = n - hdr[0];
    info_out->n_sign_cleared = hdr[1];
  }
  *out = band_adopt(res, band->device, band->grid, hdr[0], g.total, n_words, fopts ? fopts->background_outside : band->bg_out,
                    fopts ? fopts->background_inside : band->bg_in);
  return M2S_OK;
}

}  // extern "C"
