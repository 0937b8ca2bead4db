// band_redistance.hip — m2s_band_redistance: a resident band turned back into a distance field with the same zero set and the half-widths
// the caller asks for, gfx950.  The contract is include/m2s.h's (per grid point, to the bit); tests/band_redistance_model.py restates it
// in numpy.  Nothing sized 4 bytes per grid point exists: the arrays are per mask word (8 bytes per 64 points) or per candidate cell.
//
// Every kernel that walks the mask words is band_walk.hip.h's walk, units of 256 words.
//   k_rd_sign     s on every grid point (the result's sign mask): the source's sign word where no point is active, else the values' signs.
//   k_rd_frozen   F: per active point the six neighbours' act and s bits; n_frozen, n_open.
//   k_rd_dilate   one axis of the box dilation, a gather: a word first ORs the 2K + 1 shifted windows of its source (a superset: it
//                 ignores the row ends); only words where that is not zero are taken by the wave, lane t testing its own clipped range.
//   k_rd_select   C = s ? dilation by the interior K : by the exterior K.
//   k_rd_count / k_scan_tiles / k_rd_offsets   a mask's word_off (used for C and for the result): band_walk.hip.h's offsets, groups of 16.
//   k_rd_table    per candidate, once: the places in C of its six neighbours (a rank look-up each: C word, word_off, popcount below),
//                 with the in-grid, same-sign and in-C tests folded into an empty slot; meta (frozen, s); u = |x| on F, +inf on the rest
//                 of C, into both value buffers.
//   k_rd_sweep    one Jacobi sweep, one lane per candidate: six slots, six values from the sweep's input buffer, the update, a store of
//                 min(u, t) to the OTHER buffer; a sweep that lowers a value stores 1 to its flag.  It reads no index word and divides
//                 nothing.  (The form that looks the neighbours up in every sweep, a wave per 256 index words, took 0.79 ms per sweep
//                 at 256^3 and 15.3 ms at 2048^3, this one 0.036 and 1.79: profiles/band_redistance.txt.)
//   k_rd_final    the result's mask: F, or in C with u <= W.
//   k_rd_emit     the result's values at its word_off + rank: x on F, else -u / +u by s.
// All stores are plain vector stores; the ballot loops are wave-uniform.
#include "../../include/m2s.h"
#include "band_handle.h"
#include "band_walk.hip.h"
#include "capi_internal.h"
#include "common.h"
#include "scan.hip.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace m2s {
namespace {

constexpr int kRdGroup = 16;                               // units per scanned sum
constexpr int kRdScanThreads = 1024;
constexpr int kRdBatch = 4;                                // sweeps between two reads of the change flags

__device__ __forceinline__ bool rd_bit(const uint64_t* __restrict__ a, uint64_t L) { return (a[L >> 6] >> (L & 63)) & 1ull; }

// s on every grid point, bits past the grid zero.
__global__ void __launch_bounds__(kWalkThreads) k_rd_sign(BandDev X, WalkGrid g, uint64_t* __restrict__ S) {
  WALK_UNIT_HEAD(kWalkSteps, g.n_words)
  for (int step = 0; step < kWalkSteps; ++step) {
    WALK_STEP_HEAD(g.n_words)
    const uint64_t m = in_range ? X.mask[w] : 0;
    const uint64_t in = in_range && X.inside ? X.inside[w] : 0;
    const uint64_t wo = m ? X.word_off[w] : 0;
    const uint64_t valid = walk_valid(w, in_range, g.total);
    uint64_t s = in & valid;
    uint64_t todo = __ballot(m != 0);
    while (todo) {   // wave-uniform
      const int j = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const uint64_t mj = walk_lane(m, j), inj = walk_lane(in, j), woj = walk_lane(wo, j);
      const bool act = (mj >> lane) & 1ull;
      uint64_t at = woj + (uint64_t)__popcll(mj & walk_below(lane));
      at = at < X.n ? at : 0;
      bool sb = (inj >> lane) & 1ull;
      if (act) sb = X.dist[at] < 0.0f;
      const uint64_t sm = __ballot(sb);
      if (lane == j) s = sm & valid;
    }
    if (in_range) S[w] = s;
  }
}

// F, and counters[0] += n_frozen, counters[1] += n_open.
__global__ void __launch_bounds__(kWalkThreads) k_rd_frozen(const uint64_t* __restrict__ mask, const uint64_t* __restrict__ S, WalkGrid g,
                                                          uint64_t* __restrict__ Fm, uint64_t* __restrict__ counters) {
  WALK_UNIT_HEAD(kWalkSteps, g.n_words)
  uint64_t n_frozen = 0, n_open = 0;
  for (int step = 0; step < kWalkSteps; ++step) {
    WALK_STEP_HEAD(g.n_words)
    const uint64_t m = in_range ? mask[w] : 0;
    const uint64_t sw = m ? S[w] : 0;
    WalkIjk base{0, 0, 0};
    if (m) base = walk_base(w << 6, g);
    uint64_t f = 0;
    uint64_t todo = __ballot(m != 0);
    while (todo) {   // wave-uniform
      const int j = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const uint64_t mj = walk_lane(m, j), sj = walk_lane(sw, j);
      const WalkIjk p = walk_step(walk_bcast(base, j), (uint32_t)lane, g);
      const uint64_t L = ((wb + (uint64_t)j) << 6) + (uint64_t)lane;
      const bool act = (mj >> lane) & 1ull, sL = (sj >> lane) & 1ull;
      bool frozen = false;
      uint32_t open = 0;
      if (act) {   // an active point is inside the grid
#define RD_NB(cond, M)                                        \
  if (cond) {                                                 \
    const uint64_t Mv = (M);                                  \
    if (rd_bit(S, Mv) != sL) {                                \
      if (rd_bit(mask, Mv)) frozen = true;                    \
      else ++open;                                            \
    }                                                         \
  }
        RD_NB(p.i + 1 < g.nx, L + g.si)
        RD_NB(p.i > 0, L - g.si)
        RD_NB(p.j + 1 < g.ny, L + g.sj)
        RD_NB(p.j > 0, L - g.sj)
        RD_NB(p.k + 1 < g.nz, L + 1)
        RD_NB(p.k > 0, L - 1)
#undef RD_NB
      }
      const uint64_t fm = __ballot(frozen);
      if (lane == j) f = fm;
      n_open += open;
    }
    if (in_range) Fm[w] = f;
    n_frozen += (uint64_t)__popcll(f);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n_frozen += __shfl_xor(n_frozen, o, 64);
    n_open += __shfl_xor(n_open, o, 64);
  }
  if (lane == 0) {
    if (n_frozen) atomicAdd((unsigned long long*)counters, (unsigned long long)n_frozen);
    if (n_open) atomicAdd((unsigned long long*)(counters + 1), (unsigned long long)n_open);
  }
}

// 64 bits of src from bit `bit0` on (any sign, any alignment); bits off the array are zero.
__device__ __forceinline__ uint64_t rd_window(const uint64_t* __restrict__ src, int64_t bit0, uint64_t n_words) {
  const int64_t w = bit0 >> 6;   // floor
  const int sh = (int)(bit0 & 63);
  const uint64_t lo = (w >= 0 && (uint64_t)w < n_words) ? src[w] : 0;
  if (sh == 0) return lo;
  const uint64_t hi = (w + 1 >= 0 && (uint64_t)(w + 1) < n_words) ? src[w + 1] : 0;
  return (lo >> sh) | (hi << (64 - sh));
}

// dst = src dilated along one axis (AXIS 0: i, 1: j, 2: k) by the taps d * hop, |d| <= K, clipped to the grid.  hop == 1: the box
// dilation by K.
template <int AXIS>
__global__ void __launch_bounds__(kWalkThreads) k_rd_dilate(const uint64_t* __restrict__ src, WalkGrid g, int64_t K, int64_t hop, uint64_t* __restrict__ dst) {
  WALK_UNIT_HEAD(kWalkSteps, g.n_words)
  const int64_t stride = (AXIS == 0 ? (int64_t)g.si : AXIS == 1 ? (int64_t)g.sj : 1) * hop;
  const int64_t n_axis = (int64_t)(AXIS == 0 ? g.nx : AXIS == 1 ? g.ny : g.nz);
  for (int step = 0; step < kWalkSteps; ++step) {
    WALK_STEP_HEAD(g.n_words)
    uint64_t any = 0;
    if (in_range) {
      if (AXIS == 2 && hop == 1 && K < 64) {   // the windows overlap: the word, the K bits before it and the K bits after it
        any = src[w];
        if (w > 0) any |= src[w - 1] >> (64 - K);
        if (w + 1 < g.n_words) any |= src[w + 1] << (64 - K);
      } else {
        for (int64_t d = -K; d <= K; ++d) any |= rd_window(src, (int64_t)(w << 6) + d * stride, g.n_words);
      }
    }
    WalkIjk base{0, 0, 0};
    if (any) base = walk_base(w << 6, g);
    const uint64_t valid = walk_valid(w, in_range, g.total);
    uint64_t out = 0;
    uint64_t todo = __ballot(any != 0);
    while (todo) {   // wave-uniform
      const int j = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const WalkIjk p = walk_step(walk_bcast(base, j), (uint32_t)lane, g);
      const int64_t L = (int64_t)(((wb + (uint64_t)j) << 6) + (uint64_t)lane);
      const int64_t c = (int64_t)(AXIS == 0 ? p.i : AXIS == 1 ? p.j : p.k);
      bool hit = false;
      if ((uint64_t)L < g.total)
        for (int64_t d = -K; d <= K; ++d)
          if (c + d * hop >= 0 && c + d * hop < n_axis) hit = hit || rd_bit(src, (uint64_t)(L + d * stride));
      const uint64_t hm = __ballot(hit);
      if (lane == j) out = hm & valid;
    }
    if (in_range) dst[w] = out;
  }
}

// C may be DE, and DI may be DE (one reach for both sides): no __restrict__ on them.
__global__ void __launch_bounds__(256) k_rd_select(const uint64_t* DE, const uint64_t* DI, const uint64_t* __restrict__ S, uint64_t n_words,
                                                   uint64_t* C) {
  for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * 256) {
    const uint64_t s = S[w];
    C[w] = (DE[w] & ~s) | (DI[w] & s);
  }
}

// A mask's popcounts per unit, and by one atomic add per unit the sum of its group (zeroed by the launcher).
__global__ void __launch_bounds__(kWalkThreads) k_rd_count(const uint64_t* __restrict__ mask, WalkGrid g, uint32_t* __restrict__ unit_cnt,
                                                         uint64_t* __restrict__ group_sum) {
  WALK_UNIT_HEAD(kWalkSteps, g.n_words)
  uint64_t cnt = 0;
  for (int step = 0; step < kWalkSteps; ++step) {
    WALK_STEP_HEAD(g.n_words)
    cnt += in_range ? (uint64_t)__popcll(mask[w]) : 0;
  }
  walk_publish<kRdGroup>(cnt, lane, unit, unit_cnt, group_sum);
}

// word_off of a mask from the scanned group sums and the unit counts.
__global__ void __launch_bounds__(kWalkThreads) k_rd_offsets(const uint64_t* __restrict__ mask, WalkGrid g, const uint32_t* __restrict__ unit_cnt,
                                                           const uint64_t* __restrict__ group_base, uint64_t* __restrict__ word_off) {
  WALK_UNIT_HEAD(kWalkSteps, g.n_words)
  uint64_t base = walk_unit_base<kRdGroup>(lane, unit, unit_cnt, group_base);
  for (int step = 0; step < kWalkSteps; ++step) {
    WALK_STEP_HEAD(g.n_words)
    const uint64_t off = walk_word_off(in_range ? (uint64_t)__popcll(mask[w]) : 0, lane, base);
    if (in_range) word_off[w] = off;
  }
}

// x of an active point of X: bit t of word w.
__device__ __forceinline__ float rd_x(const BandDev& X, uint64_t mX, uint64_t woX, int t) {
  return X.dist[walk_rank(mX, woX, t, X.n)];
}

struct RdField {
  const uint64_t* C;
  const uint64_t* Coff;
  const uint64_t* S;
  const float* u;
  uint64_t n_cand;
};

constexpr uint32_t kRdNone = 0xffffffffu;   // a neighbour slot with nothing to read: off the grid, outside C or on the other side

// The rank in C of a neighbour on the side sL of its point, kRdNone if M is on the other side or outside C.
__device__ __forceinline__ uint32_t rd_slot(const RdField& p, uint64_t M, bool sL) {
  const uint64_t w = M >> 6;
  const int b = (int)(M & 63);
  const uint64_t cm = p.C[w];
  uint32_t slot = kRdNone;
  if (((cm >> b) & 1ull) && (((p.S[w] >> b) & 1ull) != 0) == sL) {
    const uint64_t r = p.Coff[w] + (uint64_t)__popcll(cm & walk_below(b));
    if (r < p.n_cand) slot = (uint32_t)r;   // n_cand < kRdNone (the host checks)
  }
  return slot;
}

// Per candidate, once: its six neighbour slots (i+, i-, j+, j-, k+, k-; slots[n * n_cand + r]), meta (bit 0: frozen, bit 1: s) and the
// start value u = |x| on F, +inf elsewhere, into both value buffers.  The in-grid test, the same-sign test and the membership in C
// fold into kRdNone, so a sweep needs no index word and no coordinate.
__global__ void __launch_bounds__(kWalkThreads) k_rd_table(BandDev X, WalkGrid g, const uint64_t* __restrict__ Fm, RdField fld, uint32_t* __restrict__ slots,
                                                         uint8_t* __restrict__ meta, float* __restrict__ u0, float* __restrict__ u1) {
  WALK_UNIT_HEAD(kWalkSteps, g.n_words)
  for (int step = 0; step < kWalkSteps; ++step) {
    WALK_STEP_HEAD(g.n_words)
    const uint64_t c = in_range ? fld.C[w] : 0;
    const uint64_t co = c ? fld.Coff[w] : 0;
    const uint64_t f = c ? Fm[w] : 0;
    const uint64_t sw = c ? fld.S[w] : 0;
    const uint64_t mX = f ? X.mask[w] : 0;
    const uint64_t woX = f ? X.word_off[w] : 0;
    WalkIjk base{0, 0, 0};
    if (c) base = walk_base(w << 6, g);
    uint64_t todo = __ballot(c != 0);
    while (todo) {   // wave-uniform
      const int j = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const uint64_t cj = walk_lane(c, j), coj = walk_lane(co, j), fj = walk_lane(f, j), sj = walk_lane(sw, j), mXj = walk_lane(mX, j), woXj = walk_lane(woX, j);
      const WalkIjk p = walk_step(walk_bcast(base, j), (uint32_t)lane, g);
      const uint64_t L = ((wb + (uint64_t)j) << 6) + (uint64_t)lane;
      const uint64_t r = coj + (uint64_t)__popcll(cj & walk_below(lane));
      if (((cj >> lane) & 1ull) && r < fld.n_cand) {   // a point of C is inside the grid
        const bool sL = (sj >> lane) & 1ull, frozen = (fj >> lane) & 1ull;
        uint32_t s0 = kRdNone, s1 = kRdNone, s2 = kRdNone, s3 = kRdNone, s4 = kRdNone, s5 = kRdNone;
        float v = INFINITY;
        if (frozen) {
          v = fabsf(rd_x(X, mXj, woXj, lane));
        } else {
          if (p.i + 1 < g.nx) s0 = rd_slot(fld, L + g.si, sL);
          if (p.i > 0) s1 = rd_slot(fld, L - g.si, sL);
          if (p.j + 1 < g.ny) s2 = rd_slot(fld, L + g.sj, sL);
          if (p.j > 0) s3 = rd_slot(fld, L - g.sj, sL);
          if (p.k + 1 < g.nz) s4 = rd_slot(fld, L + 1, sL);
          if (p.k > 0) s5 = rd_slot(fld, L - 1, sL);
        }
        slots[r] = s0;
        slots[fld.n_cand + r] = s1;
        slots[2 * fld.n_cand + r] = s2;
        slots[3 * fld.n_cand + r] = s3;
        slots[4 * fld.n_cand + r] = s4;
        slots[5 * fld.n_cand + r] = s5;
        meta[r] = (uint8_t)((frozen ? 1u : 0u) | (sL ? 2u : 0u));
        u0[r] = v;
        u1[r] = v;
      }
    }
  }
}

// The first-order Godunov update of include/m2s.h from the three axis minima, each with its h and w = 1 / (h * h).
__device__ __forceinline__ float rd_update(float a1, float a2, float a3, float h1, float h2, float h3, float w1, float w2, float w3) {
#define RD_SWAP(x, y) { const float tmp_ = x; x = y; y = tmp_; }
  if (a2 < a1) { RD_SWAP(a1, a2) RD_SWAP(h1, h2) RD_SWAP(w1, w2) }   // a stable sort of three: swaps on a strict < only
  if (a3 < a2) { RD_SWAP(a2, a3) RD_SWAP(h2, h3) RD_SWAP(w2, w3) }
  if (a2 < a1) { RD_SWAP(a1, a2) RD_SWAP(h1, h2) RD_SWAP(w1, w2) }
#undef RD_SWAP
  float t = a1 + h1;
  if (t > a2) {
    const float d2 = a2 - a1;
    float A = w1 + w2;
    float B = w2 * d2;
    const float q2 = B * d2;
    float Cc = q2 - 1.0f;
    float disc = B * B - A * Cc;
    disc = disc > 0.0f ? disc : 0.0f;
    t = a1 + (B + sqrtf(disc)) / A;
    if (t > a3) {
      const float d3 = a3 - a1;
      A = A + w3;
      B = B + w3 * d3;
      Cc = (q2 + w3 * d3 * d3) - 1.0f;
      disc = B * B - A * Cc;
      disc = disc > 0.0f ? disc : 0.0f;
      t = a1 + (B + sqrtf(disc)) / A;
    }
  }
  return t;
}

// c(u[slot], M): the neighbour's value cut off at W, +inf for an empty slot.
__device__ __forceinline__ float rd_value(const float* __restrict__ u, uint32_t slot, float W) {
  float v = INFINITY;
  if (slot != kRdNone) {
    const float x = u[slot];
    v = x <= W ? x : INFINITY;
  }
  return v;
}

// One Jacobi sweep, one lane per candidate: u_out = min(u_in, t) on C \ F, from u_in only (u_out is the other buffer).
__global__ void __launch_bounds__(256) k_rd_sweep(const uint32_t* __restrict__ slots, const uint8_t* __restrict__ meta, const float* __restrict__ u_in,
                                                  float* __restrict__ u_out, uint64_t n_cand, float w_out, float w_in, float hx, float hy, float hz,
                                                  float wx, float wy, float wz, uint32_t* __restrict__ flag) {
  bool changed = false;
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_cand; r += (uint64_t)gridDim.x * 256) {
    const uint32_t m = meta[r];
    if (m & 1u) continue;   // frozen: both buffers hold |x|
    const float W = (m & 2u) ? w_in : w_out;
    const uint32_t s0 = slots[r], s1 = slots[n_cand + r], s2 = slots[2 * n_cand + r], s3 = slots[3 * n_cand + r], s4 = slots[4 * n_cand + r],
                   s5 = slots[5 * n_cand + r];
    const float u = u_in[r];
    float mi = INFINITY, mj = INFINITY, mk = INFINITY, v;
    v = rd_value(u_in, s0, W); mi = v < mi ? v : mi;
    v = rd_value(u_in, s1, W); mi = v < mi ? v : mi;
    v = rd_value(u_in, s2, W); mj = v < mj ? v : mj;
    v = rd_value(u_in, s3, W); mj = v < mj ? v : mj;
    v = rd_value(u_in, s4, W); mk = v < mk ? v : mk;
    v = rd_value(u_in, s5, W); mk = v < mk ? v : mk;
    const float t = rd_update(mi, mj, mk, hx, hy, hz, wx, wy, wz);
    const bool lower = t < u;
    u_out[r] = lower ? t : u;
    changed = changed || lower;
  }
  if (changed) *flag = 1u;
}

// The result's mask: F, or in C with u <= W.
__global__ void __launch_bounds__(kWalkThreads) k_rd_final(WalkGrid g, const uint64_t* __restrict__ Fm, RdField fld, float w_out, float w_in,
                                                         uint64_t* __restrict__ R) {
  WALK_UNIT_HEAD(kWalkSteps, g.n_words)
  for (int step = 0; step < kWalkSteps; ++step) {
    WALK_STEP_HEAD(g.n_words)
    const uint64_t c = in_range ? fld.C[w] : 0;
    const uint64_t f = c ? Fm[w] : 0;
    const uint64_t co = c ? fld.Coff[w] : 0;
    const uint64_t sw = c ? fld.S[w] : 0;
    uint64_t out = 0;
    uint64_t todo = __ballot(c != 0);
    while (todo) {   // wave-uniform
      const int j = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const uint64_t cj = walk_lane(c, j), fj = walk_lane(f, j), coj = walk_lane(co, j), sj = walk_lane(sw, j);
      uint64_t r = coj + (uint64_t)__popcll(cj & walk_below(lane));
      r = r < fld.n_cand ? r : 0;
      bool keep = false;
      if ((cj >> lane) & 1ull) keep = ((fj >> lane) & 1ull) || fld.u[r] <= (((sj >> lane) & 1ull) ? w_in : w_out);
      const uint64_t km = __ballot(keep);
      if (lane == j) out = km;
    }
    if (in_range) R[w] = out | f;   // F is inside C
  }
}

// The result's values at Roff + rank: x on F, else -u or +u by s.  cap: the floats out holds.
__global__ void __launch_bounds__(kWalkThreads) k_rd_emit(BandDev X, WalkGrid g, const uint64_t* __restrict__ Fm, RdField fld, const uint64_t* __restrict__ R,
                                                        const uint64_t* __restrict__ Roff, float* __restrict__ out, uint64_t cap) {
  WALK_UNIT_HEAD(kWalkSteps, g.n_words)
  for (int step = 0; step < kWalkSteps; ++step) {
    WALK_STEP_HEAD(g.n_words)
    const uint64_t rm = in_range ? R[w] : 0;
    const uint64_t ro = rm ? Roff[w] : 0;
    const uint64_t c = rm ? fld.C[w] : 0;
    const uint64_t co = rm ? fld.Coff[w] : 0;
    const uint64_t sw = rm ? fld.S[w] : 0;
    const uint64_t f = rm ? Fm[w] : 0;
    const uint64_t mX = f ? X.mask[w] : 0;
    const uint64_t woX = f ? X.word_off[w] : 0;
    uint64_t todo = __ballot(rm != 0);
    while (todo) {   // wave-uniform
      const int j = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const uint64_t rj = walk_lane(rm, j), roj = walk_lane(ro, j), cj = walk_lane(c, j), coj = walk_lane(co, j), sj = walk_lane(sw, j), fj = walk_lane(f, j);
      const uint64_t mXj = walk_lane(mX, j), woXj = walk_lane(woX, j);
      if ((rj >> lane) & 1ull) {
        float v;
        if ((fj >> lane) & 1ull) {
          v = rd_x(X, mXj, woXj, lane);
        } else {
          uint64_t r = coj + (uint64_t)__popcll(cj & walk_below(lane));
          r = r < fld.n_cand ? r : 0;
          const float u = fld.u[r];
          v = ((sj >> lane) & 1ull) ? -u : u;
        }
        const uint64_t pos = roj + (uint64_t)__popcll(rj & walk_below(lane));
        if (pos < cap) out[pos] = v;
      }
    }
  }
}

// K_a = min(ceil(W / h_a) + 1, n_a), the division and the ceil in binary32.
int64_t reach(float width, float h, uint64_t n) {
  const float c = ceilf(width / h);
  return (double)c >= (double)n ? (int64_t)n : (int64_t)c + 1;
}

template <int AXIS>
void dilate_axis(hipStream_t st, unsigned blocks, const WalkGrid& g, int64_t K, int64_t hop, const uint64_t* src, uint64_t* dst) {
  hipLaunchKernelGGL((k_rd_dilate<AXIS>), dim3(blocks), dim3(kWalkThreads), 0, st, src, g, K, hop, dst);
}

// dst = src dilated by the box K.  One gather per axis over its 2K + 1 windows.  M2S_RD_DILATE (an A/B build, tools/build_ab.sh) selects
// what it was measured against: 1: K single steps per axis, 2: steps of 1, 2, 4, ... (three taps each), both through t1 and t2 and a copy.
void dilate(hipStream_t st, unsigned blocks, const WalkGrid& g, const int64_t K[3], const uint64_t* src, uint64_t* t1, uint64_t* t2, uint64_t* dst) {
#if defined(M2S_RD_DILATE) && M2S_RD_DILATE > 0
  const uint64_t* cur = src;
  uint64_t* bufs[2] = {t1, t2};
  int at = 0;
  for (int axis = 2; axis >= 0; --axis) {
    int64_t done = 0;
    while (done < K[axis]) {
      const int64_t hop = M2S_RD_DILATE == 1 ? 1 : std::min<int64_t>(done + 1, K[axis] - done);   // the set reaches `done`: a hop of done + 1 leaves no gap
      if (axis == 2) dilate_axis<2>(st, blocks, g, 1, hop, cur, bufs[at]);
      else if (axis == 1) dilate_axis<1>(st, blocks, g, 1, hop, cur, bufs[at]);
      else dilate_axis<0>(st, blocks, g, 1, hop, cur, bufs[at]);
      cur = bufs[at];
      at ^= 1;
      done += hop;
    }
  }
  (void)hipMemcpyAsync(dst, cur, g.n_words * 8, hipMemcpyDeviceToDevice, st);
#else
  dilate_axis<2>(st, blocks, g, K[2], 1, src, t1);
  dilate_axis<1>(st, blocks, g, K[1], 1, (const uint64_t*)t1, t2);
  dilate_axis<0>(st, blocks, g, K[0], 1, (const uint64_t*)t2, dst);
#endif
}

}  // namespace

// m2s_warmup: the first launch of a kernel of this translation unit makes the runtime load its code object (all its kernels).
__global__ void k_warm_band_redistance() {}
void warm_band_redistance(hipStream_t st) { hipLaunchKernelGGL(k_warm_band_redistance, dim3(1), dim3(64), 0, st); }

}  // namespace m2s

using namespace m2s;

extern "C" {

int m2s_band_redistance(const m2s_band* band, const m2s_band_redistance_opts* ropts, const m2s_band_field_opts* fopts, const m2s_opts* opts,
                        m2s_band** out, m2s_band_redistance_info* info_out) {
  clear_error();
  if (!out) return fail(M2S_ERR_BAD_ARG, "out is NULL");
  *out = nullptr;
  if (!band) return fail(M2S_ERR_BAD_ARG, "band is NULL");
  if (!ropts) return fail(M2S_ERR_BAD_ARG, "m2s_band_redistance_opts is NULL");
  if (ropts->struct_size != sizeof(m2s_band_redistance_opts))
    return fail(M2S_ERR_BAD_ARG, "m2s_band_redistance_opts.struct_size is not sizeof(m2s_band_redistance_opts)");
  if (!good_background(ropts->exterior) || !good_background(ropts->interior))   // a width is judged as a background is
    return fail(M2S_ERR_BAD_ARG, "the widths (%g exterior, %g interior) must be >= 0 and finite", (double)ropts->exterior, (double)ropts->interior);
  int rc = band_field_opts_args(fopts);
  if (rc) return rc;
  if (info_out && info_out->struct_size != sizeof(m2s_band_redistance_info))
    return fail(M2S_ERR_BAD_ARG, "m2s_band_redistance_info.struct_size is not sizeof(m2s_band_redistance_info)");
  rc = band_opts_args(opts, "m2s_band_redistance");
  if (rc) return rc;
  m2s_opts o;
  rc = band_call_opts(band, opts, &o);
  if (rc) return rc;
  CallCtx c;
  DeviceState* st = nullptr;
  rc = resolve_ctx(&o, &c, &st);
  if (rc) return rc;

  const float w_out = ropts->exterior, w_in = ropts->interior;
  const float hx = band->grid.cell_size[0], hy = band->grid.cell_size[1], hz = band->grid.cell_size[2];
  const float wx = 1.0f / (hx * hx), wy = 1.0f / (hy * hy), wz = 1.0f / (hz * hz);
  const WalkGrid g = walk_grid_of(band->grid.cell_count, band->total, band->n_words);
  const float hs[3] = {hx, hy, hz};
  const uint64_t ns[3] = {g.nx, g.ny, g.nz};
  int64_t k_out[3], k_in[3];
  uint64_t k_sum = 0;
  for (int a = 0; a < 3; ++a) {
    k_out[a] = reach(w_out, hs[a], ns[a]);
    k_in[a] = reach(w_in, hs[a], ns[a]);
    k_sum += (uint64_t)std::max(k_out[a], k_in[a]);   // reach is monotone in the width: the larger side's K
  }
  const uint64_t max_sweeps = ropts->max_sweeps ? ropts->max_sweeps : std::min<uint64_t>(2 * k_sum + 8, 0xffffffffull);
  const bool one_reach = memcmp(k_out, k_in, sizeof(k_out)) == 0;

  const uint64_t n_words = g.n_words;
  const uint64_t n_units = (n_words + kWalkUnit - 1) / kWalkUnit;   // below 2^22: a grid has fewer than 2^36 cells
  const uint64_t n_groups = (n_units + kRdGroup - 1) / kRdGroup;
  const unsigned blocks = (unsigned)((n_units + kWalkWaves - 1) / kWalkWaves);
  const size_t b_words = align_up(n_words * 8);
  const int n_arrays = one_reach ? 6 : 7;   // S, F, T1, T2, DE (then C), Coff[, DI]
  char* tmp = nullptr;
  char* ubuf = nullptr;
  BandBlock res;
  M2S_HIP_CHECK(hipMalloc((void**)&tmp, (size_t)n_arrays * b_words));
  auto drop = [&](int code) {
    (void)hipFree(tmp);
    (void)hipFree(ubuf);
    res.free();
    return code;
  };
  auto hip_fail = [&](hipError_t e) { return drop(fail(M2S_ERR_HIP, "HIP error: %s", hipGetErrorString(e))); };
  uint64_t* S = reinterpret_cast<uint64_t*>(tmp);
  uint64_t* Fm = reinterpret_cast<uint64_t*>(tmp + b_words);
  uint64_t* T1 = reinterpret_cast<uint64_t*>(tmp + 2 * b_words);
  uint64_t* T2 = reinterpret_cast<uint64_t*>(tmp + 3 * b_words);
  uint64_t* Cm = reinterpret_cast<uint64_t*>(tmp + 4 * b_words);
  uint64_t* Coff = reinterpret_cast<uint64_t*>(tmp + 5 * b_words);
  uint64_t* DI = one_reach ? Cm : reinterpret_cast<uint64_t*>(tmp + 6 * b_words);
  rc = ensure_capacity(*st, 4096 + 1024 + align_up((size_t)n_units * 4) + align_up((size_t)n_groups * 8));
  if (rc) return drop(rc);
  Arena ws{st->base, st->cap, 0};
  uint64_t* d_hdr = ws.take<uint64_t>(4);      // [0] n_frozen, [1] n_open, [2] a scan's total
  uint32_t* d_flags = ws.take<uint32_t>(kRdBatch);
  uint32_t* unit_cnt = ws.take<uint32_t>(n_units);
  uint64_t* group_sum = ws.take<uint64_t>(n_groups);
  if (!d_hdr || !d_flags || !unit_cnt || !group_sum) return drop(fail(M2S_ERR_HIP, "internal: workspace"));
  const BandDev X = dev_of(band);
  hipStream_t s = c.stream;
  hipError_t e = hipSuccess;
  // a mask's word_off: counts, group sums, their scan (the total to d_hdr[2])
  auto count_and_scan = [&](const uint64_t* mask) {
    hipError_t r = hipMemsetAsync(group_sum, 0, n_groups * 8, s);
    if (r != hipSuccess) return r;
    hipLaunchKernelGGL(k_rd_count, dim3(blocks), dim3(kWalkThreads), 0, s, mask, g, unit_cnt, group_sum);
    hipLaunchKernelGGL((k_scan_tiles<kRdScanThreads, uint64_t>), dim3(1), dim3(kRdScanThreads), 0, s, group_sum, n_groups, d_hdr + 2);
    return hipGetLastError();
  };

  // ---- topology: s, F, C and its index ----
  if (c.timings) e = hipEventRecord(st->ev[0], s);
  if (e == hipSuccess) e = hipMemsetAsync(d_hdr, 0, 32, s);
  if (e != hipSuccess) return hip_fail(e);
  hipLaunchKernelGGL(k_rd_sign, dim3(blocks), dim3(kWalkThreads), 0, s, X, g, S);
  hipLaunchKernelGGL(k_rd_frozen, dim3(blocks), dim3(kWalkThreads), 0, s, X.mask, (const uint64_t*)S, g, Fm, d_hdr);
  dilate(s, blocks, g, k_out, Fm, T1, T2, Cm);
  if (!one_reach) dilate(s, blocks, g, k_in, Fm, T1, T2, DI);
  hipLaunchKernelGGL(k_rd_select, dim3(blocks_for(n_words)), dim3(256), 0, s, (const uint64_t*)Cm,
                     (const uint64_t*)DI, (const uint64_t*)S, n_words, Cm);
  e = hipGetLastError();
  if (e == hipSuccess) e = count_and_scan(Cm);
  uint64_t hdr[3] = {0, 0, 0};
  if (e == hipSuccess) e = hipMemcpyAsync(hdr, d_hdr, 24, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(e);
  const uint64_t n_frozen = hdr[0], n_open = hdr[1], n_cand = hdr[2];
  if (n_cand > g.total) return drop(fail(M2S_ERR_HIP, "internal: %llu candidates on a grid of %llu cells", (unsigned long long)n_cand, (unsigned long long)g.total));
  if (n_cand >= kRdNone)
    return drop(fail(M2S_ERR_BAD_ARG, "%llu candidate cells: the widths reach 2^32 - 1 cells or more (the neighbour table holds 32-bit places)",
                     (unsigned long long)n_cand));
  const size_t b_u = align_up(std::max<uint64_t>(n_cand, 1) * 4), b_meta = align_up(std::max<uint64_t>(n_cand, 1));
  e = hipMalloc((void**)&ubuf, 2 * b_u + align_up(6 * n_cand * 4 + 4) + b_meta);   // two value buffers, the table: 33 bytes per candidate
  if (e != hipSuccess) return hip_fail(e);
  float* u[2] = {reinterpret_cast<float*>(ubuf), reinterpret_cast<float*>(ubuf + b_u)};
  uint32_t* slots = reinterpret_cast<uint32_t*>(ubuf + 2 * b_u);
  uint8_t* meta = reinterpret_cast<uint8_t*>(ubuf + 2 * b_u + align_up(6 * n_cand * 4 + 4));
  RdField fld{Cm, Coff, S, u[0], n_cand};
  hipLaunchKernelGGL(k_rd_offsets, dim3(blocks), dim3(kWalkThreads), 0, s, (const uint64_t*)Cm, g, (const uint32_t*)unit_cnt, (const uint64_t*)group_sum, Coff);
  hipLaunchKernelGGL(k_rd_table, dim3(blocks), dim3(kWalkThreads), 0, s, X, g, (const uint64_t*)Fm, fld, slots, meta, u[0], u[1]);
  e = hipGetLastError();
  if (e == hipSuccess && c.timings) e = hipEventRecord(st->ev[1], s);
  if (e != hipSuccess) return hip_fail(e);

  // ---- the sweeps, kRdBatch of them between two reads of their flags ----
  uint64_t run = 0, sweeps = 0;
  uint32_t converged = n_cand == 0 ? 1u : 0u;   // nothing to sweep: the first sweep changes nothing
  const unsigned sweep_blocks = blocks_for(n_cand);
  while (!converged && run < max_sweeps) {
    const int batch = (int)std::min<uint64_t>(kRdBatch, max_sweeps - run);
    e = hipMemsetAsync(d_flags, 0, kRdBatch * 4, s);
    if (e != hipSuccess) return hip_fail(e);
    for (int b = 0; b < batch; ++b) {
      hipLaunchKernelGGL(k_rd_sweep, dim3(sweep_blocks), dim3(256), 0, s, (const uint32_t*)slots, (const uint8_t*)meta, (const float*)u[(run + b) & 1],
                         u[(run + b + 1) & 1], n_cand, w_out, w_in, hx, hy, hz, wx, wy, wz, d_flags + b);
    }
    uint32_t flags[kRdBatch] = {0, 0, 0, 0};
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(flags, d_flags, kRdBatch * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e);
    for (int b = 0; b < batch; ++b) {
      if (flags[b]) ++sweeps;
      else converged = 1;   // every later sweep finds the same values: it changes nothing either
    }
    run += batch;
  }
  fld.u = u[run & 1];
  if (c.timings) e = hipEventRecord(st->ev[2], s);
  if (e != hipSuccess) return hip_fail(e);

  // ---- the result ----
  uint64_t* R = T1;
  hipLaunchKernelGGL(k_rd_final, dim3(blocks), dim3(kWalkThreads), 0, s, g, (const uint64_t*)Fm, fld, w_out, w_in, R);
  e = hipGetLastError();
  if (e == hipSuccess) e = count_and_scan(R);
  uint64_t n = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&n, d_hdr + 2, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(e);
  if (n > n_cand) return drop(fail(M2S_ERR_HIP, "internal: the result has %llu cells of %llu candidates", (unsigned long long)n, (unsigned long long)n_cand));
  const uint64_t cap = std::max<uint64_t>(n, 1);   // at least one float
  e = res.alloc(n_words, cap);
  if (e != hipSuccess) return hip_fail(e);
  e = hipMemsetAsync(res.dist, 0, 4, s);   // an empty result still has one defined float
  if (e == hipSuccess) e = hipMemcpyAsync(res.mask, R, n_words * 8, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(res.inside, S, n_words * 8, hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return hip_fail(e);
  hipLaunchKernelGGL(k_rd_offsets, dim3(blocks), dim3(kWalkThreads), 0, s, (const uint64_t*)R, g, (const uint32_t*)unit_cnt, (const uint64_t*)group_sum, res.word_off);
  hipLaunchKernelGGL(k_rd_emit, dim3(blocks), dim3(kWalkThreads), 0, s, X, g, (const uint64_t*)Fm, fld, (const uint64_t*)R, (const uint64_t*)res.word_off, res.dist, cap);
  e = hipGetLastError();
  if (e == hipSuccess && c.timings) e = hipEventRecord(st->ev[3], s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(e);
  if (c.timings) {
    float seed = 0.0f, sweep_ms = 0.0f, total = 0.0f;
    (void)hipEventElapsedTime(&seed, st->ev[0], st->ev[1]);
    (void)hipEventElapsedTime(&sweep_ms, st->ev[1], st->ev[2]);
    (void)hipEventElapsedTime(&total, st->ev[0], st->ev[3]);
    memset(c.timings, 0, sizeof(*c.timings));
    c.timings->seed_ms = seed;
    c.timings->distance_ms = sweep_ms;
    c.timings->total_ms = total;
    c.timings->n_units = n;
    c.timings->distance_launches = (uint32_t)run;
  }
  (void)hipFree(tmp);
  (void)hipFree(ubuf);
  if (info_out) {
    info_out->sweeps = (uint32_t)sweeps;
    info_out->converged = converged;
    info_out->reserved = 0;
    info_out->n_frozen = n_frozen;
    info_out->n_open = n_open;
    info_out->n_candidates = n_cand;
  }
  *out = band_adopt(res, band->device, band->grid, n, g.total, n_words, fopts ? fopts->background_outside : w_out, fopts ? fopts->background_inside : w_in);
  return M2S_OK;
}

}  // extern "C"
