// band_fetch.hip.h — the fetch of a band sample's K cell values behind a resident index, shared by band_query.hip (m2s_band_sample /
// m2s_band_raymarch) and band_resample.hip (m2s_band_resample).  Moved here from band_query.hip unchanged; band_query.hip's header comment
// says what the three rounds are and what M2S_BAND_FETCH chooses between.  The arithmetic around the fetch is grid_query.hip.h's prepare /
// combine.  Include it under `#pragma clang fp contract(off)`.  In an unnamed namespace, as band_handle.h's helpers are.
#pragma once
#include "band_handle.h"
#include "grid_query.hip.h"
#include "isosurface.hip.h"

#pragma clang fp contract(off)

namespace m2s {
namespace {

// The K cell values of G prepared samples in three rounds of independent loads (the header comment); support[g] = the active reads of
// sample g, 0 for a sample off the box or with a NaN coordinate.
template <int MODE, int G, bool SIGN>
__device__ __forceinline__ void fetch_rounds(const BandDev& b, const Prep<MODE>* p, float (*v)[Corners<MODE>::K], uint32_t* support) {
  constexpr int K = Corners<MODE>::K;
  constexpr int S = MODE == M2S_SAMPLE_TRILINEAR ? 4 : 1;   // corner c may share the mask word of corner c - S
  bool same[G][K];
  uint64_t mw[G][K], sw[G][K];
  // round 1: the mask (and sign) word of every corner that does not share its lower neighbour's
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int c = 0; c < K; ++c) {
      const uint64_t w = p[g].off[c] >> 6;
      same[g][c] = c >= S && (p[g].off[c >= S ? c - S : 0] >> 6) == w;
      mw[g][c] = 0;
      sw[g][c] = 0;
      if (!same[g][c]) {
        mw[g][c] = b.mask[w];
        if (SIGN) sw[g][c] = b.inside[w];
      }
    }
  uint32_t act[G], ins[G];   // bit c: corner c is active / inside by the sign mask
  uint32_t rank[G][K];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    act[g] = ins[g] = 0;
#pragma unroll
    for (int c = 0; c < K; ++c) {
      if (same[g][c]) { mw[g][c] = mw[g][c >= S ? c - S : 0]; sw[g][c] = sw[g][c >= S ? c - S : 0]; }
      const uint32_t bit = (uint32_t)p[g].off[c] & 63u;
      act[g] |= (uint32_t)((mw[g][c] >> bit) & 1ull) << c;
      if (SIGN) ins[g] |= (uint32_t)((sw[g][c] >> bit) & 1ull) << c;
      rank[g][c] = (uint32_t)__popcll(mw[g][c] & ((1ull << bit) - 1ull));
    }
  }
  // round 2: the list offset of every word with an active corner, once per word
  uint64_t wo[G][K];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int c = 0; c < K; ++c) {
      bool need = (act[g] >> c) & 1u;
#pragma unroll
      for (int f = c + S; f < K; f += S) {   // the corners that take this word's offset from here
        if (!same[g][f]) break;
        need = need || ((act[g] >> f) & 1u);
      }
      wo[g][c] = 0;
      if (!same[g][c] && need) wo[g][c] = b.word_off[p[g].off[c] >> 6];
    }
  // round 3: the values
  const float bg_out = b.bg_out, bg_in_neg = b.bg_in_neg;
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int c = 0; c < K; ++c) {
      if (same[g][c]) wo[g][c] = wo[g][c >= S ? c - S : 0];
      const bool a = (act[g] >> c) & 1u;
      uint64_t at = wo[g][c] + rank[g][c];
      at = at < b.n ? at : 0;   // at < n whenever the index is sound; the guard keeps a broken invariant in bounds
      float x = ((ins[g] >> c) & 1u) ? bg_in_neg : bg_out;
      if (a) x = b.dist[at];
      v[g][c] = x;
    }
    support[g] = p[g].state == 0 ? (uint32_t)__popc(act[g]) : 0u;
  }
}

// The same values corner after corner: mask word, then offset, then value (M2S_BAND_FETCH=1; the measurement's other arm).
template <int MODE, int G, bool SIGN>
__device__ __forceinline__ void fetch_chain(const BandDev& b, const Prep<MODE>* p, float (*v)[Corners<MODE>::K], uint32_t* support) {
  constexpr int K = Corners<MODE>::K;
  const float bg_out = b.bg_out, bg_in_neg = b.bg_in_neg;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    uint32_t hits = 0;
#pragma unroll
    for (int c = 0; c < K; ++c) {
      const uint64_t L = p[g].off[c];
      const uint64_t m = b.mask[L >> 6];
      float x = bg_out;
      if ((m >> (L & 63)) & 1ull) {
        uint64_t at = active_index(b.mask, b.word_off, L);
        at = at < b.n ? at : 0;
        x = b.dist[at];
        ++hits;
      } else if (SIGN) {
        if ((b.inside[L >> 6] >> (L & 63)) & 1ull) x = bg_in_neg;
      }
      v[g][c] = x;
    }
    support[g] = p[g].state == 0 ? hits : 0u;
  }
}

// FORM (M2S_BAND_FETCH): 0 the three rounds, a normal's samples in the larger groups; 1 the per-corner chain; 2 the three rounds, smaller groups.
template <int MODE, int G, bool SIGN, int FORM>
__device__ __forceinline__ void fetch(const BandDev& b, const Prep<MODE>* p, float (*v)[Corners<MODE>::K], uint32_t* support) {
  if (FORM == 1) fetch_chain<MODE, G, SIGN>(b, p, v, support);
  else fetch_rounds<MODE, G, SIGN>(b, p, v, support);
}

template <int MODE, bool SIGN, int FORM>
__device__ __forceinline__ float sample(const GridQuery& q, const BandDev& b, float px, float py, float pz, uint32_t* support) {
  const Prep<MODE> p = prepare<MODE>(q, px, py, pz);
  float v[1][Corners<MODE>::K];
  fetch<MODE, 1, SIGN, FORM>(b, &p, v, support);
  return combine<MODE>(q, p, v[0]);
}

}  // namespace
}  // namespace m2s
