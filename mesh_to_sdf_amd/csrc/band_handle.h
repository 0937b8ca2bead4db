// band_handle.h — the resident band behind include/m2s.h's `m2s_band`, and the host steps the calls on one share: band_query.hip
// (m2s_band_create / destroy / info / sample / raymarch), band_csg.hip (m2s_band_csg / export / field_info), band_redistance.hip,
// band_filter.hip, band_advect.hip, band_resample.hip and band_components.hip.  Here are the handle and its device view; the argument checks on m2s_opts, m2s_band_field_opts
// and two grids; a grid's cell and word counts; blocks_for; and BandBlock / band_adopt, a result's device arrays while a call fills them
// and the one place that makes them a handle.  Each is a small function a call takes where it has that step: the calls differ in their
// allocations and synchronisations, so nothing here runs a call.  The device view and the helpers are in an unnamed namespace, as
// isosurface.hip.h's are: each translation unit that includes this has its own copy.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/m2s.h"
#include "capi_internal.h"
#include "common.h"

// The handle owns, in device memory: the mask (1 bit per grid point, word L >> 6, bit L & 63), word_off (per mask word:
// the list place of its first active point), [inside] (the sign mask in the mask's layout) and dist (the values in list order, at least
// one float).  Immutable after it is made.
struct m2s_band {
  int device = -1;
  m2s_grid grid{};
  uint64_t n = 0, total = 0, n_words = 0;
  uint64_t device_bytes = 0;   // the arrays' sizes as include/m2s.h states them (the allocation adds alignment only)
  char* block = nullptr;       // one allocation: mask, word_off, [inside], dist
  char* block2 = nullptr;      // m2s_band_resample's result: dist in an allocation of its own, made once the count is known
  const uint64_t* mask = nullptr;
  const uint64_t* word_off = nullptr;
  const uint64_t* inside = nullptr;
  const float* dist = nullptr;
  float bg_out = 0.0f, bg_in = 0.0f;
};

namespace m2s {
namespace {

struct BandDev {
  const uint64_t* mask;
  const uint64_t* word_off;
  const uint64_t* inside;   // nullptr: no sign mask, every inactive cell is outside
  const float* dist;        // max(n, 1) floats
  uint64_t n;
  float bg_out, bg_in_neg;  // +background_outside, -background_inside
};

BandDev dev_of(const m2s_band* h) { return BandDev{h->mask, h->word_off, h->inside, h->dist, h->n, h->bg_out, -h->bg_in}; }

// The m2s_opts fields no band call takes.
int band_opts_args(const m2s_opts* opts, const char* what) {
  if (!opts) return 0;
  if (opts->algorithm != 0 || opts->x_begin != 0 || opts->x_end != 0)
    return fail(M2S_ERR_BAD_ARG, "m2s_opts.algorithm / x_begin / x_end must be 0 for %s", what);
  if (opts->struct_size >= sizeof(m2s_opts) && (opts->x_period != 0 || opts->n_peer_out != 0 || opts->peer_out))
    return fail(M2S_ERR_BAD_ARG, "m2s_opts.x_period / peer_out must be 0 for %s", what);
  if (opts->mem_kind != M2S_MEM_HOST && opts->mem_kind != M2S_MEM_DEVICE) return fail(M2S_ERR_BAD_ARG, "bad mem_kind");
  return 0;
}

bool good_background(float v) { return v >= 0.0f && std::isfinite(v); }

// The backgrounds a call may take for its result; NULL is the call's default.
int band_field_opts_args(const m2s_band_field_opts* fopts) {
  if (!fopts) return 0;
  if (fopts->struct_size != sizeof(m2s_band_field_opts)) return fail(M2S_ERR_BAD_ARG, "m2s_band_field_opts.struct_size is not sizeof(m2s_band_field_opts)");
  if (!good_background(fopts->background_outside) || !good_background(fopts->background_inside))
    return fail(M2S_ERR_BAD_ARG, "the backgrounds (%g outside, %g inside) must be >= 0 and finite", (double)fopts->background_outside,
                (double)fopts->background_inside);
  return 0;
}

// first_cell, cell_size and cell_count agree in every bit.
bool band_same_grid(const m2s_grid& a, const m2s_grid& b) {
  return memcmp(a.first_cell, b.first_cell, sizeof(a.first_cell)) == 0 && memcmp(a.cell_size, b.cell_size, sizeof(a.cell_size)) == 0 &&
         memcmp(a.cell_count, b.cell_count, sizeof(a.cell_count)) == 0;
}

// A grid's cells and the mask words that hold them; `noun` names the grid in the message.
int band_grid_cells(const m2s_grid* grid, const char* noun, uint64_t* total, uint64_t* n_words) {
  const uint64_t nx = grid->cell_count[0], ny = grid->cell_count[1], nz = grid->cell_count[2];
  const uint64_t nyz = ny * nz;
  if (nyz / ny != nz) return fail(M2S_ERR_BAD_ARG, "the %s has 2^36 or more cells", noun);
  *total = nyz * nx;
  if (*total / nx != nyz || *total >= ((uint64_t)1 << 36)) return fail(M2S_ERR_BAD_ARG, "the %s has 2^36 or more cells", noun);
  *n_words = (*total + 63) / 64;
  return 0;
}

constexpr uint64_t kMaxBlocks = 1u << 20;   // beyond 2^28 lanes the grid-stride loops take over
unsigned blocks_for(uint64_t n) { return (unsigned)std::min<uint64_t>(kMaxBlocks, (n + 255) / 256); }

// Options of a query on a handle: its device unless the caller names the same one (as a persistent mesh's calls).
int band_call_opts(const m2s_band* h, const m2s_opts* opts, m2s_opts* o) {
  *o = m2s_opts{};
  if (opts) memcpy(o, opts, (opts->struct_size >= sizeof(m2s_opts)) ? sizeof(m2s_opts) : (size_t)M2S_OPTS_V1_SIZE);
  else o->device = -1;
  if (o->device < 0) o->device = h->device;
  if (o->device != h->device) return fail(M2S_ERR_BAD_ARG, "the band lives on device %d, the call asked for %d", h->device, o->device);
  if (!opts) o->synchronous = 1;
  return 0;
}

// The device arrays of a result while a call fills them.  One allocation (mask, word_off, [inside], dist), or m2s_band_resample's two: the
// index arrays, then the values once their count is known.  cap: the floats of dist, at least one (a lane's guarded read needs an address).
struct BandBlock {
  char* block = nullptr;
  char* block2 = nullptr;
  uint64_t* mask = nullptr;
  uint64_t* word_off = nullptr;
  uint64_t* inside = nullptr;
  float* dist = nullptr;

  hipError_t alloc(uint64_t n_words, uint64_t cap, bool with_inside = true) {
    const size_t b_words = align_up(n_words * 8), b_index = (with_inside ? 3 : 2) * b_words;
    const hipError_t e = hipMalloc((void**)&block, b_index + align_up(cap * 4));
    if (e == hipSuccess) {
      index_at(b_words, with_inside);
      dist = reinterpret_cast<float*>(block + b_index);
    }
    return e;
  }
  hipError_t alloc_index(uint64_t n_words) {
    const size_t b_words = align_up(n_words * 8);
    const hipError_t e = hipMalloc((void**)&block, 3 * b_words);
    if (e == hipSuccess) index_at(b_words, true);
    return e;
  }
  hipError_t alloc_values(uint64_t cap) {
    const hipError_t e = hipMalloc((void**)&block2, align_up(cap * 4));
    if (e == hipSuccess) dist = reinterpret_cast<float*>(block2);
    return e;
  }
  void free() {
    (void)hipFree(block2);
    (void)hipFree(block);
  }

 private:
  void index_at(size_t b_words, bool with_inside) {
    mask = reinterpret_cast<uint64_t*>(block);
    word_off = reinterpret_cast<uint64_t*>(block + b_words);
    inside = with_inside ? reinterpret_cast<uint64_t*>(block + 2 * b_words) : nullptr;
  }
};

// The handle that owns a filled BandBlock.  device_bytes is include/m2s.h's formula: 16 bytes per mask word, 8 more with a sign mask, 4 per cell.
m2s_band* band_adopt(const BandBlock& k, int device, const m2s_grid& grid, uint64_t n, uint64_t total, uint64_t n_words, float bg_out, float bg_in) {
  m2s_band* h = new m2s_band();
  h->device = device;
  h->grid = grid;
  h->n = n;
  h->total = total;
  h->n_words = n_words;
  h->device_bytes = n_words * (k.inside ? 24 : 16) + n * 4;
  h->block = k.block;
  h->block2 = k.block2;
  h->mask = k.mask;
  h->word_off = k.word_off;
  h->inside = k.inside;
  h->dist = k.dist;
  h->bg_out = bg_out;
  h->bg_in = bg_in;
  return h;
}

}  // namespace
}  // namespace m2s
