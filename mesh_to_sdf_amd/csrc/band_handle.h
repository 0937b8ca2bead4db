// band_handle.h — the resident band behind include/m2s.h's `m2s_band`, shared by band_query.hip (m2s_band_create / destroy / info / sample /
// raymarch), band_csg.hip (m2s_band_csg / export / field_info) and the units of the later band calls.  Moved here from band_query.hip unchanged: the handle, its device view and
// the two steps every call on a handle takes with its m2s_opts.  The device view and the helpers are in an unnamed namespace, as
// isosurface.hip.h's are: each translation unit that includes this has its own copy.
#pragma once
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

}  // namespace
}  // namespace m2s
