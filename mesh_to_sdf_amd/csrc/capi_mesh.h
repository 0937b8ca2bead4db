// capi_mesh.h — the m2s_mesh handle and the helpers of a call on one, shared by capi.hip (which creates, destroys and drains it and
// runs the distance calls on it) and capi_features.hip (the query features' resident forms).
#pragma once
#include "capi_internal.h"
#include "sample.hip.h"

// Persistent mesh: triangle records + LBVH resident on one device, reusable across calls
// (it also lets one step be split into several slab calls whose all-gathers
// overlap the next slab's compute).  Caches the sign planes of the last grid it was used with.
struct m2s_mesh {
  std::mutex mu;    // the mesh's own state (cached planes, pending timings); taken before the context's lock
  int device = -1;
  int lane = 0;     // context whose spare blocks this mesh recycles
  char* mem = nullptr;
  size_t mem_bytes = 0;
  m2s::DeviceMesh dm{};
  size_t n_tris = 0;
  float build_ms = 0.0f;
  bool plane_valid = false;
  m2s_grid plane_grid{};
  char* plane_mem = nullptr;
  size_t plane_bytes = 0;
  const uint32_t* plane = nullptr;
  hipEvent_t plane_ready = nullptr;   // recorded after the sign planes were built, on plane_stream
  hipStream_t plane_stream = nullptr;
  bool multi_stream = false;          // the planes have been read from a stream other than plane_stream
  struct Pending {
    hipEvent_t a, b;
    uint64_t units;
    uint32_t launches;
  };
  std::vector<Pending> pending;  // dominant-launch event pairs of asynchronous calls, not yet read
  std::vector<hipEvent_t> free_events;
  // durations of asynchronous calls whose events have already been read and recycled (the list above stays bounded
  // however long the mesh lives: completed pairs are folded in here at the start of every asynchronous call)
  double acc_ms = 0.0;
  uint64_t acc_units = 0;
  uint32_t acc_launches = 0;
  int* d_err_async = nullptr;     // device error word of asynchronous calls (inside `mem`), read by m2s_mesh_drain_timings
  bool async_readers = false;     // asynchronous walks may still be reading the sign planes
  // walks of the tree that a later call on ANOTHER stream cannot see as finished (calls on one stream are ordered by it): the last call was
  // asynchronous (tree_last_async), or an asynchronous call was followed by a call on a different stream (tree_async_other); both end with
  // m2s_mesh_drain_timings or a device synchronisation
  bool tree_last_async = false, tree_async_other = false;
  hipStream_t tree_stream = nullptr;
  bool tree_used = false;
  // winding numbers: the nodes' moments (winding.hip NodeMom), made by the first winding call in a block of their own
  char* mom_mem = nullptr;
  hipEvent_t mom_ready = nullptr;     // recorded after the moments were made, on mom_stream
  hipStream_t mom_stream = nullptr;
  // surface sampling: the running sums C of the triangle weights and their strided top (sample.hip SampleTable), made by the first sampling
  // call in a block of their own.  That call synchronises its stream to bring Amax and W to the host, so the block is complete before any
  // later call, on whatever stream, can see it: no ready event is needed.
  char* samp_mem = nullptr;
  m2s::SampleTable samp{};
  uint32_t samp_amax_bits = 0;
  uint64_t samp_W = 0;
};

// capi.hip, where each is described.  All are called with m->mu held.
int remark_leaves(m2s_mesh* m, const m2s::CallCtx& c, uint32_t want);
void reap_pending(m2s_mesh* m, bool wait);
int mesh_call_opts(const m2s_mesh* m, const m2s_opts* opts, m2s_opts* o);
int park_async_events(m2s_mesh* m, m2s::DeviceState& st, uint64_t units, uint32_t launches);
