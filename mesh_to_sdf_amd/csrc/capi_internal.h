// capi_internal.h — per-device state and call context shared by the C-ABI translation units
// (capi.hip: contexts, staging, the distance path and the m2s_mesh lifecycle; capi_features.hip: closest points, winding numbers,
// rays, surface sampling, voxelization, narrow bands; capi_io.hip: container encode/decode, cell ordering, instance merge, grid
// queries).  The m2s_mesh handle itself is in capi_mesh.h.
#pragma once
#include <cstdio>
#include <functional>
#include <mutex>
#include <vector>

#include "../../include/m2s.h"
#include "common.h"

namespace m2s {

struct DeviceState {
  std::mutex mu;   // held by an entry point for the whole call (CallCtx::lock); one context per (device, lane)
  // Scratch of the call in progress.  It belongs to the STREAM the call is enqueued on (resolve_ctx selects it):
  // calls on one stream are ordered by the stream and share one block, calls on different streams get different
  // blocks, so asynchronous calls on two streams (the x-pieces of a sharded grid) may overlap on the device.
  char* base = nullptr;
  size_t cap = 0;
  size_t warmed_cap = 0;   // m2s_warmup: capacity of the workspace block it has already touched
  struct Scratch {
    hipStream_t stream = nullptr;
    char* base = nullptr;
    size_t cap = 0;
    uint64_t last_use = 0;
  };
  static constexpr int SCRATCH = 4;
  Scratch scratch[SCRATCH];
  int n_scratch = 0, active = -1;
  uint64_t tick = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // [5]: start of early sign planes (side_stream2)
  hipStream_t side_stream2 = nullptr;   // one-shot Raycast grid calls: the sign planes, from the input-order records, beside build and seeds
  bool early_planes = false;            // this call's planes were launched on side_stream2 (ev[5] .. ev[2])
  // Raycast sign planes depend on the mesh only: they are built on `side_stream` while the caller's stream runs the seed
  // passes and cut lists; the dominant launch waits for ev[2], which is then recorded on the side stream.
  hipStream_t side_stream = nullptr;
  hipEvent_t fork_ev = nullptr;
  hipEvent_t planes_done = nullptr;   // ev[2] while a call's planes are in flight on the side stream, else nullptr
  // one-shot grid calls also run the jump-flooding seed passes on the side stream, beside the sort / hierarchy of the build
  // (they only need the input-order centroids): the lattice, and the event recorded after the last pass
  SeedLattice raw_seeds;
  hipEvent_t seeds_done = nullptr, seeds_fork = nullptr;
  bool have_raw_seeds = false;
  hipEvent_t qlat_done = nullptr;     // ... and its bounding box + seed-lattice description are enqueued
  hipEvent_t qprep_done = nullptr;    // one-shot query calls: the query preparation (sort, packets) on the side stream has finished
  int* h_err = nullptr;  // pinned
  char* spare_mesh = nullptr;  // last destroyed m2s_mesh block, recycled by the next m2s_mesh_create
  size_t spare_mesh_bytes = 0;
  char* spare_plane = nullptr;  // sign-plane block of the last destroyed m2s_mesh (hipFree / hipMalloc cost 0.2 + 0.1 ms per mesh)
  size_t spare_plane_bytes = 0;
  std::vector<hipEvent_t> timing_events;   // timing-enabled events handed back by destroyed meshes
  // host-pointer calls: pinned ring + copy stream for the pipelined D2H of the result (capi.hip)
  static constexpr int RING = 3;
  char* ring[RING] = {nullptr, nullptr, nullptr};
  size_t ring_bytes = 0;
  hipStream_t copy_stream = nullptr;
  std::vector<hipEvent_t> piece_events;   // M2S_PEER_PUSH: piece i walked / last push done (no timing)
};

struct CallCtx {
  int device = -1;
  int mem_kind = M2S_MEM_HOST;
  int algorithm = 0;
  bool sync = true;
  hipStream_t stream = nullptr;
  m2s_timings* timings = nullptr;
  uint64_t x_begin = 0, x_end = 0;
  int lane = 0;
  PeerOut peers{};                       // m2s_opts.peer_out (grid path, device memory)
  int peer_mode = 0;
  std::unique_lock<std::mutex> lock;     // the context's lock, taken by resolve_ctx, released when the CallCtx dies
};

extern std::mutex g_mu;                  // guards the table of contexts only; every context has its own lock
DeviceState* find_state(int device, int lane);   // creates the context if needed; does NOT lock it
void clear_error();
int fail(int code, const char* fmt, ...);
int resolve_ctx(const m2s_opts* opts, CallCtx* c, DeviceState** st);
int ensure_capacity(DeviceState& s, size_t bytes);
int select_scratch(DeviceState& s, hipStream_t stream);   // called by resolve_ctx
void release_scratch(DeviceState& s);                     // device must be idle
// Pageable host arrays <-> device at PCIe speed through the pinned ring (capi.hip); complete on return.
int staged_h2d(DeviceState& st, hipStream_t stream, char* d_dst, const char* h_src, size_t bytes);
int staged_d2h(DeviceState& st, hipStream_t stream, char* h_dst, const char* d_src, size_t bytes);
int staged_d2h_to_file(DeviceState& st, hipStream_t stream, FILE* f, const char* d_src, size_t bytes);   // M2S_ERR_IO on a short write
inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// Steps of a mesh call (capi.hip) that the feature entry points (capi_features.hip) take as the distance calls do.
int check_mesh_args(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes, int topology);
struct StagedMesh {
  const float* d_verts = nullptr;
  const void* d_indices = nullptr;
};
// Copies the mesh to the device when the caller passed host pointers.
int stage_mesh(Arena& ws, const CallCtx& c, const float* vertices, size_t n_vertices, const void* indices, size_t n_indices,
               int index_bytes, StagedMesh* out);
// The grid, and the x-slab `opts` names (NULL: the whole grid), into `g`; *slab_cells = the cells of the slab.
int fill_grid_params(const m2s_grid* grid, const m2s_opts* opts, GridParams* g, size_t* slab_cells);
// Ends a synchronous call (an asynchronous one returns at once): waits, fills `t` from ev[0] .. ev[4], reports the device's error word.
// (capi.hip's own calls may leave had_seed_event out: its definition defaults it to false.)
int finish_call(const CallCtx& c, DeviceState& st, int* d_err, m2s_timings* t, size_t n_tris, size_t n_units, bool had_sign,
                bool had_seed_event);

// Grid queries (capi_io.hip), shared with the band queries (band_query.hip).
// grid_query_args: the grid, the sample options and the m2s_opts fields a grid query does not take, into `q` and `mode`; everything
// include/m2s.h lists as M2S_ERR_BAD_ARG for them that needs no device.  `grid` is not NULL.
int grid_query_args(const m2s_grid* grid, const m2s_sample_opts* so, bool ray, const m2s_opts* opts, GridQuery* q, int* mode);
// run_query runs `launch(stream)` with every io[i].dev on the device: host data is staged through the workspace, outputs copied back.
struct QueryIo {
  const void* src;      // caller's pointer
  size_t bytes;
  bool output;
  char* dev = nullptr;  // what the kernel sees
};
int run_query(const m2s_opts* opts, QueryIo* io, int n_io, uint64_t n_units, const std::function<int(hipStream_t)>& launch);

}  // namespace m2s
