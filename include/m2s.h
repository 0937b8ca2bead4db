/* m2s.h — C ABI of the MI355X-native hot path of Azkellas/mesh_to_sdf.
 *
 * Drop-in boundary.  The reference has no FFI layer of its own; its public surface for this
 * path is two generic Rust functions (paths relative to /root/reference/mesh_to_sdf/src):
 *
 *   pub fn generate_sdf<V: Point, I: Copy + Into<u32> + Sync + Send>(
 *       vertices: &[V], indices: Topology<I>, query_points: &[V],
 *       acceleration_method: AccelerationMethod) -> Vec<f32>              lib.rs:291-300
 *   pub fn generate_grid_sdf<V: Point + Sync + Send, I: ...>(
 *       vertices: &[V], indices: Topology<I>, grid: &Grid<V>,
 *       sign_method: SignMethod) -> Vec<f32>                              generate/grid.rs:265-274
 *
 * The entry points below are exactly what a Rust `extern "C"` block bound behind those two
 * signatures needs (see INTEGRATION.md for the shim): plain pointers and sizes, packed
 * xyz float triples (`[f32; 3]` is zero-copy), u16 or u32 indices, enums as ints.
 *
 * Semantics.  Distances are the reference's f32 arithmetic (geo.rs:70-138 closest point,
 * point.rs:99-126 operation order, no FMA contraction) minimised over ALL triangles, i.e. what
 * generate_sdf(AccelerationMethod::None(..)) returns and what the reference's own test
 * generate/grid.rs:693-724 asserts the grid path to equal.  (The reference's grid path is a
 * heap-ordered label propagation whose result depends on the thread count and is >= this
 * minimum on <0.5% of cells; see DESIGN.md "Exact vs propagation".)
 *
 * Threading: synchronous and re-entrant.  The library keeps one context (workspace, streams, events) per
 * (device, m2s_opts.lane); an entry point holds only ITS context's lock, so calls on different devices — or on
 * different lanes of one device — run concurrently from different host threads (m2s_generate_grid_sdf_multi does
 * exactly that, one thread per device).  Calls on the same (device, lane) are serialised; the work they enqueue is
 * not: asynchronous calls (m2s_opts.synchronous = 0) on different streams use separate scratch blocks and may
 * overlap on the device.
 *
 * Limits (validated, M2S_ERR_BAD_ARG): n_vertices < 2^31, n_indices < 3 * 2^31, at most 2^25 triangles per mesh
 * (32-bit byte offsets into the 96-byte triangle records), n_queries < 2^32 - 64 per call, every cell_count < 2^31
 * and every product of two cell counts < 2^32 (grid lines per face are counted in 32 bits).
 *
 * Non-finite QUERY coordinates (m2s_generate_sdf): with None / Bvh and SignMethod::Raycast the result is +f32::MAX, as in the
 * reference (every distance is NaN and f32::min drops it, default.rs:47; no ray hits); with SignMethod::Normal the call returns
 * M2S_ERR_NAN where the reference panics (lib.rs:257).  Rtree / RtreeBvh: the reference measures the distance to whichever
 * triangle rstar's nearest_neighbor returns for a NaN / inf point — unspecified by that crate — so the value for such a query
 * is unspecified here too (+f32::MAX for RtreeBvh today); the other queries of the call are unaffected.
 */
#ifndef M2S_H
#define M2S_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M2S_VERSION_MAJOR 0
#define M2S_VERSION_MINOR 5   /* 0.5: + m2s_tuning_set, m2s_tuning_describe (and, additive within 0.5: m2s_sample_surface, m2s_mesh_sample_surface, m2s_voxelize, m2s_mesh_voxelize, m2s_narrow_band_sdf, m2s_mesh_narrow_band_sdf, m2s_band_isosurface, m2s_band_create / destroy / info / sample / raymarch, m2s_band_csg, m2s_band_export, m2s_band_field_info, m2s_band_redistance); additive within 0.5 too: m2s_band_filter, m2s_band_resample, m2s_band_advect; 0.4: + m2s_warmup, m2s_peer_bandwidth, m2s_balanced_slabs, M2S_PART_ADAPTIVE, m2s_multi_opts.partition_used / slabs (additive) */

/* Return codes.  The reference panics where this ABI returns a negative code; the Rust shim
 * turns a negative code back into panic!(m2s_last_error()). */
#define M2S_OK 0
#define M2S_ERR_BAD_ARG (-1)     /* null pointer / bad enum / vertex index out of range (reference: index panic) */
#define M2S_ERR_NAN (-2)         /* "NaN distance" — lib.rs:257 expect(), Normal sign only; m2s_grid_isosurface: a NaN or +-inf grid value */
#define M2S_ERR_EMPTY_MESH (-3)  /* AccelerationMethod::Rtree on a mesh with no triangle — generic/rtree.rs:117 unwrap() */
#define M2S_ERR_HIP (-4)         /* HIP runtime failure, or no HIP device / kernels not loadable */

/* Topology — lib.rs:151-167.  List: consecutive triples, a trailing partial triple is dropped
 * (itertools::tuples).  Strip: sliding window, NO winding flip on odd triangles (lib.rs:188-191).
 * indices == NULL means 0..n_vertices (Topology::*(None)). */
enum m2s_topology { M2S_TRIANGLE_LIST = 0, M2S_TRIANGLE_STRIP = 1 };

/* SignMethod — lib.rs:204-216 (default Raycast). */
enum m2s_sign_method { M2S_SIGN_RAYCAST = 0, M2S_SIGN_NORMAL = 1 };

/* AccelerationMethod — lib.rs:224-239 (default RtreeBvh).  It selects the SIGN RULE, which is
 * observable, not just a speed path:
 *   NONE  + Raycast: parity of +X hits over all triangles          generic/default.rs:32-38,65-72
 *   NONE  + Normal : compare_distances fold over all triangles     generic/default.rs:40-59
 *   BVH   + Raycast: best of three +X/+Y/+Z rays from the query    generic/bvh.rs:106-141
 *   BVH   + Normal : compare_distances fold                        generic/bvh.rs:82-94
 *   RTREE          : normal sign of the single nearest triangle    generic/rtree.rs:113-125 (sign_method ignored)
 *   RTREE_BVH      : nearest distance + best of three rays         generic/rtree_bvh.rs:123-173 (sign_method ignored)
 */
enum m2s_accel { M2S_ACCEL_NONE = 0, M2S_ACCEL_BVH = 1, M2S_ACCEL_RTREE = 2, M2S_ACCEL_RTREE_BVH = 3 };

/* Grid<V> — grid.rs:30-37: centre of the first cell, cell size (may differ per axis, may be
 * negative), cell count.  Output index of cell (x,y,z) is z + y*nz + x*ny*nz (grid.rs:122-124). */
typedef struct m2s_grid {
  float first_cell[3];
  float cell_size[3];
  uint64_t cell_count[3];
} m2s_grid;

/* Where the data pointers of a call live. */
enum m2s_mem_kind {
  M2S_MEM_HOST = 0,   /* vertices/indices/queries/out are host pointers (the drop-in case; H2D/D2H inside the call) */
  M2S_MEM_DEVICE = 1  /* all four are device pointers on `device`; nothing crosses PCIe */
};

/* Phase timings of the last call, milliseconds, measured with HIP events on the call's stream
 * (the reference logs the same three phases, generate/grid.rs:303-307,342-346,369-373). */
typedef struct m2s_timings {
  float accel_build_ms;  /* topology flatten + triangle records + LBVH */
  float sign_ms;         /* grid-line ray parity planes (Raycast grid path) */
  float distance_ms;     /* nearest-triangle search (+ fused sign resolve) — the dominant kernel's launch */
  float total_ms;        /* first kernel to last kernel, device side */
  float seed_ms;         /* grid path: what precedes the dominant launch besides the build — jump-flooding seed lattice
                            (one triangle per packet brick) and the cut lists (k_cut).  Closest-point calls: the first pass (the
                            distance walk whose results seed k_closest), included in their distance_ms */
  float reserved_f;
  uint64_t n_triangles;
  uint64_t n_units;      /* voxels or queries produced by this call */
  uint32_t distance_launches;  /* number of launches of the dominant kernel in this call */
  uint32_t reserved;
} m2s_timings;

/* Optional per-call options; pass NULL for defaults.  Set struct_size = sizeof(m2s_opts). */
typedef struct m2s_opts {
  uint32_t struct_size;
  int32_t device;       /* HIP device ordinal; -1 = current device */
  void* stream;         /* hipStream_t to enqueue on; NULL = the library's own stream for that device */
  int32_t mem_kind;     /* enum m2s_mem_kind */
  int32_t algorithm;    /* 0 = default (LBVH); 1 = brute force over all triangles (validation / AccelerationMethod::None) */
  /* Grid path only: compute the x-slab [x_begin, x_end) of cells (cell axis 0 is the slowest
   * axis, so a slab is one contiguous range of the output).  x_end == 0 means the whole grid.
   * `out` always addresses the WHOLE grid; only the slab's range is written. */
  uint64_t x_begin;
  uint64_t x_end;
  m2s_timings* timings; /* filled when non-NULL (forces a stream sync before returning) */
  int32_t synchronous;  /* device-memory calls: 1 (default when opts==NULL) = sync before return; 0 = leave work enqueued */
  int32_t stream_mode;  /* 0: stream == NULL selects the library's own (non-blocking) stream;
                           1: `stream` is used exactly as given, and NULL means the device's default (null) stream —
                              needed by callers whose "current stream" IS the default stream (torch does this) and who
                              order other work (e.g. an RCCL collective) after this call without a host sync */
  /* ---- fields below exist when struct_size >= sizeof(m2s_opts) of version 0.2 (M2S_OPTS_V1_SIZE bytes = version 0.1) ---- */
  int32_t lane;         /* context lane on `device`, 0 .. M2S_MAX_LANES-1: calls on different lanes do not serialise (Threading) */
  uint32_t n_peer_out;  /* grid path, device memory: number of entries of peer_out (<= M2S_MAX_PEERS) */
  float* const* peer_out; /* whole-grid buffers like `out`, on OTHER devices (peer access enabled: same process after
                             hipDeviceEnablePeerAccess, or mapped from another process with m2s_ipc_open) or on this one:
                             the x-slab this call computes is written to each of them as well, so that after every shard's
                             call each buffer holds the whole grid with no separate all-gather */
  int32_t peer_mode;    /* how: 0 = M2S_PEER_PUSH, one copy kernel per slab piece after its walk, 16 B per lane = 1 KiB per wave
                                    store instruction (xGMI-friendly request size; the default);
                                1 = M2S_PEER_STORE, the walk's epilogue stores every value to every peer itself (no extra pass over
                                    the slab, but 16-byte runs: a 4x4x4 brick row);
                                2 = M2S_PEER_TRAIL, one walk over the whole slab whose packets count themselves per unit of 8
                                    x-layers, and a copy kernel beside it that pushes every unit (1 KiB per wave store) as soon as
                                    it is complete: no pieces, and only the last unit's push is exposed */
  uint32_t x_period;    /* grid path, device memory; 0 = [x_begin, x_end) is one contiguous slab.  Otherwise the call owns the CHUNKS
                           [x_begin + j * x_period, x_end + j * x_period), j = 0, 1, ... up to the end of the grid: interleaved slabs.
                           Shards that take the chunks r and N + r of 2N balance far better than N contiguous slabs when the
                           cost of a layer varies along x (the deep interior of a body is the expensive part).  x_end - x_begin must
                           be a power of two and a multiple of 4 packet bricks (16 layers for cubic cells), x_period a multiple of it */
} m2s_opts;
#define M2S_OPTS_V1_SIZE 56
#define M2S_MAX_LANES 16
#define M2S_MAX_PEERS 15
enum m2s_peer_mode { M2S_PEER_PUSH = 0, M2S_PEER_STORE = 1, M2S_PEER_TRAIL = 2 };

/* generate_sdf — lib.rs:291-311.
 * vertices: n_vertices packed xyz f32.  indices: n_indices values of index_bytes (2 or 4) each, or NULL.
 * queries: n_queries packed xyz.  out: n_queries f32.  *n_out (optional) receives the number of
 * distances written: n_queries, or 0 for RTREE_BVH on a mesh without triangles (the reference
 * returns an empty Vec there, generic/rtree_bvh.rs:104-106). */
int m2s_generate_sdf(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes,
                     int topology, const float* queries, size_t n_queries, int accel, int sign_method, float* out,
                     size_t* n_out, const m2s_opts* opts);

/* generate_grid_sdf — generate/grid.rs:265-378.  out: cell_count[0]*[1]*[2] f32, caller owned.
 * Semantics: the EXACT minimum over all triangles (what generate/grid.rs:693-724 asserts the grid path to equal).  SURVEY.md §8(b)
 * sketched a `semantics` argument selecting the reference's label propagation (generate/grid.rs:495-558) instead; it is
 * deliberately absent: that output depends on rayon::current_num_threads(), is never below the exact minimum and exceeds it on
 * 0.03 % (512^3) to 59 % (1 M triangles in 128^3) of the cells — there is no one result to reproduce. */
int m2s_generate_grid_sdf(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices,
                          int index_bytes, int topology, const m2s_grid* grid, int sign_method, float* out,
                          const m2s_opts* opts);

/* ---- multi-GPU generate_grid_sdf (SURVEY.md 8b "device list", 8e) -----------------------------------------
 * generate/grid.rs:265-274 is the one signature a caller of the reference has; this is the same call spread over the
 * GPUs of one node from ONE process: one host thread per listed device, the mesh replicated (every device builds its own
 * LBVH: the build is sub-millisecond and needs no exchange), the grid cut into contiguous x-slabs (cell axis 0 is the
 * slowest axis of the output, grid.rs:122-124, so a slab is one contiguous range), sign planes marked per device for
 * the whole grid (hits are slab independent).  No data-path collective:
 *   mem_kind == M2S_MEM_HOST   vertices / indices / outs[0] are host pointers.  Every device uploads the mesh and streams
 *                              its finished slab straight into the caller's array over its own PCIe link (pinned ring,
 *                              pipelined with the compute) — the drop-in form behind generate_grid_sdf's Vec<f32>.
 *   mem_kind == M2S_MEM_DEVICE vertices / indices live on devices[0]; outs[k] is a whole-grid buffer on devices[k].
 *                              On return EVERY buffer holds the whole grid:
 *                                exchange M2S_XCHG_PEER  each device writes its slab into all buffers itself over xGMI
 *                                                        (hipDeviceEnablePeerAccess; m2s_opts.peer_out / peer_mode);
 *                                exchange M2S_XCHG_RCCL  ncclAllGather from librccl (loaded on first use), in place;
 *                                exchange M2S_XCHG_NONE  nothing: buffer k holds slab k only;
 *                                exchange M2S_XCHG_AUTO  PEER when every pair of devices can access each other, else RCCL.
 * `devices` may name a device more than once (two shards on one GPU: how the path is tested on a 1-GPU box).
 * Errors as m2s_generate_grid_sdf; the first failing shard's code is returned. */
enum m2s_exchange { M2S_XCHG_AUTO = 0, M2S_XCHG_PEER = 1, M2S_XCHG_RCCL = 2, M2S_XCHG_NONE = 3 };
typedef struct m2s_multi_opts {
  uint32_t struct_size;
  int32_t n_devices;        /* number of shards; 0 = one per visible device */
  const int32_t* devices;   /* n_devices HIP ordinals; NULL = 0 .. n_devices-1 */
  int32_t mem_kind;         /* enum m2s_mem_kind */
  int32_t exchange;         /* enum m2s_exchange; device memory only */
  int32_t peer_mode;        /* enum m2s_peer_mode for M2S_XCHG_PEER */
  int32_t algorithm;        /* as m2s_opts.algorithm */
  m2s_timings* timings;     /* optional, n_devices entries: per-shard phase timings */
  float* wall_ms;           /* optional: host wall time of the whole call */
  int32_t* exchange_used;   /* optional: the exchange that ran (M2S_XCHG_PEER / RCCL / NONE) */
  /* ---- fields below exist when struct_size >= M2S_MULTI_OPTS_V2_SIZE (version 0.2; M2S_MULTI_OPTS_V1_SIZE = without) ---- */
  int32_t partition;        /* enum m2s_partition.  A caller whose struct ends before this field gets M2S_PART_CONTIGUOUS. */
  int32_t reserved;
  /* ---- fields below exist when struct_size >= sizeof(m2s_multi_opts) (version 0.3) ---- */
  int32_t* partition_used;  /* optional: M2S_PART_CONTIGUOUS / INTERLEAVED / ADAPTIVE as it ran */
  uint64_t* slabs;          /* optional, 3 * n_devices entries: x_begin, x_end, x_period of every shard as it ran (m2s_opts meaning) */
} m2s_multi_opts;
#define M2S_MULTI_OPTS_V1_SIZE 56
#define M2S_MULTI_OPTS_V2_SIZE 64
/* How the grid is cut.  CONTIGUOUS: shard k computes one x-slab.  INTERLEAVED: shard k computes the chunks k and n + k of 2n
 * (m2s_interleaved_slab): the cost of a layer varies along x — the deep interior of a body is the expensive part — and
 * contiguous slabs leave the middle shards with 30 % more work than the outer ones.  AUTO: interleaved for device-resident
 * results that are exchanged (PEER / RCCL) where the grid allows it, contiguous otherwise (host results stream out slab by slab;
 * with M2S_XCHG_NONE buffer k holds m2s_slab_bounds(nx, n, k)).  ADAPTIVE: contiguous slabs of equal COST — the library keeps,
 * per (grid, mesh size, sign method, shard count), the slab boundaries that m2s_balanced_slabs derives from the per-shard
 * times of the previous call; the first call uses even slabs.  For callers that repeat a call (a time loop): the cost of a
 * layer is not known in advance, but it can be measured.  `slabs` reports what ran. */
enum m2s_partition { M2S_PART_AUTO = 0, M2S_PART_CONTIGUOUS = 1, M2S_PART_INTERLEAVED = 2, M2S_PART_ADAPTIVE = 3 };
int m2s_generate_grid_sdf_multi(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices,
                                int index_bytes, int topology, const m2s_grid* grid, int sign_method, float* const* outs,
                                const m2s_multi_opts* opts);
/* generate_sdf over several GPUs (lib.rs:291-300 is still the one signature a caller has).  Shard k computes the contiguous query
 * range m2s_slab_bounds(n_queries, n, k): every query depends only on the mesh.  mem_kind / devices / exchange / timings /
 * wall_ms / exchange_used as for the grid call; partition and peer_mode are ignored.
 *   M2S_MEM_HOST    outs[0] = the caller's array of n_queries floats; every device returns its range over its own PCIe link.
 *   M2S_MEM_DEVICE  vertices, indices and queries lie on devices[0]; outs[k] = n_queries floats on devices[k]; on return EVERY
 *                   buffer holds all distances (M2S_XCHG_PEER: each shard copies its finished range into the other buffers itself
 *                   over xGMI and the other devices read the inputs where they lie; M2S_XCHG_RCCL: inputs replicated by peer
 *                   copies, ranges gathered by ncclAllGather / ncclBroadcast; M2S_XCHG_NONE: buffer k holds range k only).
 * *n_out (optional): n_queries, or 0 for RTREE_BVH on a mesh without triangles, as m2s_generate_sdf. */
int m2s_generate_sdf_multi(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes,
                           int topology, const float* queries, size_t n_queries, int accel, int sign_method, float* const* outs,
                           size_t* n_out, const m2s_multi_opts* opts);
/* Contiguous range [x_begin, x_end) of shard k out of n over nx units (x-layers, queries): sizes differ by at most one. */
void m2s_slab_bounds(uint64_t nx, int n, int k, uint64_t* x_begin, uint64_t* x_end);
/* Slab boundaries of equal cost.  prev_bounds[0 .. n] (0 = prev_bounds[0] <= ... <= prev_bounds[n] = nx) are the contiguous slabs of a
 * previous call and cost[k] >= 0 what shard k spent on its slab (any unit; leave out what every shard repeats, e.g. the LBVH
 * build).  With the cost density taken as constant inside every previous slab, new_bounds[0 .. n] cuts [0, nx) into n slabs of
 * equal cost, every boundary a multiple of `unit` layers (a packet brick: 4 for cubic cells; 0 = 1) and every slab at least one unit
 * (even slabs when nothing was measured or there are fewer units than shards).  Host-only, deterministic: every rank of a
 * multi-process run computes the same boundaries from the same gathered costs. */
int m2s_balanced_slabs(uint64_t nx, int n, uint64_t unit, const uint64_t* prev_bounds, const float* cost, uint64_t* new_bounds);
/* The balanced partition: shard k takes the chunks k and n + k of 2n (m2s_opts.x_begin / x_end / x_period) when the grid allows
 * it — returns 1 — else its contiguous slab with *x_period = 0 — returns 0. */
int m2s_interleaved_slab(const m2s_grid* grid, int n, int k, uint64_t* x_begin, uint64_t* x_end, uint64_t* x_period);

/* What the links give: the copy kernel of M2S_PEER_PUSH (16 B per lane, 1 KiB per wave store instruction) writes the first n_cells
 * floats of `src` (on `device`; -1 = current) into each of the n_peers buffers (peer-mapped device memory, as m2s_opts.peer_out) —
 * first one peer at a time (gbps_each[k], optional), then all peers in one launch (*gbps_all, optional: the sum over the links).
 * GB/s of payload, best of three timed launches per figure.  xGMI is point-to-point, so gbps_each is a per-link number and
 * gbps_all / n_peers shows what a link keeps when all are busy: together they decide whether a slab's delivery hides under the
 * walk.  Blocks until done.  The first n_cells floats of every peer buffer ARE OVERWRITTEN with src's (the probe is
 * the push itself); the caller's current device is left as it was. */
int m2s_peer_bandwidth(const float* src, float* const* peers, uint32_t n_peers, size_t n_cells, int device, float* gbps_each, float* gbps_all);

/* One process per GPU (torch.distributed / MPI launchers): the same no-collective exchange across processes.
 * Every rank allocates its whole-grid buffer with m2s_shared_alloc (a dedicated hipMalloc block, so that its IPC handle
 * maps exactly this buffer), exports it, exchanges the 64-byte handles by any host-side means, opens the other ranks'
 * handles and passes the mapped pointers as m2s_opts.peer_out.  A host-side barrier after the local stream has drained
 * tells a rank that its own buffer is complete (the peers' pushes are ordinary device writes, finished when their
 * streams are). */
#define M2S_IPC_HANDLE_BYTES 64
int m2s_shared_alloc(size_t bytes, int device, void** device_ptr);
int m2s_shared_free(void* device_ptr, int device);
int m2s_ipc_export(const void* device_ptr, uint8_t handle[M2S_IPC_HANDLE_BYTES]);
int m2s_ipc_open(const uint8_t handle[M2S_IPC_HANDLE_BYTES], int device, void** device_ptr);
int m2s_ipc_close(void* device_ptr, int device);

/* ---- persistent mesh (optional) ------------------------------------------------------------------
 * The reference rebuilds its acceleration structures inside every call (generate/grid.rs:95-111,
 * generic/rtree_bvh.rs:109-119).  A caller that queries the same mesh repeatedly — the reference's
 * own client regenerates the grid on every parameter change, mesh_to_sdf_client/src/sdf.rs:32-137 —
 * or that splits one grid into several x-slab calls can build once and reuse:
 * triangle records + LBVH stay resident on `opts->device`; the sign planes of the last grid are cached.
 * Results are identical to the one-shot entry points.
 * A call may re-mark the resident tree's leaves for its own grid / query set (how many triangles a leaf holds follows the triangles
 * per brick, or the queries per triangle: a 5 us launch on the call's stream).  When that happens while earlier asynchronous
 * calls, or calls on another stream, may still be walking the tree, the call synchronises the device first; callers that keep
 * several streams busy on one mesh avoid it by giving them grids of the same density class (the x-slabs of one grid always are). */
typedef struct m2s_mesh m2s_mesh;
int m2s_mesh_create(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes,
                    int topology, const m2s_opts* opts, m2s_mesh** out_mesh);
void m2s_mesh_destroy(m2s_mesh* mesh);
size_t m2s_mesh_triangle_count(const m2s_mesh* mesh);
int m2s_mesh_generate_grid_sdf(m2s_mesh* mesh, const m2s_grid* grid, int sign_method, float* out, const m2s_opts* opts);
int m2s_mesh_generate_sdf(m2s_mesh* mesh, const float* queries, size_t n_queries, int accel, int sign_method, float* out,
                          size_t* n_out, const m2s_opts* opts);
/* Device-memory calls made with opts->synchronous == 0 return before the GPU has finished and report no
 * per-call timings; this sums the dominant-kernel durations of all such calls since the last drain
 * (distance_ms, distance_launches, n_units; accel_build_ms = the mesh build).  Blocks until they finished.
 * Asynchronous calls also DEFER their device-side error report to this call: M2S_ERR_NAN if any of them met a
 * NaN distance in SignMethod::Normal (the reference panics, lib.rs:257). */
int m2s_mesh_drain_timings(m2s_mesh* mesh, m2s_timings* timings);

/* ---- closest points: which triangle is nearest, and where on it -------------------------------------
 * What libigl signed_distance (I, C), trimesh closest_point or Open3D compute_closest_points return beside the distance, for the
 * SDF gradient sign * (p - c) / |d|, attribute transfer from the nearest face and snapping points onto the surface.  Per point p:
 *   triangle_out[i]        the t minimising point_triangle_distance2(p, T_t) (geo.rs:33-37,70-138, f32, no FMA), t in the caller's
 *                          triangle order (Topology::get_triangles, lib.rs:175-193); on exact ties of d2 the lowest t; a NaN d2 is never
 *                          nearest; UINT32_MAX when no triangle has a comparable distance.
 *   point_out[3i .. 3i+2]  closest_point_triangle(p, a, b, c) of that triangle (geo.rs:70-138), bit for bit; NaN x 3 under UINT32_MAX.
 *   distance_out[i]        its unsigned distance sqrt(d2): bit-equal to |m2s_generate_sdf(.., M2S_ACCEL_RTREE_BVH, ..)| and to
 *                          |m2s_generate_grid_sdf(.., M2S_SIGN_RAYCAST, ..)| at the same point (f32::MAX where those give it).
 * Any of the three outputs may be NULL, not all of them (M2S_ERR_BAD_ARG).  A mesh without triangles: M2S_ERR_EMPTY_MESH.
 * Two passes on the call's stream: the unsigned distance walk of the generate call, then a walk that finds the triangle attaining each
 * distance.  m2s_opts as for the generate calls — device, stream / stream_mode, mem_kind (ALL data pointers on one side),
 * synchronous, lane; timings: accel_build_ms = the build, distance_ms = both passes, seed_ms = the first pass alone (the distances that
 * seed the second), total_ms = the whole device time; algorithm = 1: every triangle for every point (validation).  Host-memory indices are range-checked before any device work (M2S_ERR_BAD_ARG).
 *
 * m2s_closest_points — queries: n_queries packed xyz (NULL only with n_queries == 0); outputs n_queries entries (x 3 for point_out). */
int m2s_closest_points(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes,
                       int topology, const float* queries, size_t n_queries,
                       uint32_t* triangle_out, float* point_out, float* distance_out, const m2s_opts* opts);
/* m2s_grid_closest_points — the grid's cell centres (grid.rs:135-141, as the grid path computes them) in its output layout
 * z + y*nz + x*ny*nz; the outputs address the whole grid (3 floats per cell for point_out).  opts->x_begin / x_end select an x-slab as for
 * m2s_generate_grid_sdf: only the slab is written.  A grid without cells, x_period or peer_out: M2S_ERR_BAD_ARG. */
int m2s_grid_closest_points(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes,
                            int topology, const m2s_grid* grid,
                            uint32_t* triangle_out, float* point_out, float* distance_out, const m2s_opts* opts);
/* The same on a persistent mesh (below): its resident tree, no build; results identical to the one-shot calls.  The tree is walked as it
 * is (no re-marking of its leaves), so later generate calls on the mesh are unaffected. */
int m2s_mesh_closest_points(m2s_mesh* mesh, const float* queries, size_t n_queries,
                            uint32_t* triangle_out, float* point_out, float* distance_out, const m2s_opts* opts);
int m2s_mesh_grid_closest_points(m2s_mesh* mesh, const m2s_grid* grid,
                                 uint32_t* triangle_out, float* point_out, float* distance_out, const m2s_opts* opts);

/* ---- generalized winding numbers: a robust inside / outside for meshes that are not watertight -------------------------------
 * Raycast needs a watertight mesh and Normal leaks; on scans and game assets with holes, open borders, doubled sheets or
 * self-intersections the remedy of libigl (SIGNED_DISTANCE_TYPE_WINDING_NUMBER), Houdini and Open3D is
 *   w(p) = (1 / 4 pi) sum_t Omega_t(p),   Omega_t = the signed solid angle of triangle t seen from p
 * (Jacobson et al. 2013).  Orientation: the right-hand normal (b - a) x (c - a) points outward, as for the isosurface below; then w is 1
 * inside and 0 outside a closed mesh, degrades smoothly across holes, and w >= 1/2 is the inside test (threshold; callers default to 0.5).
 *   winding_out[i]  w(p_i), f32.
 *   sdf_out[i]      w >= threshold ? -d : d, with d the unsigned distance of the closest-point calls: |sdf_out[i]| is bit-equal to their
 *                   distance_out[i].  A NaN w gives +d.
 * Either output may be NULL, not both (M2S_ERR_BAD_ARG).
 * Arithmetic.  Exact term (Van Oosterom-Strackee), f32, a, b, c relative to p and n = the raw normal of the triangle:
 *   Omega = 2 atan2(a . n, |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|)          (a . n = a . (b x c), formed from the edge vectors);
 * a triangle whose raw normal is zero, or whose numerator is exactly 0 (p in its plane), contributes 0; a NaN point gives NaN.
 * Every point must account for every triangle, so the walk is a Barnes-Hut one (Barill et al. 2018, order 1): every node of the tree
 * has a centre c~ (area-weighted mean of its triangles' centroids), a radius r (>= the distance from c~ to any of its vertices), and the
 * moments S = sum a_t and M = sum a_t (x) (c_t - c~) of its area vectors a_t = (b - a) x (c - a) / 2.  A point with |c~ - p| > beta r
 * takes S . K(x) + <M, grad K(x)>, x = c~ - p, K(x) = x / (4 pi |x|^3), grad K = (I / |x|^3 - 3 x x^T / |x|^5) / 4 pi, instead of the
 * node's triangles; subtrees of at most 8 triangles are summed exactly.  beta is finite and >= 1, or +inf (no node is ever accepted:
 * the exact sum through the tree); NaN or < 1: M2S_ERR_BAD_ARG.  M2S_WINDING_BETA_DEFAULT = 3: tests/winding_model.py measures a largest
 * error of 4.1e-2 / 1.7e-2 / 8.4e-3 at beta = 2 / 3 / 4 (tests/golden/winding_model_error.json); 1.7e-2 is well inside the band
 * |w - 1/2| < 0.1 in which a hole, not the expansion, decides the sign (4.1e-2 is nearly half of it), and the walk's cost grows with beta.
 * algorithm = 1: every triangle for every point, exactly, in the tree's triangle order (validation).
 * Reproducibility.  A point's value depends only on (tree, point, beta): on one m2s_mesh the grid forms, their x-slabs and the point
 * forms agree bit for bit at the same f32 point, whatever other calls re-marked the tree in between.  One-shot calls may build
 * different trees from call to call (M2S_TREELETS) and agree only within the accuracy above.
 * A mesh without triangles: w = 0 everywhere, M2S_ERR_EMPTY_MESH only if sdf_out is asked for.
 * m2s_opts as for the closest-point calls — device, stream / stream_mode, mem_kind, synchronous, lane, x_begin / x_end for the grid forms
 * (only the slab is written); x_period or peer_out: M2S_ERR_BAD_ARG.  timings: accel_build_ms = the build, seed_ms = the moments (a
 * persistent mesh makes them in its first winding call and keeps them until m2s_mesh_destroy), distance_ms = the distance pass (only
 * with sdf_out) + the winding walk, total_ms = the whole device time.  Host-memory arguments are checked before any device work.
 * Asynchronous calls on a mesh finish, and add their spans up, in m2s_mesh_drain_timings. */
#define M2S_WINDING_BETA_DEFAULT 3.0f
int m2s_winding_numbers(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes,
                        int topology, const float* queries, size_t n_queries, float beta, float threshold,
                        float* winding_out, float* sdf_out, const m2s_opts* opts);
/* The grid's cell centres in its output layout z + y*nz + x*ny*nz, as m2s_grid_closest_points addresses them. */
int m2s_grid_winding_numbers(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes,
                             int topology, const m2s_grid* grid, float beta, float threshold,
                             float* winding_out, float* sdf_out, const m2s_opts* opts);
int m2s_mesh_winding_numbers(m2s_mesh* mesh, const float* queries, size_t n_queries, float beta, float threshold,
                             float* winding_out, float* sdf_out, const m2s_opts* opts);
int m2s_mesh_grid_winding_numbers(m2s_mesh* mesh, const m2s_grid* grid, float beta, float threshold,
                                  float* winding_out, float* sdf_out, const m2s_opts* opts);

/* ---- ray casting against the mesh: first hit, hit count, occlusion -----------------------------------------------------------------
 * What Open3D RaycastingScene cast_rays / count_intersections / test_occlusions, trimesh ray.intersects_* and libigl ray_mesh_intersect
 * answer, with the watertight test of Woop, Benthin and Wald (2013) instead of Moeller-Trumbore, which leaks through the shared edges
 * and vertices of a closed mesh in f32.  Per ray (o, d) and the call's range [t_min, t_max]:
 *   t_out[i]             the smallest t over all triangles the ray hits in range; +inf when none.
 *   triangle_out[i]      the triangle attaining it, in the caller's triangle order (Topology::get_triangles); the lowest index on exact
 *                        ties of t; UINT32_MAX when none.
 *   uv_out[2i], [2i+1]   barycentric weights of b and c at that hit: hit = a + u (b - a) + v (c - a); NaN x 2 when none.
 *   count_out[i]         the number of triangles hit in range.  A ray through a shared edge or vertex counts EVERY triangle that includes
 *                        it (zeros of the edge functions are inside), so on a closed mesh the count's parity is an inside test only for
 *                        rays that avoid edges and vertices.
 *   occluded_out[i]      uint8, 1 iff at least one hit in range.  When this is the only output asked for the walk stops at a ray's first hit.
 * Any output may be NULL, not all of them (M2S_ERR_BAD_ARG; with n_rays == 0 nothing is written and none is needed).  d is used as given, not normalised: t is in units of |d|.
 * Arithmetic: IEEE binary32, no FMA, sums left to right, correctly rounded divisions (mesh_to_sdf_amd/csrc/ray.hip.h; tests/ray_model.py
 * restates it in numpy).
 *   Ray:       kz = the index of the largest |d_k| (the lowest index on ties), kx = (kz + 1) % 3, ky = (kx + 1) % 3, kx and ky swapped if
 *              d[kz] < 0;  Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].
 *   Triangle:  (a, b, c) the caller's vertices.  A = a - o;  Ax = A[kx] - Sx * A[kz], Ay = A[ky] - Sy * A[kz], Az = Sz * A[kz]; the same for
 *              B and C.  U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax.
 *              Miss if (U < 0 || V < 0 || W < 0) && (U > 0 || V > 0 || W > 0): zeros are inside, nothing is culled, there is no f64 fallback.
 *              det = U + V + W; miss if det == 0 or NaN.
 *              Miss unless the ray's axis (0, 0) lies in the rectangle of (Ax, Ay), (Bx, By), (Cx, Cy) widened by mxy: miss if
 *              min(Ax, Bx, Cx) > mxy, max(Ax, Bx, Cx) < -mxy, or the same in y;  mxy = 2^-20 * the largest of |Ax| ... |Cy|.
 *              t = (U * Az + V * Bz + W * Cz) / det.  Miss if t < min(Az, Bz, Cz) - mz or t > max(Az, Bz, Cz) + mz;
 *              mz = 2^-21 * the largest of |Az|, |Bz|, |Cz|.  Hit iff t_min <= t <= t_max.
 *              u = V / det, v = W / det.  Swapping b and c keeps the hit; u and v change places and, like t, agree only up to
 *              rounding (det and the numerator are summed in another order).
 *   A ray with a non-finite component in o or d, or d = (0, 0, 0): no hit, count 0.  A mesh without triangles: no hit anywhere, M2S_OK.
 * The two "miss unless" clauses are this library's addition to the paper's test.  They change no bit for a triangle whose image in
 * the ray's frame is not degenerate.  For one seen EDGE-ON — the ray lies in its plane, or it is a sliver below the
 * resolution of its coordinates — U, V and W are rounding noise, and with zeros inside and no f64 fallback the bare test reports hits
 * although the axis passes far outside the three points; the clauses make those misses, by a rule a tree can prune for exactly.  They do
 * not open a closed mesh: a ray through a shared edge or vertex has its axis on the rectangle of every triangle that includes it.
 * algorithm = 1 (every triangle for every ray, no tree) is the definition.  The default walks the tree and skips a node only when the
 * same clauses, applied to the node's box with the triangle test's own operations, exclude every triangle below it: it returns the same
 * bits for every output on every ray, however the tree's leaves are marked.
 * The range: m2s_ray_opts, NULL = [0, +inf]; t_min <= t_max with neither NaN, otherwise M2S_ERR_BAD_ARG.
 * m2s_opts as for the closest-point calls: device, stream / stream_mode, mem_kind (EVERY data pointer on one side), synchronous, lane,
 * algorithm.  M2S_ERR_BAD_ARG before any device work: x_begin, x_end, x_period or peer_out not zero; NULL inputs with n > 0; every output
 * NULL; bad enums; host-memory indices out of range.  n_rays == 0: M2S_OK.  timings: accel_build_ms = the build, distance_ms = the ray
 * kernel, n_units = rays. */
typedef struct m2s_ray_opts {
  uint32_t struct_size;  /* sizeof(m2s_ray_opts) */
  float t_min;           /* NULL opts: 0 */
  float t_max;           /* NULL opts: +inf */
} m2s_ray_opts;
/* origins, directions: n_rays packed xyz. */
int m2s_cast_rays(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes, int topology,
                  const float* origins, const float* directions, size_t n_rays, const m2s_ray_opts* ropts,
                  float* t_out, uint32_t* triangle_out, float* uv_out, uint32_t* count_out, uint8_t* occluded_out, const m2s_opts* opts);
/* The same on a persistent mesh: its resident tree as it is — no build, no re-marking of its leaves — and the same bits as the one-shot
 * call.  Asynchronous calls finish, and add their spans up, in m2s_mesh_drain_timings. */
int m2s_mesh_cast_rays(m2s_mesh* mesh, const float* origins, const float* directions, size_t n_rays, const m2s_ray_opts* ropts,
                       float* t_out, uint32_t* triangle_out, float* uv_out, uint32_t* count_out, uint8_t* occluded_out, const m2s_opts* opts);

/* ---- area-weighted surface sampling: the points the other calls are asked at ----------------------------------------------------------
 * What trimesh sample_surface, Open3D sample_points_uniformly, libigl random_points_on_mesh and mesh_to_sdf's sample_sdf_near_surface start
 * from: points uniformly distributed over the surface, with the triangle, the barycentric weights and the normal of each.  The result is
 * defined to the bit (mesh_to_sdf_amd/csrc/sample.hip.h; tests/sample_model.py restates it in numpy): sample i of a call is GLOBAL sample
 * g = first_sample + i, and its value depends only on (the triangles in the caller's order, seed, g).  IEEE binary32, no FMA, sums left to
 * right, correctly rounded sqrt and division, except where f64 or integers are named.
 *   Weights.    Triangles in the caller's order (Topology::get_triangles).  For t = (a, b, c): e1 = b - a, e2 = c - a, n = e1 x e2
 *               (n.x = e1.y*e2.z - e1.z*e2.y, ...), A_t = sqrt((n.x*n.x + n.y*n.y) + n.z*n.z) = twice the area; a non-finite A_t counts as 0.
 *               Amax = max A_t.  Amax == 0 or no triangles: *area_out = 0 and the call returns M2S_ERR_EMPTY_MESH when n_samples > 0, else
 *               M2S_OK.  e = floor(log2(Amax)) (the f32's exponent, subnormals included);  w_t = (uint64) floor((double)A_t * 2^(37 - e))
 *               (exact: a power-of-two scale; w_t < 2^38);  C_t = w_0 + ... + w_t in uint64 (< 2^63 for 2^25 triangles), W = C_last.  Integer
 *               sums are associative: every scan order gives the same table.  *area_out = ldexp((double)W, e - 38): the total area of the
 *               triangles the sampler can reach.
 *   Generator.  Philox4x32-10 (Salmon et al. 2011): counter (g & 0xffffffff, g >> 32, 0, 0), key (seed & 0xffffffff, seed >> 32),
 *               multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85; the output is (r0, r1, r2, r3).
 *   Triangle.   x = r0 | (uint64)r1 << 32;  T = floor(x * W / 2^64), the high half of the 128-bit product;  t = the smallest index with
 *               C_t > T.  A triangle of weight 0 is never chosen.
 *   Point.      u' = (r2 >> 9) * 2^-23 + 2^-24, v' likewise from r3: exact, strictly inside (0, 1), and so are 1 - u', 1 - v'.  If u' + v' > 1
 *               (f32 sum): u = 1 - u', v = 1 - v'; else u = u', v = v'.  p_k = (a_k + u * (b_k - a_k)) + v * (c_k - a_k).
 *   point_out[3i ..]        p.
 *   triangle_out[i]         t, in the caller's triangle order.
 *   uv_out[2i], [2i + 1]    u, v: the weights of b and c, as m2s_cast_rays reports them.
 *   normal_out[3i ..]       n_k / A_t of the chosen triangle: the unit right-hand normal, which winding numbers and isosurfaces call outward.
 *   area_out                one double on the HOST, whatever mem_kind says; written by every call that passes the argument checks.
 * Any output may be NULL; all five NULL is M2S_ERR_BAD_ARG.  n_samples == 0 with area_out alone is the "surface area" query.
 * m2s_surface_sample_opts: NULL = seed 0, first_sample 0.  reserved != 0, a struct_size other than sizeof(m2s_surface_sample_opts), or
 * first_sample + n_samples overflowing uint64: M2S_ERR_BAD_ARG.  Ranks of a multi-GPU job take disjoint ranges of g of one seed.
 * Consequences: the one-shot and the m2s_mesh form agree bit for bit; two calls over [0, k) and [k, n) equal one call over [0, n);
 * re-marking a resident tree's leaves changes nothing (the tree is not consulted at all).
 * m2s_opts as for the ray calls: device, stream / stream_mode, mem_kind (EVERY data pointer on one side, area_out excepted), synchronous,
 * lane.  M2S_ERR_BAD_ARG before any device work: x_begin, x_end, x_period or peer_out not zero; bad enums; host-memory indices out of
 * range.  algorithm = 1 picks the triangle by a linear scan of C (validation): the same bits.  The table's total travels to the host
 * once — the call's stream is synchronised after the table is made, also when synchronous == 0 — so a one-shot call does that every
 * time, a persistent mesh only in its first sampling call: it keeps C in a block of its own until m2s_mesh_destroy.
 * timings: accel_build_ms = 0 for the one-shot form (it builds no tree), seed_ms = the weight table (0 on a mesh that has it),
 * distance_ms = the sampling kernel, n_units = samples.  Asynchronous calls on a mesh finish, and add their spans up, in
 * m2s_mesh_drain_timings. */
typedef struct m2s_surface_sample_opts {
  uint32_t struct_size;   /* sizeof(m2s_surface_sample_opts) */
  uint32_t reserved;      /* 0 */
  uint64_t seed;          /* NULL opts: 0 */
  uint64_t first_sample;  /* NULL opts: 0; sample i of the call is global sample g = first_sample + i */
} m2s_surface_sample_opts;
int m2s_sample_surface(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes, int topology,
                       size_t n_samples, const m2s_surface_sample_opts* sopts,
                       float* point_out, uint32_t* triangle_out, float* uv_out, float* normal_out, double* area_out, const m2s_opts* opts);
int m2s_mesh_sample_surface(m2s_mesh* mesh, size_t n_samples, const m2s_surface_sample_opts* sopts,
                            float* point_out, uint32_t* triangle_out, float* uv_out, float* normal_out, double* area_out, const m2s_opts* opts);

/* ---- voxelization: which cells the mesh occupies -----------------------------------------------------------------------------------------
 * What trimesh voxelized, Open3D VoxelGrid.create_from_triangle_mesh, kaolin trianglemeshes_to_voxelgrids and binvox compute: one bit per
 * cell of the grid, set where a triangle touches the cell's box (SURFACE) or, in addition, where the cell's centre is inside (SOLID).  The
 * result is defined to the bit (mesh_to_sdf_amd/csrc/voxel.hip.h; tests/voxel_model.py restates it in numpy).  IEEE binary32, no FMA, sums
 * left to right.
 *   Cell (i, j, k).  Centre q_m = first_cell_m + (float)idx_m * cell_size_m (m2s_grid_cell_center); half extent h_m = cell_size_m * 0.5f.  The
 *               box is closed: touching counts.
 *   Triangle t = (a, b, c) in the caller's order (Topology::get_triangles).  A triangle with any non-finite coordinate overlaps nothing.
 *               e0 = b - a, e1 = c - b, e2 = a - c;  n = e0 x e1 (n.x = e0.y*e1.z - e0.z*e1.y, ...).  Per cell: v0 = a - q, v1 = b - q, v2 = c - q.
 *   overlap(t, cell) holds iff none of 13 clauses misses.  `min(x, y, z) > r` below means "x > r and y > r and z > r" and `max(x, y, z) < -r`
 *               means "x < -r and y < -r and z < -r": a NaN in any term never misses.
 *     box axes,   m = x, y, z:  miss if min(v0_m, v1_m, v2_m) > h_m or max(v0_m, v1_m, v2_m) < -h_m.
 *     plane:      d = (n.x*v0.x + n.y*v0.y) + n.z*v0.z;  r = (h.x*|n.x| + h.y*|n.y|) + h.z*|n.z|;  miss if d > r or d < -r.
 *     cross axes, each edge e = e_j (j = 0, 1, 2) and each m with (m1, m2) = ((m+1)%3, (m+2)%3):  p_i = e_m1 * vi_m2 - e_m2 * vi_m1 for i = 0, 1,
 *                 2 (all three computed, none reused);  r = h_m1*|e_m2| + h_m2*|e_m1|;  miss if min(p_0, p_1, p_2) > r or max(p_0, p_1, p_2) < -r.
 *               This is the separating-axis test of Akenine-Moller (2001) with its operations fixed.  A zero-area triangle (a segment, a
 *               point) takes the same clauses with n = 0; there is no special case.
 *   M2S_VOXELIZE_SURFACE  the cell is set iff overlap(t, cell) holds for some t.
 *   M2S_VOXELIZE_SOLID    the surface set, OR the inside bit that m2s_generate_grid_sdf(..., M2S_SIGN_RAYCAST) applies to that cell (the
 *               majority plane of sign.hip): on any mesh, solid == surface | signbit(generate_grid_sdf(Raycast)), cell for cell.  A cell
 *               whose centre lies on a triangle is a surface cell, so the sign of a zero distance never matters.
 * m2s_opts.algorithm = 1 evaluates every triangle against every cell and is the definition; the default path returns the same bits in every
 * output on every input, one-shot or m2s_mesh, host or device memory.  The result is an OR: it does not depend on the order of evaluation.
 *   bits_out       uint32[nx*ny*nzw], nzw = ceil(nz/32): cell (i, j, k) is bit k & 31 of word (i*ny + j)*nzw + (k >> 5) (the layout of the sign
 *                  planes); bits at k >= nz are 0.
 *   occupancy_out  uint8[nx*ny*nz], 0 or 1, at L = k + j*nz + i*ny*nz (Grid::get_cell_idx).
 *   cells_out      the L of every set cell as uint64, ascending; cell_capacity = the entries it can hold.
 *   n_set_out      the number of set cells: one uint64 on the HOST, whatever mem_kind says (like area_out); written by every call that passes
 *                  the argument checks.
 * Each may be NULL; all four NULL is M2S_ERR_BAD_ARG.  A cell_capacity below the count is M2S_ERR_BAD_ARG with *n_set_out written, bits_out
 * and occupancy_out complete and cells_out untouched.  A call that asks for cells_out or n_set_out synchronises its stream once for the
 * count; one that asks only for bits_out / occupancy_out honours synchronous = 0.
 * m2s_voxelize_opts: NULL = SURFACE.  M2S_ERR_BAD_ARG before any device work: NULL grid; a zero cell count, a face of 2^32 or more lines or
 * 2^36 or more cells; a cell size <= 0 or not finite; a non-finite first_cell; a bad mode or a struct_size other than
 * sizeof(m2s_voxelize_opts); x_begin, x_end, x_period or peer_out not zero (slabs are out of scope here: the whole grid is voxelized); bad
 * enums; host-memory indices out of range.  A mesh without triangles sets nothing and returns M2S_OK, in both modes.
 * m2s_opts otherwise as for the ray calls: device, stream / stream_mode, mem_kind (EVERY data pointer on one side, n_set_out excepted),
 * synchronous, lane, algorithm.  timings: accel_build_ms = the triangle records (the one-shot form builds no tree), seed_ms = the sign
 * planes (0 for SURFACE), distance_ms = the voxelization kernels, n_units = the grid's cells.  The tree of an m2s_mesh is not consulted, so
 * re-marking its leaves changes nothing; asynchronous calls on a mesh add their spans up in m2s_mesh_drain_timings.
 * Cost: proportional to the sum over triangles of (candidate columns x z extent) of their boxes — a mesh of many grid-spanning skewed
 * triangles in a 1024^3 grid is legal and slow. */
enum { M2S_VOXELIZE_SURFACE = 0, M2S_VOXELIZE_SOLID = 1 };
typedef struct m2s_voxelize_opts {
  uint32_t struct_size;   /* sizeof(m2s_voxelize_opts) */
  uint32_t mode;          /* M2S_VOXELIZE_SURFACE / M2S_VOXELIZE_SOLID */
} m2s_voxelize_opts;
int m2s_voxelize(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes, int topology,
                 const m2s_grid* grid, const m2s_voxelize_opts* vopts, uint32_t* bits_out, uint8_t* occupancy_out,
                 uint64_t* cells_out, uint64_t cell_capacity, uint64_t* n_set_out, const m2s_opts* opts);
int m2s_mesh_voxelize(m2s_mesh* mesh, const m2s_grid* grid, const m2s_voxelize_opts* vopts, uint32_t* bits_out, uint8_t* occupancy_out,
                      uint64_t* cells_out, uint64_t cell_capacity, uint64_t* n_set_out, const m2s_opts* opts);

/* ---- narrow-band grid SDFs: the cells near the surface, and their distances --------------------------------------------------------------
 * What OpenVDB meshToLevelSet(exteriorBand, interiorBand), kaolin's sparse grids and sparse-brick SDF stores ask for: the signed distance
 * at the cells within a few cell widths of the surface and nothing else — O(n^2) cells of an n^3 grid.  The result is DEFINED as a filter
 * of the dense call, so it has no floating-point model of its own:
 *   D = m2s_generate_grid_sdf(mesh, grid, sign_method), negative inside; exterior >= 0 and interior >= 0 in world units;
 *   the active set is  A = { L : -interior <= D[L] <= exterior },  L = k + j*nz + i*ny*nz.
 * Both widths may be +inf.  A NaN in D[L] is never active (both comparisons fail); -0 and +0 count as 0.  With exterior = +inf the cells
 * where the dense call keeps f32::MAX (a mesh without triangles, or without a finite one) are active like any other; with a finite
 * exterior such a mesh activates nothing.
 *   cells_out      the L of every active cell as uint64, ascending.
 *   distances_out  distances_out[n] = D[cells_out[n]], every bit including the sign bit.
 *   bits_out       the active set as a mask in the layout of m2s_voxelize's bits_out (the sign planes'); bits at k >= nz are 0.
 *   n_active_out   the number of active cells: one uint64 on the HOST, whatever mem_kind says; written by every call that passes the
 *                  argument checks.
 * Each may be NULL; all four NULL is M2S_ERR_BAD_ARG.  `capacity` = the entries cells_out and distances_out can each hold.  A capacity
 * below the count is M2S_ERR_BAD_ARG with *n_active_out written, bits_out complete and cells_out / distances_out untouched (the call
 * compacts into its workspace and copies once the count is known to fit: counting first would walk every candidate twice).
 * sign_method: M2S_SIGN_NORMAL or M2S_SIGN_RAYCAST, the rules of m2s_generate_grid_sdf.  m2s_opts.algorithm = 1 is the definition made
 * literal — the dense grid call into the workspace, then the filter — and needs room for the dense grid; the default path returns the
 * same bits in every output on every input, one-shot or m2s_mesh, host or device memory.  It evaluates only candidates: cells whose
 * centre is within max(exterior, interior), grown by the walks' own pruning margin, of some triangle's axis-aligned box (band.hip.h gives
 * the predicate and the argument that no active cell is missed), in chunks of M2S_BAND_CHUNK candidates through the query walk.
 * M2S_ERR_BAD_ARG before any device work: everything m2s_voxelize rejects for a grid (2^36 or more cells, a face of 2^32 or more lines, ...);
 * x_begin, x_end, x_period or peer_out not zero; NULL bopts, a width that is negative or NaN, a struct_size other than
 * sizeof(m2s_band_opts); all outputs NULL; a bad sign method; bad enums; host-memory indices out of range.  M2S_ERR_NAN as
 * m2s_generate_grid_sdf reports it (Normal) when the walk of a candidate meets a NaN distance.
 * m2s_opts otherwise as for m2s_voxelize.  The call synchronises its stream twice — for the number of candidates, which sizes the chunks,
 * and for the number of active cells — so synchronous = 0 on an m2s_mesh only moves the timings into m2s_mesh_drain_timings.
 * timings: accel_build_ms = the build (the one-shot form builds a tree with the leaf size the query walk asks for), seed_ms = the sign
 * planes plus the candidate pass, distance_ms = the query walks plus filter and compaction, n_units = the candidates evaluated (the
 * grid's cells under algorithm 1).
 * Workspace: two masks, the sign planes (Raycast), one chunk's queries and query workspace, and min(capacity, cells) entries of 12 bytes
 * when cells_out or distances_out is asked for. */
typedef struct m2s_band_opts {
  uint32_t struct_size;   /* sizeof(m2s_band_opts) */
  float exterior;         /* >= 0, +inf allowed: the band's width outside (D > 0), world units */
  float interior;         /* >= 0, +inf allowed: its width inside (D < 0) */
} m2s_band_opts;
int m2s_narrow_band_sdf(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes, int topology,
                        const m2s_grid* grid, int sign_method, const m2s_band_opts* bopts,
                        uint64_t* cells_out, float* distances_out, uint64_t capacity, uint32_t* bits_out,
                        uint64_t* n_active_out, const m2s_opts* opts);
int m2s_mesh_narrow_band_sdf(m2s_mesh* mesh, const m2s_grid* grid, int sign_method, const m2s_band_opts* bopts,
                             uint64_t* cells_out, float* distances_out, uint64_t capacity, uint32_t* bits_out,
                             uint64_t* n_active_out, const m2s_opts* opts);

/* Grid helpers with the reference's exact f32 arithmetic (so callers need not re-derive it).
 * m2s_grid_from_bounding_box — Grid::from_bounding_box, grid.rs:59-74.
 * m2s_grid_cell_center      — Grid::get_cell_center,   grid.rs:135-141.
 * m2s_grid_cell_idx         — Grid::get_cell_idx,      grid.rs:122-124. */
void m2s_grid_from_bounding_box(const float bbox_min[3], const float bbox_max[3], const uint64_t cell_count[3],
                                m2s_grid* grid);
void m2s_grid_cell_center(const m2s_grid* grid, const uint64_t cell[3], float out[3]);
uint64_t m2s_grid_cell_idx(const m2s_grid* grid, const uint64_t cell[3]);

/* Number of triangles Topology::get_triangles (lib.rs:175-193) yields for these arguments. */
size_t m2s_triangle_count(size_t n_vertices, size_t n_indices, int has_indices, int topology);

/* ---- the data formats and callers either side of the path -------------------
 *
 * V1 container — mesh_to_sdf/src/serde.rs:75-221.  `save_to_file` writes rmp-serde's compact MessagePack
 * encoding of SerializeVersion::V1(SerializeSdf::{Generic,Grid}) (serde.rs:161-166): enums are one-entry
 * maps keyed by the variant name, structs are arrays, f32 is `ca` + 4 big-endian bytes, usize is the
 * shortest unsigned form, a point is `93 ca.. ca.. ca..`:
 *   Grid    81 a2 "V1" 81 a4 "Grid"    92 [93 first_cell(3 f32) cell_size(3 f32) 93 cell_count(3 uint)] [array n: f32...]
 *   Generic 81 a2 "V1" 81 a7 "Generic" 92 [array nq: point...] [array nd: f32...]
 * Pinned byte for byte on the reference's golden files tests/sdf_grid_v1.bin and tests/sdf_generic_v1.bin
 * (serde.rs:314-374).  The payload arrays (5 B per distance, 16 B per point) are produced / consumed by
 * HIP kernels so a device-resident result is encoded without a round trip through host f32 arrays.
 * `distances` / `queries` / `bytes` follow opts->mem_kind like every other data pointer. */
enum m2s_sdf_kind { M2S_SDF_GENERIC = 0, M2S_SDF_GRID = 1 };

typedef struct m2s_sdf_info {
  int32_t kind;              /* enum m2s_sdf_kind */
  int32_t canonical;         /* 1: both arrays use exactly the fixed-width encoding above (decoded by the HIP kernels);
                                0: some element uses another valid MessagePack number form (f64, ints) that serde would
                                   accept for an f32 — decoded by the scalar host reader */
  m2s_grid grid;             /* kind == M2S_SDF_GRID */
  uint64_t n_queries;        /* kind == M2S_SDF_GENERIC, else 0 */
  uint64_t n_distances;
  uint64_t queries_offset;   /* byte offset of the first element of each array (canonical == 1) */
  uint64_t distances_offset;
} m2s_sdf_info;

/* Exact size in bytes of the container; 0 if a count does not fit MessagePack's 32-bit array header. */
size_t m2s_sdf_grid_encoded_size(const m2s_grid* grid, size_t n_distances);
size_t m2s_sdf_generic_encoded_size(size_t n_queries, size_t n_distances);

/* serialize(&SerializeSdf::Grid(..)) — serde.rs:99-107,161-166.  n_distances is NOT required to equal the
 * grid's cell count (the reference does not check either).  *written (optional) receives the size. */
int m2s_sdf_encode_grid(const m2s_grid* grid, const float* distances, size_t n_distances, uint8_t* bytes,
                        size_t capacity, size_t* written, const m2s_opts* opts);
/* serialize(&SerializeSdf::Generic(..)) — serde.rs:87-95,161-166.  queries: n_queries packed xyz. */
int m2s_sdf_encode_generic(const float* queries, size_t n_queries, const float* distances, size_t n_distances,
                           uint8_t* bytes, size_t capacity, size_t* written, const m2s_opts* opts);

/* First half of deserialize() — serde.rs:169-176: reads the envelope and the array headers so the caller
 * can size its buffers.  M2S_ERR_BAD_ARG = SerdeError::DeserializationFailed. */
int m2s_sdf_probe(const uint8_t* bytes, size_t n_bytes, m2s_sdf_info* info, const m2s_opts* opts);
/* Second half: fills queries_out (n_queries*3 f32; may be NULL for a grid container) and distances_out
 * (n_distances f32).  Always synchronous (a malformed element is reported by the return code). */
int m2s_sdf_decode(const uint8_t* bytes, size_t n_bytes, float* queries_out, float* distances_out,
                   const m2s_opts* opts);

/* save_to_file / read_from_file — serde.rs:192-198, 216-220.  M2S_ERR_IO = SerdeError::IoError. */
#define M2S_ERR_IO (-5)
int m2s_sdf_save_grid(const char* path, const m2s_grid* grid, const float* distances, size_t n_distances,
                      const m2s_opts* opts);
int m2s_sdf_save_generic(const char* path, const float* queries, size_t n_queries, const float* distances,
                         size_t n_distances, const m2s_opts* opts);
int m2s_sdf_probe_file(const char* path, m2s_sdf_info* info);
int m2s_sdf_read_file(const char* path, float* queries_out, float* distances_out, const m2s_opts* opts);

/* Client post-step on a generated grid — mesh_to_sdf_client/src/sdf.rs:62-72 and :120:
 *   ordered_indices = (0..n).sorted_by(|i, j| data[i].total_cmp(&data[j])).map(|i| i as u32)   (stable sort)
 *   iso_limits      = data.iter().copied().minmax()                                            (itertools)
 * ordered_indices: n u32, same side as `distances` (opts->mem_kind).  iso_limits: 2 floats on the HOST, optional;
 * first of equal minima / last of equal maxima as itertools; NaNs (never produced by the generators) are skipped,
 * (NaN, NaN) if nothing is comparable.  n must be < 2^32 (the reference's u32 cast).  Always synchronous when
 * iso_limits is requested. */
int m2s_order_cells_by_distance(const float* distances, size_t n, uint32_t* ordered_indices, float* iso_limits,
                                const m2s_opts* opts);

/* Client pre-step — mesh_to_sdf_client/src/sdf_program.rs:607-632: a glTF scene holds several model instances;
 * the client merges them into the single vertex / index buffer the generator takes:
 *   vertices.extend(model.vertices.map(|v| transform.transform_point3(v.position)))   glam Mat4 (no FMA)
 *   indices.extend(model.indices.map(|i| i + len as u32))                             len = vertices so far
 * and takes the per-axis minmax of the merged vertices as the mesh bounding box.
 * `vertices`/`indices` of every instance and the outputs follow opts->mem_kind; the instance table itself and
 * `bbox` ({xmin,ymin,zmin,xmax,ymax,zmax}, optional) are host memory.  Outputs hold sum(n_vertices) xyz and
 * sum(n_indices) u32. */
typedef struct m2s_instance {
  const void* vertices;        /* first position (3 consecutive f32) */
  size_t n_vertices;
  size_t vertex_stride;        /* bytes between positions; 0 = 12 (packed).  The client's Vertex carries more attributes */
  const uint32_t* indices;
  size_t n_indices;
  float transform[16];         /* glam::Mat4, column-major: x_axis, y_axis, z_axis, w_axis */
} m2s_instance;
int m2s_merge_instances(const m2s_instance* instances, size_t n_instances, float* vertices_out, uint32_t* indices_out,
                        float* bbox, const m2s_opts* opts);

/* ---- queries on a finished grid SDF: sampling and ray marching ------------------------------------------------------
 * What the reference client does with a generated grid on the GPU (mesh_to_sdf_client/shaders/draw_raymarching.wgsl), over a
 * grid that stays where it is: sdf_grid (:118-200), estimate_normal (:202-209), sdf_3d with intersectAABB (:245-287) and
 * compute_tetrahedral_barycenter (:585-640).  IEEE binary32 in the shader's operation order, no FMA.
 * The grid: `grid` and its cell_count[0]*[1]*[2] distances in the library's layout z + y*nz + x*ny*nz (= the shader's get_distance,
 * :92-99), with the client's uniforms (sdf.rs:74-81): start = first_cell, end = first_cell + (float)cell_count * cell_size
 * (Grid::get_last_cell, grid.rs:82-88: one cell past the last centre), cell_size, cell_count.
 * Sampling a point p at `iso`:
 *   any(p < start) || any(p > end)  ->  `outside` (the shader's 100.0).
 *   SNAP         idx = floor((p - (start - cell_size * 0.5)) / cell_size);  d[idx] - iso                        (:128-135)
 *   TRILINEAR    c = (p - start) / cell_size, f = c - floor(c), idx = floor(c); the 8 corners (each - iso) interpolated
 *                along x, then y, then z as a * (1 - f) + b * f                                                       (:137-175)
 *   TETRAHEDRAL  the same idx and f; the six cases of compute_tetrahedral_barycenter in the shader's order (the LAST matching
 *                case wins: all three fractions equal is case 6); dot(bary, samples) left to right                 (:177-197)
 *   Every cell read clamps each index to [0, count - 1], so points between the last centre and `end` read the boundary cells twice.
 * Normal (estimate_normal): eps = 0.01f * max(cs.x, max(cs.y, cs.z)); central differences of six samples (x, y, z order, each with its
 *   own box test); v / sqrtf(v.x*v.x + v.y*v.y + v.z*v.z), and (0, 0, 0) where that length is 0 (WGSL leaves it undefined).  SNAP gives
 *   zero normals almost everywhere, as the shader says.
 * Ray marching (o, dir) (sdf_3d, `iso` for surface_iso, max_steps for MAX_STEPS): o outside the box enters it through intersectAABB with
 *   fminf / fmaxf semantics (the non-NaN operand wins, so zero direction components are well defined); tNear > tFar is a miss:
 *   (0, 0, 0, 1) and 0 steps; otherwise the march starts at o + (tNear + eps) * dir, as the shader writes it (also when the box lies
 *   behind o).  Then up to max_steps times: dist = sample(pos); break if dist < eps; pos += dir * dist.  hit_out[4i..4i+3] = (pos, dist),
 *   steps_out[i] = the advances made; a ray is a HIT when it entered the box and dist < eps; normal_out = estimate_normal(pos) for hits,
 *   (0, 0, 0) otherwise.  `dir` is used as given, not normalised (the client normalises its camera rays).
 * Defined where the shader is not: a point with a NaN coordinate samples as NaN with a NaN normal; a ray with a NaN in its origin or
 *   direction gives NaN x 4, 0 steps and no hit; +-inf coordinates follow the box test (`outside`).
 * Errors (M2S_ERR_BAD_ARG, before any device work): NULL grid or distances; a grid with a zero cell count, a cell size <= 0 or not finite,
 *   or a start / end that is not finite (the shader's box would be empty or undefined); a bad mode; max_steps == 0 (ray march);
 *   every output NULL; NULL inputs with n > 0; m2s_opts.algorithm, x_begin, x_end, x_period or peer_out not zero.  n == 0: M2S_OK.
 * m2s_opts: device, stream / stream_mode, lane, synchronous; mem_kind covers EVERY data pointer (grid distances included).  Host memory
 *   works but copies the whole grid over PCIe in every call: keep the grid on the device (M2S_MEM_DEVICE) for repeated queries.
 *   timings: distance_ms = the kernel, n_units = points or rays. */
enum m2s_sample_mode { M2S_SAMPLE_SNAP = 0, M2S_SAMPLE_TRILINEAR = 1, M2S_SAMPLE_TETRAHEDRAL = 2 };   /* = the shader's MODE_* (:43-45) */
typedef struct m2s_sample_opts {
  uint32_t struct_size;  /* sizeof(m2s_sample_opts) */
  int32_t mode;          /* enum m2s_sample_mode; NULL opts: TRILINEAR, the client's default (sdf_program.rs:264) */
  float iso;             /* NULL opts: 0 */
  float outside;         /* value outside the box; NULL opts: 100.0f */
  uint32_t max_steps;    /* ray march only, >= 1; NULL opts: 100 */
} m2s_sample_opts;
/* points: n_points packed xyz.  value_out: n_points floats; normal_out: 3 per point; either may be NULL, not both. */
int m2s_sample_grid(const m2s_grid* grid, const float* distances, const float* points, size_t n_points, const m2s_sample_opts* sopts,
                    float* value_out, float* normal_out, const m2s_opts* opts);
/* origins, directions: n_rays packed xyz.  hit_out: 4 floats per ray; steps_out: 1 per ray; normal_out: 3 per ray; any may be NULL,
 * not all. */
int m2s_raymarch_grid(const m2s_grid* grid, const float* distances, const float* origins, const float* directions, size_t n_rays,
                      const m2s_sample_opts* sopts, float* hit_out, uint32_t* steps_out, float* normal_out, const m2s_opts* opts);

/* ---- isosurface of a finished grid SDF: marching cubes (no reference counterpart) -----------------------------------------------
 * m2s_grid_isosurface extracts the level set d = iso of `distances` (the grid's cells in the library's layout) as a welded, indexed
 * triangle mesh.  The output is exact: tests/isosurface_model.py reproduces it bit for bit.  IEEE binary32, no FMA.
 * Grid points: the cell centres, pos(i,j,k) = m2s_grid_cell_center = first_cell + (float)i * cell_size per axis; the value at a point
 *   is d[L], L = k + j*nz + i*ny*nz.  A point is INSIDE iff d[L] < iso (a value equal to iso is outside).
 * Vertices: the edge (P, a), a in {x, y, z}, joins P and P + e_a and crosses iff exactly one end is inside.  Each crossing edge gives
 *   exactly one vertex: t = (iso - d0) / (d1 - d0) with d0 the value at P; the axis-a coordinate is p0 + t * (p1 - p0), the other two
 *   are pos(P)'s.  Vertices are ordered by ascending 3*L + a.
 * Triangles: a cell has its lowest corner at P with i < nx-1, j < ny-1, k < nz-1; its case is
 *   sum inside(P + (dx,dy,dz)) << (4*dx + 2*dy + dz).  Triangles are ordered by the lowest corner's L, then by the table's order within
 *   the cell.  The table (mesh_to_sdf_amd/csrc/isosurface_table.h, generated by tools/gen_isosurface_table.py, which states the rule):
 *   on every cube face the crossing edges are paired into segments, and an ambiguous face (two inside corners on a diagonal) keeps
 *   the inside corners SEPARATED, a decision that depends on that face's four signs only, so neighbouring cells agree.  Each cell's
 *   segments form disjoint closed loops; each loop is fanned from its lowest local edge id, loops in order of that id.  At most
 *   5 triangles per cell.
 * Winding: the right-hand normal (v1-v0) x (v2-v0) points from inside to outside (towards increasing d): for an SDF that is negative
 *   inside, outwards, as M2S_SIGN_NORMAL expects of an input mesh.
 * The mesh is closed except where the level set meets the grid boundary: every interior mesh edge is used by as many triangles in one
 *   direction as in the other.  That is one each, except that the fan diagonals of the two cells beside an ambiguous face can join the
 *   same two vertices of that face, so such an edge has two triangles each way.  A value exactly equal to iso can give zero-area
 *   triangles; they are kept.
 * Counting and capacity: vertices_out == indices_out == NULL only counts; exactly one of them NULL is M2S_ERR_BAD_ARG.  counts (host,
 *   2 x uint64 = { n_vertices, n_triangles }) is always written when the arguments are valid ({0, 0} with M2S_ERR_NAN).  A capacity
 *   (3 floats per vertex, 3 uint32 per triangle) below its count is M2S_ERR_BAD_ARG with counts written, and nothing is written
 *   past either capacity; n_vertices >= 2^32 is M2S_ERR_BAD_ARG with counts written (the indices are u32).  Always synchronous.
 * Errors before any device work (M2S_ERR_BAD_ARG): NULL grid, distances or counts; a zero cell count; a cell size <= 0 or not finite;
 *   a non-finite first_cell; a non-finite iso; m2s_opts.algorithm, x_begin, x_end, x_period or peer_out not zero.
 * A count of 1 on some axis: no cells, M2S_OK with zero triangles (crossing edges along the other axes still give vertices).
 * A NaN or +-inf distance anywhere: M2S_ERR_NAN, and no output is written.
 * m2s_opts: device, stream / stream_mode, lane; mem_kind covers the grid and both outputs (host memory copies the grid over PCIe in
 *   every call).  timings: distance_ms = the call's kernels, n_units = grid points. */
int m2s_grid_isosurface(const m2s_grid* grid, const float* distances, float iso, float* vertices_out, uint64_t vertex_capacity,
                        uint32_t* indices_out, uint64_t triangle_capacity, uint64_t* counts, const m2s_opts* opts);

/* ---- isosurface of a narrow band: sparse marching cubes ------------------------------------------------------------------------------
 * m2s_band_isosurface extracts the level set d = iso from the result of m2s_narrow_band_sdf (or any list of grid points and values) with
 * work proportional to the list; no array of distances sized by the grid is made.  What volumeToMesh is to meshToLevelSet in OpenVDB.
 * The result is DEFINED as a filter of m2s_grid_isosurface, so it has no floating-point model of its own:
 *   cells[0 .. n_cells)      strictly ascending L = k + j*nz + i*ny*nz, every L below the cell count; these grid points are ACTIVE.
 *   distances[0 .. n_cells)  their values.
 *   D'                       any dense grid that equals `distances` on the active points and is finite elsewhere;
 *   (V, T) = m2s_grid_isosurface(grid, D', iso), exactly as defined above (inside is d < iso, t = (iso - d0) / (d1 - d0), no FMA,
 *                            vertices by ascending 3*L + a, triangles by cell L then table order).
 * Vertices: the vertices of V whose edge has both ends active, in the same order.
 * Triangles: the triangles of T whose cell has all 8 corners active, in the same order, their indices renumbered to the kept vertices
 *   (every one is kept: the 12 edges of a complete cell join active points).
 * Nothing depends on the values of D' at inactive points: a kept vertex reads 2 active values, a kept cell 8.
 * Corollary: if every cell of a dense grid D whose 8 corners are not all on one side of iso has all 8 corners in the band, the result on
 *   that band equals m2s_grid_isosurface(grid, D, iso) bit for bit in both arrays (every axis with at least 2 points).  For an exact
 *   distance field that holds when the band contains [iso - w, iso + w] with w one cell diagonal sqrt(sx^2 + sy^2 + sz^2).
 * counts (host, 3 x uint64) = { n_vertices, n_triangles, n_open }.  n_open is the number of active points P that own a cell
 *   (i < nx-1, j < ny-1, k < nz-1) with two properties: the cell's 8 corners are not all active; among its active corners at least one
 *   is inside and at least one is outside.  A non-zero value proves the band was too narrow for this iso.  Zero does not prove the
 *   opposite, because cells whose lowest corner is inactive are not visited.
 * Counting and capacity: vertices_out == indices_out == NULL only counts; exactly one of them NULL is M2S_ERR_BAD_ARG.  counts is always
 *   written when the arguments are valid ({0, 0, 0} with M2S_ERR_NAN).  A capacity (3 floats per vertex, 3 uint32 per triangle) below its
 *   count is M2S_ERR_BAD_ARG with counts written, and nothing is written past either capacity; n_vertices >= 2^32 is M2S_ERR_BAD_ARG
 *   with counts written (the indices are u32).  Always synchronous.  n_cells == 0: M2S_OK with {0, 0, 0}.
 * Errors before any device work (M2S_ERR_BAD_ARG): everything m2s_grid_isosurface rejects for grid, iso and opts; a grid of 2^36 or more
 *   cells; NULL counts; NULL cells or distances with n_cells > 0; n_cells above the cell count; a bad mem_kind.
 * cells not strictly ascending, or an entry at or above the cell count: M2S_ERR_BAD_ARG, no output and no count written.  Host memory:
 *   decided on the host, before any device work.  Device memory: decided by a flag the first kernel raises and the host reads with the
 *   counts; no kernel uses an unchecked entry as an index.
 * A NaN or +-inf in distances: M2S_ERR_NAN, no output written, counts {0, 0, 0}.  f32::MAX is finite and legal (a band with
 *   exterior = +inf holds it).
 * m2s_opts: device, stream / stream_mode, lane; mem_kind covers cells, distances and both outputs.  timings: distance_ms = the call's
 *   kernels, n_units = n_cells.
 * Workspace: sized by the grid are the mask (1 bit per point) and one 64-bit list offset per 64 points; the rest is 8 bytes per band
 *   cell (20 with host memory, plus the staged outputs). */
int m2s_band_isosurface(const m2s_grid* grid, const uint64_t* cells, const float* distances, uint64_t n_cells, float iso,
                        float* vertices_out, uint64_t vertex_capacity, uint32_t* indices_out, uint64_t triangle_capacity,
                        uint64_t* counts /* host, 3: n_vertices, n_triangles, n_open */, const m2s_opts* opts);

/* ---- queries on a narrow band: sampling and ray marching without a dense grid ------------------------------------------------------
 * A resident BAND FIELD answers m2s_sample_grid / m2s_raymarch_grid from a narrow band (m2s_narrow_band_sdf's result, or any list of
 * grid points and values): distance and normal lookups at arbitrary points, sphere tracing, at 2048^3 and beyond, where the dense
 * float[nx*ny*nz] costs 32 GiB.  What a sparse level set's sampler and ray intersector are in OpenVDB.  Nothing sized 4 * nx*ny*nz
 * bytes is ever allocated.  The result is DEFINED as the dense call on a grid the band stands for, so it has no model of its own:
 *   cells[0 .. n_cells)      strictly ascending L = k + j*nz + i*ny*nz, every L below the cell count; these grid points are ACTIVE.
 *   distances[0 .. n_cells)  their values, finite.
 *   background_outside, background_inside   both >= 0 and finite.
 *   inside_bits              optional: uint32[nx][ny][ceil(nz / 32)], cell k of a row is bit k & 31 of word k >> 5 (m2s_voxelize's
 *                            bits_out, m2s_narrow_band_sdf's bits_out).
 *   D'[L] = distances[n]           if L == cells[n]                        (every bit, the sign bit included)
 *         = -background_inside     else if inside_bits and its bit (i, j, k) is set
 *         = +background_outside    otherwise
 *   m2s_band_sample(band, points, ...)                 == m2s_sample_grid(grid, D', points, ...)
 *   m2s_band_raymarch(band, origins, directions, ...)  == m2s_raymarch_grid(grid, D', origins, directions, ...)
 * bit for bit in every output, in all three modes.  iso, outside, max_steps, the normals (estimate_normal), the clamped reads at the box
 * faces and the NaN and +-inf rules are those stated above for the dense calls.  IEEE binary32, no FMA.
 * support_out (uint8 per point or ray, may be NULL) is the one extra output.  Sample: how many of the sample's K cell reads (K = 1 SNAP,
 *   8 TRILINEAR, 4 TETRAHEDRAL) hit an active cell, counted after clamping (a cell read twice counts twice); 0 for a point off the box or
 *   with a NaN coordinate.  March: the support of the last sample the march evaluated; 0 for a ray that never marched.  A value of K
 *   means the result used band values only.  For the normal outputs it describes the centre sample, not the six offset ones.
 * Why one sign mask is enough: for a 1-Lipschitz field whose band is at least one cell wide on both sides, a sign change along a grid
 *   line passes through active cells, so the inactive cells fall into regions of one sign each; m2s_voxelize(..., solid = 1) on the same
 *   grid has bit = "centre inside by the Raycast sign" on every inactive cell as soon as interior >= half a cell diagonal (a cell whose
 *   box touches the surface is then active).  The bits are nevertheless taken as given: the definition does not depend on their origin.
 * Why sphere tracing stays safe: with background_outside <= the band's exterior and background_inside <= its interior, |D'| <= |D| on
 *   the inactive cells, so a step never passes the surface that the dense field would not pass.  A zero background stalls a march
 *   that enters the region it fills (dist < eps ends it there).
 * m2s_band_create copies what it needs into device memory the handle owns and keeps no pointer of the caller's: the active mask (1 bit
 *   per grid point), one 64-bit list offset per 64 points, the distances and, if given, the sign mask (1 bit per point).  `cells` is not
 *   kept: after the index is built nothing reads it.  m2s_band_info's device_bytes = 16 * ceil(cells / 64) + 4 * n_cells, + 8 *
 *   ceil(cells / 64) with a sign mask: 2 GiB (3 GiB) + the band at 2048^3, where a dense grid is 32 GiB.  The handle is immutable and bound to the device it was made on.
 *   Always synchronous.  n_cells == 0 is a valid band (all background).  f32::MAX is a legal distance.
 *   Errors before any device work (M2S_ERR_BAD_ARG): NULL grid, out or field opts; field opts' struct_size other than sizeof; a
 *   background that is negative or not finite; what m2s_sample_grid rejects of a grid, or 2^36 or more cells; NULL cells or distances with
 *   n_cells > 0; n_cells above the cell count; m2s_opts.algorithm, x_begin, x_end, x_period or peer_out not zero; a bad mem_kind.
 *   cells not strictly ascending, or an entry at or above the cell count: M2S_ERR_BAD_ARG; a NaN or +-inf distance: M2S_ERR_NAN.  Host
 *   memory: both decided on the host before any device work.  Device memory: decided by the flag the index kernel raises; no later
 *   kernel ever uses an unchecked entry as an index.  No handle is returned in either case (*out = NULL).
 *   m2s_opts: device, stream / stream_mode, lane; mem_kind covers cells, distances and inside_bits.  timings: seed_ms = the index build.
 * The query calls reject what the dense calls reject (a bad mode, max_steps == 0, every output NULL — support_out alone does not count
 *   as an output —, NULL inputs with n > 0, the m2s_opts fields above), a NULL handle, and an m2s_opts.device that is not the handle's
 *   (-1 means the handle's).  mem_kind covers points, rays and outputs; synchronous, stream and lane behave as for m2s_sample_grid;
 *   timings: distance_ms = the kernel, n_units = points or rays.  A handle may serve calls from several threads; destroy it after the
 *   last asynchronous call on it has finished (m2s_band_destroy waits for the device). */
typedef struct m2s_band m2s_band;   /* opaque, immutable after create, bound to one device */
typedef struct m2s_band_field_opts {
  uint32_t struct_size;      /* sizeof(m2s_band_field_opts) */
  float background_outside;  /* D' on inactive cells outside: +background_outside */
  float background_inside;   /* D' on inactive cells whose inside bit is set: -background_inside */
} m2s_band_field_opts;
int m2s_band_create(const m2s_grid* grid, const uint64_t* cells, const float* distances, uint64_t n_cells,
                    const uint32_t* inside_bits /* may be NULL */, const m2s_band_field_opts* fopts, const m2s_opts* opts, m2s_band** out);
void m2s_band_destroy(m2s_band* band);
int m2s_band_info(const m2s_band* band, m2s_grid* grid, uint64_t* n_cells, uint64_t* device_bytes);   /* any output may be NULL */
int m2s_band_sample(const m2s_band* band, const float* points, size_t n_points, const m2s_sample_opts* sopts, float* value_out,
                    float* normal_out, uint8_t* support_out, const m2s_opts* opts);
int m2s_band_raymarch(const m2s_band* band, const float* origins, const float* directions, size_t n_rays, const m2s_sample_opts* sopts,
                      float* hit_out, uint32_t* steps_out, float* normal_out, uint8_t* support_out, const m2s_opts* opts);

/* ---- CSG on narrow bands: union, intersection, difference; a handle's lists back out ---------------------------------------------------
 * m2s_band_csg combines two resident bands on the same grid into a new one without a dense grid: what csgUnion, csgIntersection and
 * csgDifference are in OpenVDB.  m2s_band_export is the inverse of m2s_band_create, so a combined band reaches m2s_band_isosurface
 * (mesh booleans: mesh -> band -> CSG -> band isosurface -> mesh).  The result is DEFINED per grid point, to the bit
 * (tests/band_csg_model.py restates it in numpy).
 * A handle X stands for the dense grid D'_X above.  Per grid point L:
 *   actX[L]   its mask bit: L is one of X's cells.
 *   x         D'_X[L]: the band's value if active, else -X.background_inside if X's inside bit is set, else +X.background_outside.
 *   sX[L]     actX ? (x < 0) : insideX[L]; the inside bit counts as 0 everywhere when X has no sign mask.
 * The negation -X (used only to define the difference): values -x (the sign bit flipped), the same active set,
 *   s_{-X}[L] = actX ? (-x < 0) : !insideX[L], the backgrounds swapped (outside = X's inside, inside = X's outside); D'_{-X} = -D'_X.
 * With a = D'_A[L] and b = D'_B[L] (all finite; comparisons are IEEE, so -0 == +0):
 *   M2S_CSG_UNION         pickB = (b < a) || (a == b && !actA[L]);   r = pickB ? b : a   (every bit)
 *                         active = (actA && !(b < a)) || (actB && !(a < b));   s = sA | sB
 *   M2S_CSG_INTERSECTION  pickB = (b > a) || (a == b && !actA[L]);   r = pickB ? b : a
 *                         active = (actA && !(b > a)) || (actB && !(a > b));   s = sA & sB
 *   M2S_CSG_DIFFERENCE    A \ B = INTERSECTION(A, -B)
 * A cell is active in the result exactly when an operand that supplies its value is active there; on a tie an active operand
 * supplies the bits.
 * The result is a new immutable m2s_band on the same grid and device: the active points ascending, their r, a sign mask equal to s on
 *   EVERY grid point (a result always has a sign mask), and the backgrounds of `fopts`.  fopts == NULL: the min rule,
 *   outside = min(A.outside, B*.outside) and inside = min(A.inside, B*.inside), where B* = B, or -B for the difference.  With it
 *   |D'_R| <= |op(D'_A, D'_B)| on the inactive cells, so sphere tracing stays safe.
 * Consequence 1: if A and B* have the same two backgrounds, both > 0, and the result gets them too, then D'_R == op(D'_A, D'_B) on
 *   every grid point, bit for bit (op = the select above, min or max, on the dense grids): an inactive result cell had its value
 *   supplied by an inactive operand, that is one of the two backgrounds with the sign that s repeats.
 * Consequence 2: let the true fields D_A, D_B be 1-Lipschitz, each band contain [-W, W] with W above one cell diagonal, and all
 *   backgrounds be W.  Then D'_X = clamp(D_X, -W, W), and op of the two is clamp(op(D_A, D_B), -W, W), because clamping is monotone.
 *   op(D_A, D_B) is 1-Lipschitz too, so in a cell its zero level cuts every corner is within one diagonal of a zero: |op| < W there.
 *   Such a corner's value is not a background, so the operand that supplies it is active: all 8 corners are active in the result.
 *   m2s_band_isosurface of the exported result therefore equals m2s_grid_isosurface of the dense op(D'_A, D'_B), with n_open == 0.
 * Caveat: min / max of distance fields has the right zero set and is a lower bound of the distance to it; it is NOT the exact distance
 *   field of the combined solid (near the seams of a union's inside, of an intersection's outside).  The usual level-set CSG.
 * m2s_band_csg: always synchronous (one stream synchronisation, for the count).  a == b is legal.  *out = NULL on every failure.
 *   M2S_ERR_BAD_ARG before any device work: a NULL handle or out; a bad op; handles on different devices; grids that differ in any bit
 *   of first_cell, cell_size or cell_count; fopts with a struct_size other than sizeof or a negative or non-finite background; an
 *   m2s_opts.device that is not the handles' (-1 means theirs); algorithm, x_begin, x_end, x_period or peer_out not zero; a bad mem_kind.
 *   m2s_opts: device, stream / stream_mode, lane.  timings: seed_ms = the call's kernels, n_units = the result's cells.
 *   m2s_band_info of the result: device_bytes by the formula above for a handle with a sign mask; the allocation itself is sized by
 *   the bound min(nA + nB, cells) of the result's count.  Nothing sized 4 bytes per grid point is allocated: the work is the index
 *   words of the operands plus their band cells.
 * m2s_band_export writes cells_out (ascending L) and distances_out (every bit), `capacity` entries each at least, and inside_bits_out
 *   in the caller's layout uint32[nx][ny][ceil(nz / 32)] with the bits at k >= nz zero; all zero for a handle without a sign mask.
 *   Any output may be NULL, not all.  A capacity below the handle's n_cells (m2s_band_info) is M2S_ERR_BAD_ARG and nothing is
 *   written.  Also M2S_ERR_BAD_ARG before any device work: a NULL handle, and the m2s_opts fields above.  mem_kind covers the three
 *   outputs.  Always synchronous.  timings: distance_ms = the call's kernels, n_units = n_cells.  Round trips hold bit for bit:
 *   export(create(lists)) == lists, and a handle recreated from an export answers every query identically.
 * m2s_band_field_info: the handle's backgrounds (struct_size set to sizeof) and whether it has a sign mask; either output may be NULL. */
enum m2s_csg_op { M2S_CSG_UNION = 0, M2S_CSG_INTERSECTION = 1, M2S_CSG_DIFFERENCE = 2 };
int m2s_band_csg(const m2s_band* a, const m2s_band* b, int op, const m2s_band_field_opts* fopts /* NULL = the min rule */,
                 const m2s_opts* opts, m2s_band** out);
int m2s_band_export(const m2s_band* band, uint64_t* cells_out, float* distances_out, uint64_t capacity,
                    uint32_t* inside_bits_out, const m2s_opts* opts);
int m2s_band_field_info(const m2s_band* band, m2s_band_field_opts* fopts_out, int* has_inside);

/* ---- Redistancing a narrow band: true distances after CSG, wider or narrower bands ----------------------------------------------------
 * m2s_band_redistance takes a resident band and returns a resident band with the same zero set, values that are distances again and
 * the half-widths the caller asks for: what LevelSetFilter::normalize / dilate are to csgUnion in OpenVDB.  It closes the chain
 * mesh -> band -> CSG -> redistance -> offset / isosurface / march / CSG again with no dense grid anywhere.  The result is DEFINED per
 * grid point, to the bit (tests/band_redistance_model.py restates it in numpy).
 * Input: a handle X, widths exterior >= 0 and interior >= 0 (finite), max_sweeps.  act, x = D'_X and s = act ? (x < 0) : inside bit
 *   are those of the CSG definition above; h = (hx, hy, hz) is the grid's cell_size; W(L) = s[L] ? interior : exterior.
 *   All arithmetic is IEEE binary32 with no FMA, each operation in the order written; `/` and sqrt are correctly rounded.
 * Frozen set F: an active point L with an axis neighbour M (+-1 in i, j or k, inside the grid) that is active and has s[M] != s[L].
 *   Frozen points keep x[L] in every bit, so the zero level's mesh is untouched.  n_open counts the ordered pairs (L active, M an
 *   inactive axis neighbour, s[M] != s[L]): n_open > 0 proves that the input does not bracket its own zero set there (the idea of
 *   m2s_band_isosurface's n_open).  The call still succeeds; those pairs freeze nothing.  Sign changes between two inactive points
 *   are not looked for: the sign bits are taken as given.
 * Candidate region C: L is in C if it lies in the box |di| <= Kx, |dj| <= Ky, |dk| <= Kz of some frozen point, with
 *   K_a = min(ceil(W(L) / h_a) + 1, n_a): the division in binary32, the ceil of that quotient, computed on the host; K is taken per
 *   side, so two box dilations of F are selected by s.  Points outside C have u = +inf for ever, by definition: this is what makes
 *   the work proportional to the band without a causality argument.
 * Start: u0[L] = |x[L]| on F, +inf elsewhere.
 * One sweep, Jacobi: every u(n+1) is computed from u(n) only.  For L in C \ F:
 *   c(v, M) = v <= W(M) ? v : +inf (the cut-off applies to frozen values too).
 *   Per axis a, m_a = the min over the two axis neighbours M inside the grid with s[M] == s[L] of c(u(n)[M], M); +inf if there is none.
 *   The three (m_a, h_a) sorted ascending by m, stably in the axis order i, j, k (swap on a strict < only: (i,j), (j,k), (i,j)):
 *   a1 <= a2 <= a3 with h1, h2, h3 and w_n = 1 / (h_n * h_n).
 *     t = a1 + h1
 *     if (t > a2) { d2 = a2 - a1;  A = w1 + w2;  B = w2 * d2;  q2 = B * d2;  C = q2 - 1;  D = B * B - A * C;  D = D > 0 ? D : 0;
 *                   t = a1 + (B + sqrt(D)) / A;
 *       if (t > a3) { d3 = a3 - a1;  A = A + w3;  B = B + w3 * d3;  C = (q2 + (w3 * d3) * d3) - 1;  D = B * B - A * C;  D = D > 0 ? D : 0;
 *                     t = a1 + (B + sqrt(D)) / A; } }
 *   A +inf neighbour never enters the arithmetic (the branches exclude it), and a point with a1 = +inf stays +inf.
 *   u(n+1)[L] = t < u(n)[L] ? t : u(n)[L]   (a NaN t, which needs a cell size whose square underflows, changes nothing).
 * Sweeps run until one changes no bit or max_sweeps have run.  sweeps = the number of sweeps that changed something; converged = the
 *   last one run changed nothing.  Further sweeps after convergence change nothing, so the library reads its change flags every few
 *   sweeps.  max_sweeps == 0: the default 2 * (Kx + Ky + Kz) + 8 with the larger side's K; a cap, not a target.
 * IT MUST BE JACOBI.  With asynchronous, in-place updates the iteration converges to DIFFERENT BITS, because the binary32 update is not
 *   monotone across its branches: a Gauss-Seidel sweep, a multi-sweep LDS tile, a fast iterative method or anything else that lets a
 *   point see a value of the same sweep cannot meet this definition.  The library keeps two value buffers.
 * Result: a new immutable m2s_band on the same grid and device.  Active set: F and the L in C with u[L] <= W(L).  Values: x[L] on F,
 *   otherwise s[L] ? -u : +u.  Sign mask: s on EVERY grid point.  Backgrounds: fopts', or by default outside = exterior and inside =
 *   interior.  Input cells that are neither frozen nor reached are dropped: their values were not distances.  F empty: an empty band
 *   with the sign mask.
 * Accuracy (first order; measured with the numpy model): a sphere of radius 0.6 on cells (0.05, 0.04, 0.0625), max
 *   error 0.14 / 0.30 cells of 0.0625 at widths of 3 / 5 such cells; the seam of a union of two spheres 0.21 cells where the min rule of
 *   m2s_band_csg is off by 1.20.
 * Always synchronous.  *out = NULL on every failure.  M2S_ERR_BAD_ARG before any device work: a NULL handle, ropts or out; a
 *   struct_size other than sizeof (ropts, fopts, info_out); negative or non-finite widths or backgrounds; an m2s_opts.device that is not
 *   the handle's (-1 means its own); algorithm, x_begin, x_end, x_period or peer_out not zero; a bad mem_kind.
 *   m2s_opts: device, stream / stream_mode, lane.  timings: seed_ms = the topology (s, F, C and its index), distance_ms = the sweeps,
 *   total_ms = the whole call, n_units = the result's cells.  m2s_band_info of the result: device_bytes by the formula for a handle
 *   with a sign mask.  Nothing sized 4 bytes per grid point is allocated: during the call six or seven words per 64 grid points and
 *   33 bytes per candidate (two values, six 32-bit neighbour places, a byte); 2^32 - 1 or more candidates are M2S_ERR_BAD_ARG.
 *   info_out (may be NULL; set struct_size): the figures above and n_candidates = |C|. */
typedef struct m2s_band_redistance_opts { uint32_t struct_size; float exterior, interior; uint32_t max_sweeps; } m2s_band_redistance_opts;
typedef struct m2s_band_redistance_info { uint32_t struct_size, sweeps, converged, reserved; uint64_t n_frozen, n_open, n_candidates; } m2s_band_redistance_info;
int m2s_band_redistance(const m2s_band* band, const m2s_band_redistance_opts* ropts, const m2s_band_field_opts* fopts /* NULL = the widths */,
                        const m2s_opts* opts, m2s_band** out, m2s_band_redistance_info* info_out /* may be NULL */);

/* ---- Smoothing a narrow band: mean, Laplacian, mean-curvature flow, everywhere or inside a region -------------------------------------
 * m2s_band_filter takes a resident band and returns a resident band on the same cells whose values have been smoothed: what
 * LevelSetFilter::mean / gaussian / laplacian / meanCurvature are in OpenVDB.  It rounds the crease a CSG leaves into a fillet, fairs a
 * re-meshed surface and removes the staircase of a coarse band, with no dense grid and nothing leaving the device.  The result is
 * DEFINED per grid point, to the bit (tests/band_filter_model.py restates it in numpy).
 * Input: a handle X, a kind, iterations, and optionally a region handle `where` on the same grid.  act, x = D'_X[L] and
 *   s = act ? (x < 0) : inside bit are those of the CSG definition above; h = (h_i, h_j, h_k) is the grid's cell_size.
 *   All arithmetic is IEEE binary32 with no FMA, each operation in the order written; `/` is correctly rounded.
 * Host constants, computed in binary32 and handed to the kernels as values: r_a = 1 / h_a, w_a = r_a * r_a,
 *   dt = 1 / (2 * ((w_i + w_j) + w_k)); for cubic cells dt = h^2 / 6.
 * The field a pass reads: v[L] is the current value where L is active; elsewhere it is D'_X[L], that is +background_outside, or
 *   -background_inside when X's inside bit is set (X's own backgrounds, not the result's).  Inactive points never change.
 * Neighbour reads: N(di, dj, dk) is v at (clamp(i + di, 0, nx - 1), clamp(j + dj, 0, ny - 1), clamp(k + dk, 0, nz - 1)): the box faces
 *   use clamped reads, as in m2s_sample_grid.  N(+a) steps +1 along axis a alone, N(+a-b) steps +1 along a and -1 along b.  c = N(0,0,0).
 * One pass, for an active L, computes a candidate:
 *   M2S_FILTER_LAPLACIAN       t_a = ((N(+a) - c) + (N(-a) - c)) * w_a
 *                              cand = c + dt * ((t_i + t_j) + t_k)
 *   M2S_FILTER_MEAN            one iteration is three passes, axis i, then j, then k.  Pass a:
 *                              cand = ((N(-a) + c) + N(+a)) / 3
 *                              The separable 3 x 3 x 3 box, as in OpenVDB.  `width` must be 1; the field exists so that the struct can
 *                              grow.  Four iterations of M2S_FILTER_MEAN approximate OpenVDB's Gaussian.
 *   M2S_FILTER_MEAN_CURVATURE  g_a = (N(+a) - N(-a)) * (0.5f * r_a);   t_a as for M2S_FILTER_LAPLACIAN
 *                              for ab in ij, ik, jk:  x_ab = ((N(+a+b) - N(+a-b)) - (N(-a+b) - N(-a-b))) * (0.25f * (r_a * r_b))
 *                              q_a = g_a * g_a
 *                              num = ((t_i*(q_j+q_k) + t_j*(q_i+q_k)) + t_k*(q_i+q_j)) - 2 * (((g_i*g_j)*x_ij + (g_i*g_k)*x_ik) + (g_j*g_k)*x_jk)
 *                              g2 = (q_i + q_j) + q_k
 *                              cand = g2 > 0 ? c + dt * (num / g2) : c
 *                              One explicit step of phi_t = kappa |grad phi|, kappa the sum of the principal curvatures; 19 points.
 *   next[L] = (W[L] && isfinite(cand)) ? cand : c.  W[L] is 1 when `where` is NULL, else s_where[L]: the CSG definition's s of the
 *   `where` handle, read as "inside the region".  A cell outside the region evaluates no candidate and keeps every bit through every
 *   pass.  A non-finite cand of a cell inside the region keeps c and counts once, per cell and pass, in n_nonfinite; values of
 *   +-f32::MAX in a band are legal and make this reachable.  (A NaN g2 fails g2 > 0, so that cand is c: finite, not counted.)
 * IT MUST BE JACOBI.  Every pass reads the previous pass's values only; the library keeps two value buffers, as for redistancing.
 *   An in-place pass ends in different bits, and so does a tile that runs several passes in local memory.
 * Result: a new immutable m2s_band on the same grid and device.  The active set is X's.  The values r are those after `iterations`
 *   iterations.  Sign mask: on EVERY grid point, act ? (r < 0) : s.  Backgrounds: fopts', or X's by default.  m2s_band_info's
 *   device_bytes follows the formula for a handle with a sign mask.  An empty band gives an empty band with the sign mask.
 * info_out (may be NULL; set struct_size): passes = iterations, or 3 * iterations for M2S_FILTER_MEAN; n_changed = the active cells
 *   whose final bits differ from x; n_sign_flips = the active cells with (r < 0) != (x < 0); max_change = the largest fabsf(r - x)
 *   over the active cells (0 for an empty band; it may be +inf); n_nonfinite as above.  All are deterministic: integer sums and a maximum.
 * What the definition does NOT promise: the result is not a distance field, follow it with m2s_band_redistance.  Cells at the band's
 *   rim read the backgrounds, that is the clamped field, so their stencils see a kink.  The band should hold the zero set with two
 *   cells to spare, plus the distance it is meant to move.
 * Accuracy (measured with the numpy model): on a sphere the zero set follows R^2 = R0^2 - 4 n dt under
 *   M2S_FILTER_MEAN_CURVATURE and M2S_FILTER_LAPLACIAN to a few hundredths of a cell over 8 iterations.
 * Always synchronous: one synchronisation at the end, for the info, none between passes.  *out = NULL on every failure.
 *   M2S_ERR_BAD_ARG before any device work: a NULL band, fl or out; a struct_size other than sizeof (fl, fopts, info_out); a bad kind;
 *   iterations == 0 or above 65 536; width != 1; a negative or non-finite background; a `where` on another device, or on a grid that
 *   differs in any bit of first_cell, cell_size or cell_count; n_cells + 2 >= 2^32; an m2s_opts.device that is not the handle's (-1
 *   means its own); algorithm, x_begin, x_end, x_period or peer_out not zero; a bad mem_kind.  band == where is legal.
 *   m2s_opts: device, stream / stream_mode, lane.  timings: seed_ms = the neighbour table, distance_ms = the passes, total_ms = the
 *   whole call, n_units = the cell count.
 * Memory during the call: per active cell two values and 24 (M2S_FILTER_MEAN, M2S_FILTER_LAPLACIAN) or 72 (M2S_FILTER_MEAN_CURVATURE)
 *   bytes of 32-bit neighbour places plus a byte, 33 or 81 bytes in all; per 64 grid points the result's sign word (with the copies of
 *   the mask and its offsets, the result itself).  Nothing sized 4 bytes per grid point is allocated.  An inactive neighbour is one of
 *   two extra places behind the values, which is why n_cells + 2 must stay below 2^32. */
enum m2s_filter_kind { M2S_FILTER_MEAN = 0, M2S_FILTER_LAPLACIAN = 1, M2S_FILTER_MEAN_CURVATURE = 2 };
typedef struct m2s_band_filter_opts { uint32_t struct_size; int32_t kind; uint32_t iterations; uint32_t width; } m2s_band_filter_opts;
typedef struct m2s_band_filter_info { uint32_t struct_size, passes; float max_change; uint32_t reserved;
                                      uint64_t n_changed, n_sign_flips, n_nonfinite; } m2s_band_filter_info;
int m2s_band_filter(const m2s_band* band, const m2s_band* where /* may be NULL = everywhere */, const m2s_band_filter_opts* fl,
                    const m2s_band_field_opts* fopts /* NULL = the input's backgrounds */, const m2s_opts* opts,
                    m2s_band** out, m2s_band_filter_info* info_out /* may be NULL */);

/* ---- Moving a narrow band: advection by a velocity, propagation along the normal by a speed ----------------------------------------------
 * m2s_band_advect takes a resident band and a field with one entry per cell, and returns a resident band on the same cells whose
 * values have taken `steps` explicit first-order upwind steps of dt: what LevelSetAdvect, and the step under LevelSetMorph, are in
 * OpenVDB with FIRST_BIAS.  A particle surface is carried by a flow, a part thickened by an amount that varies over its surface, a
 * front propagated at a given speed, one shape morphed into another (speed = minus the target's value), with no dense grid and nothing
 * leaving the device.  The result is DEFINED per grid point, to the bit (tests/band_advect_model.py restates it in numpy).
 * Input: a handle X, a kind, steps, dt and the field.  act, x = D'_X[L], s, the clamped neighbour reads N(+a), N(-a) and c = N(0,0,0)
 *   are exactly those of m2s_band_filter's definition above: v[L] is the current value where L is active and D'_X[L] elsewhere (X's own
 *   backgrounds, not the result's).  Inactive points never change.  h = (h_i, h_j, h_k) is the grid's cell_size.
 *   All arithmetic is IEEE binary32 with no FMA, each operation in the order written; sqrtf is correctly rounded.
 * Host constants, computed in binary32 and handed to the kernels as values: r_a = 1 / h_a.
 * field: host or device memory as m2s_opts.mem_kind says, n_cells x 3 floats (M2S_ADVECT_VELOCITY: u_i, u_j, u_k of a cell side by
 *   side) or n_cells floats (M2S_ADVECT_NORMAL: F), in list order: entry n belongs to the band's n-th cell in ascending order, the
 *   order of m2s_band_export.  One field and one dt serve the whole call.
 * Moving cells: an active cell is MOVING when any of its three velocity components != 0 (M2S_ADVECT_VELOCITY), or its speed != 0
 *   (M2S_ADVECT_NORMAL); -0.0 is 0 and a NaN counts as moving.  A cell that is not moving evaluates no candidate and keeps every bit
 *   through every step.
 * One step, for a moving L:  Dm_a = (c - N(-a)) * r_a,  Dp_a = (N(+a) - c) * r_a, and
 *   M2S_ADVECT_VELOCITY  phi_t + u . grad phi = 0, each axis differenced against the wind:
 *                        t_a = u_a > 0 ? u_a * Dm_a : u_a * Dp_a
 *                        cand = c - dt * ((t_i + t_j) + t_k)
 *   M2S_ADVECT_NORMAL    phi_t + F |grad phi| = 0, Godunov's scheme; F > 0 moves the surface outward.
 *                        With pos(v) = v > 0 ? v : 0 and neg(v) = v < 0 ? v : 0:
 *                        A_a = F > 0 ? pos(Dm_a) : neg(Dm_a)
 *                        B_a = F > 0 ? neg(Dp_a) : pos(Dp_a)
 *                        qa = A_a * A_a, qb = B_a * B_a, q_a = qb > qa ? qb : qa
 *                        g = sqrtf((q_i + q_j) + q_k)
 *                        cand = c - dt * (F * g)
 *   next[L] = isfinite(cand) ? cand : c.  A non-finite cand of a moving cell keeps c and counts once, per cell and step, in
 *   n_nonfinite; non-finite entries of `field` are accepted and end there, and so do values of +-f32::MAX in a band.
 * IT MUST BE JACOBI.  Every step reads the previous step's values only; the library keeps two value buffers, as for redistancing.
 *   An in-place step ends in different bits, and so does a tile that runs several steps in local memory.
 * Result: a new immutable m2s_band on the same grid and device.  The active set is X's.  The values r are those after the last
 *   step.  Sign mask: on EVERY grid point, act ? (r < 0) : s.  Backgrounds: fopts', or X's by default.  m2s_band_info's device_bytes
 *   follows the formula for a handle with a sign mask.  An empty band gives an empty band with the sign mask; `field` may then be NULL.
 * info_out (may be NULL; set struct_size): steps; n_moving = the moving cells; n_changed = the active cells whose final bits differ
 *   from x; n_sign_flips = the active cells with (r < 0) != (x < 0); max_change = the largest fabsf(r - x) over the active cells (0 for
 *   an empty band; it may be +inf); n_nonfinite as above; max_cfl = the largest over the active cells of
 *   dt * ((|u_i|*r_i + |u_j|*r_j) + |u_k|*r_k) (M2S_ADVECT_VELOCITY) or dt * (|F| * ((r_i + r_j) + r_k)) (M2S_ADVECT_NORMAL), taken as a
 *   maximum of the bit patterns of the values that are not NaN; +inf is possible; 0 for an empty band.  All are deterministic: integer
 *   sums and maxima.
 * What the definition does NOT promise: the result is not a distance field.  Cells at the band's rim read the backgrounds, that is
 *   the clamped field, so error enters from the upwind rim and travels at the flow's speed.  A caller moves the surface by less than
 *   the half-width minus two cells and then calls m2s_band_redistance, which keeps the cells next to the zero set in every bit and
 *   re-grows the band around it.  Stability needs max_cfl <= 1: the call reports the figure and does not enforce it, and the
 *   definition holds above 1 too.  First-order upwind is diffusive; `scheme` must be 0 and exists so that a higher order can follow.
 * Accuracy (measured with the numpy model): a sphere carried a few cells by a constant velocity, or grown or shrunk
 *   along its normal, keeps its zero set within about a quarter of a cell; a quarter turn about an off-centre axis within about a cell.
 * Always synchronous: one synchronisation at the end, for the info, none between steps.  *out = NULL on every failure.
 *   M2S_ERR_BAD_ARG before any device work: a NULL band, aopts or out; a struct_size other than sizeof (aopts, fopts, info_out); a bad
 *   kind; scheme != 0; steps == 0 or above 65 536; a dt that is not finite or not > 0; a NULL field with n_cells > 0; a negative or
 *   non-finite background; n_cells + 2 >= 2^32; an m2s_opts.device that is not the handle's (-1
 *   means its own); algorithm, x_begin, x_end, x_period or peer_out not zero; a bad mem_kind.
 *   m2s_opts: device, stream / stream_mode, lane, mem_kind (where `field` lives).  timings: seed_ms = the neighbour table and the
 *   moving bytes, distance_ms = the steps, total_ms = the whole call, n_units = the cell count.
 * Memory during the call: per active cell two values, 24 bytes of 32-bit neighbour places and a byte, 33 bytes, plus the copy of a
 *   host caller's field, 12 or 4 bytes (a device caller's field is read where it lies); per 64 grid points the result's sign word
 *   (with the copies of the mask and its offsets, the result itself).  Nothing sized 4 bytes per grid point is allocated.  An inactive
 *   neighbour is one of two extra places behind the values, which is why n_cells + 2 must stay below 2^32. */
enum m2s_advect_kind { M2S_ADVECT_VELOCITY = 0, M2S_ADVECT_NORMAL = 1 };
typedef struct m2s_band_advect_opts { uint32_t struct_size; int32_t kind; uint32_t steps; uint32_t scheme /* must be 0 */; float dt; } m2s_band_advect_opts;
typedef struct m2s_band_advect_info { uint32_t struct_size, steps; float max_change, max_cfl;
                                      uint64_t n_moving, n_changed, n_sign_flips, n_nonfinite; } m2s_band_advect_info;
int m2s_band_advect(const m2s_band* band, const float* field /* list order: n_cells x 3 (VELOCITY) or n_cells (NORMAL) */,
                    const m2s_band_advect_opts* aopts, const m2s_band_field_opts* fopts /* NULL = the input's backgrounds */,
                    const m2s_opts* opts, m2s_band** out, m2s_band_advect_info* info_out /* may be NULL */);

/* ---- Resampling a narrow band onto another grid under a similarity: crop, pad, move, turn, scale, refine --------------------------------
 * m2s_band_resample evaluates a resident band at the cell centres of another grid, under an optional map from target space to source
 * space, and returns a new resident band on that grid with its sign mask on every point: what GridTransformer / resampleToMatch are
 * in OpenVDB.  It lets a field leave the grid it was born on: two parts voxelised on their own boxes meet in m2s_band_csg, a band is
 * cropped to a region, a finished field is placed somewhere else, a band goes to finer cells before m2s_band_isosurface.  Follow it
 * with m2s_band_redistance, as OpenVDB follows its resampling with a renormalisation.  The result is DEFINED per target grid point, to
 * the bit (tests/band_resample_model.py restates it in numpy).
 * Input: a handle X on its grid Gs, a target grid T, a mode (m2s_sample_mode), to_source = m, the row-major 3 x 4 map from target
 *   space to source space, and value_scale > 0.  The library takes m as given and inverts nothing.  All arithmetic is IEEE binary32
 *   with no FMA, each operation in the order written.
 * Per target point L = k + j*nz + i*ny*nz of T:
 *   Centre        p = m2s_grid_cell_center(T, (i, j, k)), that is first_cell + (float)idx * cell_size per axis.
 *   Source point  q_a = ((m[4a] * p.x + m[4a+1] * p.y) + m[4a+2] * p.z) + m[4a+3] for a = 0, 1, 2.
 *   Sample        (v, support) = m2s_band_sample(X, q) with `mode`, iso = 0 and outside = X.background_outside, exactly as defined
 *                 above: the clamped reads between the last centre and `end`, the `outside` and NaN rules, support counted after
 *                 clamping.  K = 1 (SNAP), 8 (TRILINEAR), 4 (TETRAHEDRAL).
 *   Value         r = v * value_scale.
 *   Active set    active[L] = (support == K) && isfinite(r).  A point with support == K and a non-finite r is inactive and counts in
 *                 n_nonfinite; cells of +-f32::MAX and a scale above 1 make this reachable.
 *   Sign          s[L] = active ? (r < 0) : sX[c].  c is the cell the SNAP rule of m2s_sample_grid reads for q, and sX is the CSG
 *                 definition's s of X: act ? (x < 0) : inside bit.  s[L] = 0 when q is off the source box or has a NaN coordinate.
 *                 It is the SNAP rule and not v < 0: a zero background is legal and has no sign.
 * Result: a new immutable m2s_band on T and on X's device.  The active points ascending with their r; a sign mask equal to s on EVERY
 *   target point; the backgrounds of `fopts`, or by default X.background_outside * value_scale and X.background_inside * value_scale
 *   (a default that comes out non-finite is M2S_ERR_BAD_ARG).  m2s_band_info's device_bytes follows the formula for a handle with a
 *   sign mask.
 * info_out (may be NULL; set struct_size): n_cells = the result's cell count.  n_partial = the points on the source box with
 *   0 < support < K: the rim the interpolation loses.  n_nonfinite as above.  n_open = the ordered pairs (L active, M an inactive axis
 *   neighbour inside T, s[M] != s[L]), with the meaning it has in m2s_band_redistance: the result does not bracket its own zero set
 *   there, which is what happens when the target cells outgrow the source band.
 * Consequence 1: SNAP, the identity map and T == Gs give X back: the cells and values keep every bit and the sign mask is sX on every
 *   point.  This holds on any grid, not only dyadic ones, because the SNAP index has half a cell of slack.  TRILINEAR has no such
 *   property: (first + i*cs - first) / cs need not be i, and a point needs all 8 corners active.
 * Consequence 2: SNAP with a target grid that is the source grid shifted by whole cells is crop and pad.  A target centre that falls
 *   exactly on the source box's `end` face (one cell past the last centre) is still on the box and repeats the last cell: the clamped
 *   reads.  Cropping the padded result back to Gs drops that layer, so pad and crop return X in every bit.
 * Consequence 3: for a similarity p = s R q + t (the map from source space to target space, of which m is the inverse) with
 *   value_scale = s, and a distance field, r is the moved solid's distance within the interpolation error.  Measured with the numpy
 *   model: a sphere on cells of about 0.03 turned, scaled by 0.75 and moved onto cells (0.05, 0.04, 0.0625) is off by
 *   at most 0.0075 cells of 0.0625 under TRILINEAR, 0.0101 under TETRAHEDRAL and 0.311 under SNAP.
 * What the definition does NOT promise: the result is not a distance field after TRILINEAR or TETRAHEDRAL, follow it with
 *   m2s_band_redistance.  A map that is not a similarity is accepted and gives something that is not a distance at all.  In the outer
 *   half cell of the source box the field is constant extrapolation, because of the clamped reads: pad the source.  Resampling to much
 *   coarser cells aliases, as OpenVDB's point samplers do.
 * Always synchronous, with one synchronisation inside the call, for the count: the values are allocated at their true size.  *out =
 *   NULL on every failure.  M2S_ERR_BAD_ARG before any device work: a NULL band, target or out; a struct_size other than sizeof (ropts,
 *   fopts, info_out); a bad mode; a non-finite entry of to_source; a value_scale that is not finite or not > 0; what m2s_band_create
 *   rejects of a grid, 2^36 or more cells included; negative or non-finite backgrounds; an m2s_opts.device that is not the handle's (-1
 *   means its own); algorithm, x_begin, x_end, x_period or peer_out not zero; a bad mem_kind.
 *   m2s_opts: device, stream / stream_mode, lane.  timings: seed_ms = the mask pass and the scan, distance_ms = the value pass,
 *   total_ms = the whole call, n_units = the result's cells.
 * Memory during the call: per 64 target points the result's three index words plus 4 bytes per 64 words and 8 per 4096 words of
 *   counts; per result cell its value.  Nothing sized 4 bytes per point of either grid is allocated. */
typedef struct m2s_band_resample_opts { uint32_t struct_size; int32_t mode; float to_source[12]; float value_scale; } m2s_band_resample_opts;   /* 60 bytes */
typedef struct m2s_band_resample_info { uint32_t struct_size, reserved; uint64_t n_cells, n_partial, n_nonfinite, n_open; } m2s_band_resample_info;   /* 40 bytes */
int m2s_band_resample(const m2s_band* band, const m2s_grid* target, const m2s_band_resample_opts* ropts /* NULL = identity, TRILINEAR, 1 */,
                      const m2s_band_field_opts* fopts /* NULL = the input's backgrounds times value_scale */, const m2s_opts* opts,
                      m2s_band** out, m2s_band_resample_info* info_out /* may be NULL */);

/* ---- Connected components of a narrow band: label, measure, select ------------------------------------------------------------------------
 * m2s_band_components labels the connected components of a resident band's active cells and measures each; m2s_band_select returns the
 * band with some of them erased: what segmentActiveVoxels / segmentSDF and "keep the largest component" / "drop islands below N voxels"
 * are in OpenVDB, split() in trimesh and ndimage.label in scipy.  They take apart what the other band calls produce: the slivers and
 * floating debris m2s_band_csg leaves where two surfaces nearly coincide, the loose parts of a voxelised scan, the two halves of a part
 * that a difference cut in two.  Both are DEFINED to the bit (tests/band_components_model.py restates them in numpy).
 *
 * m2s_band_components.  The graph's nodes are the band's active cells.  Two cells are joined when their (i, j, k) differ by at most 1 on
 *   every axis and by 1 on at most 1, 2 or 3 axes: connectivity 6 (faces), 18 (faces and edges) or 26 (faces, edges and corners).  There
 *   is NO clamping: a step off the grid finds no neighbour, unlike the filters' clamped step.  The values play no part.
 *   Numbering: the components are numbered 0 .. C-1 in ascending order of their smallest linear cell index L = k + j*nz + i*ny*nz, the
 *   raster numbering of scipy.ndimage.label.  labels_out[r] is the component of list place r (the r-th active cell in ascending L,
 *   the order of m2s_band_export), n_cells entries.  M2S_LABEL_NONE is never written; it is a value for callers to mark cells with.
 *   Per component, components_out[c] holds: first_cell = its smallest L; n_cells; n_negative = its cells whose value is < 0 (-0.0 is
 *   not), a volume proxy for a band that holds a solid's skin; lo / hi = the inclusive bounding box of its (i, j, k).  Everything
 *   reported is an integer, so the atomics that gather it give the same bits in any order.
 *   Protocol: *n_components_out = C is written whenever the arguments are valid.  labels_out == components_out == NULL only counts
 *   (either may be NULL alone).  A `capacity` below C with components_out given is M2S_ERR_BAD_ARG with C written and components_out
 *   untouched: call again with room.  Always synchronous.  m2s_opts.mem_kind covers labels_out and components_out.  An empty band
 *   gives 0 components and M2S_OK.
 *   M2S_ERR_BAD_ARG before any device work: a NULL band or count pointer; a copts->struct_size other than sizeof; a connectivity other
 *   than 6, 18 or 26 (copts == NULL means 6); an m2s_opts.device that is not the handle's (-1 means its own); algorithm, x_begin,
 *   x_end, x_period or peer_out not zero; a bad mem_kind; 2^32 - 1 or more active cells: labels and parents are 32-bit, the limit
 *   m2s_band_redistance puts on its candidates.  m2s_opts: device, stream / stream_mode, lane.  timings: distance_ms = total_ms = the
 *   whole call, n_units = the band's cells.
 *   Method: a lock-free union-find over the list places with parent[r] <= r; each cell is united with the active cells of the backward
 *   half of its stencil, the larger root hooked under the smaller by compare-and-swap.  A component's root is its smallest place in any
 *   order of execution, so the result is deterministic without sweeps.  (Label propagation in Jacobi sweeps would need as many sweeps
 *   as the cell graph's diameter, thousands at 2048^3.)
 *   Memory during the call: 4 bytes per active cell beside the outputs (twice that when labels_out is host memory, or NULL with
 *   components_out given), and 8 bytes per 4096 cells of scan partials.  Nothing is sized per grid point or per mask word.
 *
 * m2s_band_select.  Cell r (list place) is KEPT iff labels[r] < n_keep && keep[labels[r]] != 0; every other cell is DROPPED.
 *   M2S_LABEL_NONE and any label from elsewhere therefore drop the cell, and no validation pass exists.  labels has n_cells entries,
 *   keep n_keep bytes; the labels need not come from m2s_band_components.
 *   Result: a new immutable m2s_band on the same grid and device.  Its cells are the kept cells, ascending, with every bit of their
 *   values.  A dropped cell becomes inactive and outside.  Backgrounds: fopts', or the input's by default.  Sign mask, on EVERY grid
 *   point as for every derived handle:
 *     a kept cell              v < 0
 *     a dropped cell           0
 *     an inactive point of the input whose inside bit is clear    0
 *     an inactive point of the input whose inside bit is set      CLEARED iff, in its own k-row (same i, j), the nearest active cell
 *                              of the input towards +k and the nearest towards -k are dropped cells, for every side that has one, and
 *                              at least one side has one; otherwise it keeps its bit.
 *   An input without a sign mask has no such points.  This is a scan-line flood like OpenVDB's signedFloodFill, restricted to what an
 *   erased component owned: without it m2s_band_sample and m2s_band_raymarch would still see the solid interior of an erased island.
 *   THE LIMIT: the rule knows rows, not solids.  Erasing the band around a CAVITY (the inner skin of a hollow part) turns the cavity
 *   into outside, which it already was, and leaves the row segments of solid that ended on it bracketed on one side only by a kept
 *   cell: they keep their bit, but the cavity's skin is gone, so the field steps from -background_inside to +background_outside with
 *   no band cell between.  A row segment of solid between two erased cavities is cleared.  Erase islands, not voids.
 *   info_out (may be NULL; set struct_size): n_cells = the result's cells, n_dropped = the input's cells minus those, n_sign_cleared
 *   = the inactive points whose inside bit was cleared.  m2s_band_info of the result: device_bytes by the formula for a handle with a
 *   sign mask.
 *   Always synchronous.  *out = NULL on every failure.  m2s_opts.mem_kind covers labels and keep.  M2S_ERR_BAD_ARG before any device
 *   work: a NULL band, labels or out; keep == NULL with n_keep > 0; a struct_size other than sizeof (fopts, info_out); a negative or
 *   non-finite background; the m2s_opts fields as above.  timings: seed_ms = total_ms = the three launches, n_units = the result's cells.
 *   Memory during the call: the result, 4 bytes per 256 mask words and 8 per 4096 of counts, and a host caller's labels and keep.  The
 *   row search loads at most nz / 64 + 1 mask words per direction, and only for words that have inactive-inside bits. */
enum m2s_connectivity { M2S_CONNECT_6 = 6, M2S_CONNECT_18 = 18, M2S_CONNECT_26 = 26 };
typedef struct m2s_band_components_opts { uint32_t struct_size; int32_t connectivity; } m2s_band_components_opts;   /* 8 bytes */
typedef struct m2s_band_component { uint64_t first_cell, n_cells, n_negative; uint32_t lo[3], hi[3]; } m2s_band_component;   /* 48 bytes */
typedef struct m2s_band_select_info { uint32_t struct_size, reserved; uint64_t n_cells, n_dropped, n_sign_cleared; } m2s_band_select_info;   /* 32 bytes */
#define M2S_LABEL_NONE 0xffffffffu
int m2s_band_components(const m2s_band* band, const m2s_band_components_opts* copts /* NULL = 6 */, const m2s_opts* opts,
                        uint32_t* labels_out /* n_cells, list order; may be NULL */, m2s_band_component* components_out /* may be NULL */,
                        uint64_t capacity, uint64_t* n_components_out /* host */);
int m2s_band_select(const m2s_band* band, const uint32_t* labels /* n_cells */, const uint8_t* keep, uint64_t n_keep,
                    const m2s_band_field_opts* fopts /* NULL = the input's backgrounds */, const m2s_opts* opts,
                    m2s_band** out, m2s_band_select_info* info_out /* may be NULL */);

/* ---- Measures of a narrow band: area, volume, centroid, per component ----------------------------------------------------------------------
 * m2s_band_measure measures the level set d = iso of a resident band field as m2s_band_isosurface would mesh it, without building that
 * mesh: what LevelSetMeasure is in OpenVDB and area / volume / center_mass in trimesh.  It answers "what is the interference volume of
 * these two parts" after m2s_band_csg, "how big was the debris" after m2s_band_select, "how much material did that add" after an
 * offset.  Nothing is sized by the grid, the band or the triangle count: the workspace is one record of raw sums per group.
 *
 * Groups.  labels == NULL: one group, measures_out[0].  Otherwise labels has n_cells entries in list order (what m2s_band_components
 *   returns; device or host memory as m2s_opts.mem_kind says) and measures_out n_groups entries.  A complete cell belongs to the group
 *   labels[r] of its base corner's list place r; a counted vertex, and an open cell, to the group of the point that owns the edge or
 *   the cell.  Places with labels[r] >= n_groups are skipped (their cell, their vertices) and counted in n_skipped; M2S_LABEL_NONE is
 *   the way to leave cells out, so n_groups is at most 2^32 - 1.  Nothing validates labels.  The VALUES of skipped places still serve
 *   as corners of their neighbours' cells.
 *
 * THE DEFINITION (tests/band_measure_model.py restates it in numpy; the device equals it in every bit of every integer field).
 *   The cells, cases, triangles and their order are m2s_band_isosurface's: the cells whose 8 corners are all active, the case from
 *   d < iso, the table of isosurface_table.h.  A vertex on the edge from corner point p along axis a has the mesh vertex's
 *   t = (iso - d0) / (d1 - d0) in float32.  Its local coordinate u in its cell is the edge's corner offset (0 or 1 per axis) with
 *   u[a] = t; its index coordinate is U = (double)(i, j, k) + (double)u, (i, j, k) the cell's base corner.  No operation is fused;
 *   float64 is only added, subtracted, multiplied and rounded to the nearest even integer (llrint), which numpy reproduces.  Per triangle
 *   (U0, U1, U2) of a group:
 *   Area, in world scale (cell sizes may differ per axis): in float32, q = u * cell_size per axis, A2 = |(q1 - q0) x (q2 - q0)| as
 *     m2s_sample_surface's triangle weight (the squares summed left to right, sqrt; a non-finite A2 counts as 0); E =
 *     floor(log2(cmax * cmax)) with cmax the largest cell size and the product in float32 (info_out->area_exponent);
 *     w = (uint64) floor((double)A2 * 2^(24 - E)).  area_q = the sum of w; area = ldexp((double)area_q, E - 25).  A2 < 2^(E + 3), so
 *     w < 2^27; 5 triangles per cell and fewer than 2^32 cells keep the sum below 2^62.
 *   Volume, in index space (it is affine-covariant; the cell sizes come in once at the end): in float64, a = U1 - U0, b = U2 - U0,
 *     nz = a.x * b.y - a.y * b.x, sz = (U0.z + U1.z) + U2.z.  volume_q = the sum of llrint((nz * sz) * 2^20): six times the enclosed
 *     index volume (the divergence theorem along z) at a scale of 2^-20.  volume = volume_q * 2^-20 / 6 * cs_x * cs_y * cs_z.  The mesh
 *     is wound outwards: a solid's volume is positive, a cavity's negative.
 *   First moments: n = a x b; per axis c, s = ((x0*x0 + x1*x1) + x2*x2) + ((x0*x1 + x1*x2) + x2*x0) over the three U[c].  moment_q[c] =
 *     the sum of llrint((n[c] * s) * 2^8): 24 times the first moment at a scale of 2^-8.  centroid[c] = first_cell[c] + (moment_q[c] *
 *     2^-8 / 24) / (volume_q * 2^-20 / 6) * cell_size[c], NaN where volume_q == 0 (an empty band's, too).
 *   A float64 term that is not finite (values so large that d1 - d0 overflows) counts as 0.
 *   The sums are 64-bit integer adds: every order of execution gives the same bits, and two's-complement wrap-around of partial sums
 *   is harmless as long as the true sum fits.  For a closed surface 6 V * 2^20 < 2^59 (a grid has fewer than 2^36 cells) and
 *   24 M * 2^8 < 2^63 whenever total_cells * max(cell_count) < 2^50, THE MOMENT LIMIT: larger grids are refused.  2048^3 is 2^44.
 *   Counts: n_triangles as above.  n_vertices = the crossing edges with both ends active, counted at the point that owns the edge (its
 *     lower end).  n_open = the cells cut inside the band but incomplete, m2s_band_isosurface's n_open.  n_border = the counted
 *     vertices whose edge lies in a boundary face of the grid: for an axis other than the edge's own, the owner's index is 0 or
 *     cell_count - 1.
 *   CLOSED: the surface of a group is closed exactly when n_open == 0 && n_border == 0.  Only then are volume and centroid a volume
 *   and a centre of mass; otherwise they are still the sums defined above and depend on the grid's origin.  For a closed group
 *   n_vertices - n_triangles / 2 is its Euler characteristic.  Label with connectivity 26 to have it per mesh component: the 8 corners
 *   of a cell are mutually 26-adjacent, so a mesh component never straddles two labels.
 *   The raw sums do not depend on first_cell, and on cell_size only through the area.
 * measures_out is HOST memory whatever mem_kind says (as area_out of m2s_sample_surface).  Always synchronous.  An empty band gives
 *   zeros (and NaN centroids) and M2S_OK.  M2S_ERR_BAD_ARG before any device work: a NULL band or measures_out; a struct_size other than
 *   sizeof (mopts, info_out); a non-finite iso; labels with n_groups == 0 or n_groups >= 2^32; an m2s_opts.device that is not the
 *   handle's (-1 means its own); algorithm, x_begin, x_end, x_period or peer_out not zero; a bad mem_kind; a grid past the moment limit.
 *   m2s_opts: device, stream / stream_mode, lane; mem_kind covers labels.  timings (the argument; m2s_opts.timings serves when it is
 *   NULL): distance_ms = total_ms = the one kernel and the clearing of its records, n_units = the band's cells.
 *   Memory during the call: 72 bytes per group, and a host caller's labels. */
typedef struct m2s_band_measure_opts { uint32_t struct_size; float iso; } m2s_band_measure_opts;          /* NULL = iso 0 */
typedef struct m2s_band_measure_record {
  uint64_t n_triangles, n_vertices, n_open, n_border;   /* integers, as counted above */
  uint64_t area_q;  int64_t volume_q;  int64_t moment_q[3];   /* the raw sums the definition fixes to the bit */
  double area, volume, centroid[3];                     /* world units, derived on the host from the raw sums */
} m2s_band_measure_record;   /* 112 bytes; a typedef cannot share the call's name */
typedef struct m2s_band_measure_info { uint32_t struct_size; int32_t area_exponent; uint64_t n_groups, n_skipped; } m2s_band_measure_info;   /* 24 bytes */
int m2s_band_measure(const m2s_band* band, const m2s_band_measure_opts* mopts, const uint32_t* labels /* n_cells, list order; NULL = one group */,
                     uint64_t n_groups, const m2s_opts* opts, m2s_band_measure_record* measures_out /* HOST, n_groups entries (1 if labels is NULL) */,
                     m2s_band_measure_info* info_out /* may be NULL */, m2s_timings* timings /* may be NULL */);

/* ---- Band fields from spheres and capsules: points, particles, struts ----------------------------------------------------------------------
 * m2s_band_from_capsules makes a resident band field of a union of capsules without a mesh: what ParticlesToLevelSet,
 * createLevelSetSphere and createLevelSetCapsule are in OpenVDB.  A capsule is a segment a-b with a radius r; a sphere is the capsule
 * with a == b (b == NULL makes every shape one).  A particle set becomes a surface (this, a filter, m2s_band_isosurface), a graph of
 * edges a strut lattice, `field - capsule` (m2s_band_csg) a drilled hole.  Nothing is sized 4 bytes per grid point: the result's three
 * bit planes, its values, and 72 bytes per shape of workspace.
 *
 * THE DEFINITION (mesh_to_sdf_amd/csrc/shape.hip.h states it with its error bound; tests/band_shapes_model.py restates it in numpy; the
 * device equals it in every bit).  A shape is SOUND when its coordinates are finite and its radius is finite and >= 0; the others are
 * counted in n_skipped and take no part.  For a grid point with centre c = first_cell + (float)index * cell_size per axis and a sound
 * shape s, in binary32 with no operation fused and sums left to right:
 *     ab = b - a;  ap = c - a;  den = (ab.x*ab.x + ab.y*ab.y) + ab.z*ab.z
 *     t  = den > 0 ? clamp(((ap.x*ab.x + ap.y*ab.y) + ap.z*ab.z) / den, 0, 1) : 0
 *     e  = ap - t*ab                    (per component: one product, one subtraction)
 *     d_s = sqrtf((e.x*e.x + e.y*e.y) + e.z*e.z) - r
 *   D(c) = the minimum of d_s over the sound shapes (+inf when there is none; a d_s that is NaN takes no part).  A point is ACTIVE iff
 *   -interior <= D <= exterior, and its value is D.  The sign bit is D < 0 at EVERY grid point, active or not.  So a point buried deeper
 *   than `interior` in one shape is inactive even where another shape's surface passes through it, and a small ball inside a large one
 *   adds no cells.  A minimum is the same in any order: the result does not depend on the order of the shapes or of execution.
 *   Outside the union D is the Euclidean distance to it up to 96 * 2^-24 * the largest |coordinate| (shape.hip.h derives it); inside it
 *   is a lower bound of the depth, as after every level-set CSG: m2s_band_redistance makes distances of it again.
 * sopts: the half-widths (both >= 0 and finite) and the radius every shape takes when `radius` is NULL (>= 0 and finite).  fopts: the
 *   result's backgrounds; NULL = (exterior, interior), the widths.  a, b, radius: host or device memory as m2s_opts.mem_kind says.
 * info: n_cells = the result's cells; n_inside = the set bits of its sign mask; n_skipped = the shapes that are not sound;
 *   n_off_grid = the sound shapes with no grid point at d_s <= exterior.
 * The result is an ordinary handle with a sign mask (m2s_band_info's device_bytes by the formula for one; the values are an allocation
 *   of their own, sized by the count).  n == 0, or no shape that reaches the grid, gives an empty field and M2S_OK.
 * M2S_ERR_BAD_ARG before any device work: a NULL out, grid or sopts; a struct_size other than sizeof (sopts, fopts); a width or
 *   sopts->radius that is negative or not finite; a NULL `a` with n > 0; n >= 2^32; a cell_size that is not > 0 and finite, a grid box
 *   that is not finite, a cell_count of 0, or of 2^32 or more on one axis; a grid of 2^36 or more points; algorithm, x_begin, x_end,
 *   x_period or peer_out not zero; a bad mem_kind.  m2s_opts: device, stream / stream_mode, lane, mem_kind.  Always synchronous.
 *   timings (the argument; m2s_opts.timings serves when it is NULL): seed_ms = the shapes' boxes, the three bit planes, the mask and
 *   its offsets; distance_ms = the values; total_ms = the whole call; n_units = the result's cells; n_triangles = the sound shapes. */
typedef struct m2s_band_shapes_opts {
  uint32_t struct_size;
  float exterior, interior;   /* half-widths: active iff -interior <= D <= exterior; both >= 0 and finite */
  float radius;               /* used by every shape when `radius` (the array) is NULL; >= 0 and finite */
} m2s_band_shapes_opts;
typedef struct m2s_band_shapes_info {
  uint64_t n_cells;      /* active cells of the result */
  uint64_t n_inside;     /* grid points with D < 0 (set bits of the sign mask) */
  uint64_t n_skipped;    /* shapes with a non-finite coordinate or a radius that is negative or non-finite */
  uint64_t n_off_grid;   /* sound shapes that reach no grid point within `exterior` */
} m2s_band_shapes_info;
int m2s_band_from_capsules(const m2s_grid* grid, const float* a /* n x 3 */, const float* b /* n x 3, or NULL: spheres, b = a */,
                           const float* radius /* n, or NULL: sopts->radius for all */, uint64_t n /* < 2^32; 0 gives an empty field */,
                           const m2s_band_shapes_opts* sopts, const m2s_band_field_opts* fopts /* NULL = the widths */,
                           const m2s_opts* opts, m2s_band** out, m2s_band_shapes_info* info /* may be NULL */,
                           m2s_timings* timings /* may be NULL */);

/* glTF 2.0 / GLB ingestion (host side) — what the reference client extracts from a file before the merge:
 * mesh_to_sdf_client/src/gltf/mod.rs:56-174 (models keyed by mesh index, one primitive per mesh survives;
 * POSITION + indices, sparse accessors and byteStride honoured; missing indices = 0..n, pbr/model.rs:29-32),
 * gltf/scene/mod.rs:56-160 (node tree, simplify_tree) and gltf/mod.rs:91-106 (flatten_hierarchy: children
 * first, world = parent * local in glam's f32 arithmetic).  Instances come out in that order, over all scenes.
 * Errors: M2S_ERR_IO (cannot read), M2S_ERR_BAD_ARG (invalid file, or a required extension other than
 * KHR_lights_punctual — the reference's gltf build rejects those, gltf/mod.rs:407-410). */
typedef struct m2s_gltf m2s_gltf;
typedef struct m2s_gltf_info {
  uint64_t n_scenes, n_models, n_instances;
  uint64_t n_vertices, n_indices;   /* summed over the instances = sizes of the merged buffers */
} m2s_gltf_info;
int m2s_gltf_open(const char* path, m2s_gltf** out, m2s_gltf_info* info);
/* Fills `capacity` >= n_instances entries with HOST pointers into the handle (valid until m2s_gltf_close);
 * pass them to m2s_merge_instances with opts->mem_kind == M2S_MEM_HOST. */
int m2s_gltf_instances(const m2s_gltf* gltf, m2s_instance* out, size_t capacity);
void m2s_gltf_close(m2s_gltf* gltf);

/* Library / device introspection. */
/* The one-off costs of a process's first call, paid now instead: the HIP runtime and this library's code objects on `device`
 * (-1 = the current one), the streams and events of the device's context, `workspace_bytes` of device workspace (0 = none: it
 * grows on demand; a 512^3 grid call needs ~0.4 GB, 10 M queries ~1.5 GB) and, for callers of the host-pointer entry points, the
 * pinned staging ring (`host_ring_bytes` > 0: three slots of min(host_ring_bytes, 64 MB)).  Optional, idempotent (a repeated call
 * touches only what has grown since), blocking.  The workspace it grows is the one of the library's OWN stream: a caller that passes
 * m2s_opts.stream (or stream_mode 1) works out of a block per stream, which still grows, and is first touched, in that caller's first call.
 * The reference's usage is one call per process (examples/demo.rs:29-54): without this the first call pays 20-40 ms (grid,
 * host result) to ~0.9 s (10 M queries through host pointers) on top of its steady-state time — INTEGRATION.md has the breakdown;
 * M2S_HOST_TIMES=1 prints it per call on stderr. */
int m2s_warmup(int device, size_t workspace_bytes, size_t host_ring_bytes);
int m2s_version(void);               /* major*1000 + minor */
int m2s_device_count(void);          /* HIP devices visible; 0 if none (every compute call then fails with M2S_ERR_HIP) */
const char* m2s_last_error(void);    /* thread-local message of the last failing call on this thread */
/* Drops the cached per-device workspace (device memory is otherwise kept between calls). */
void m2s_release_workspace(void);
/* Run-time knobs (mesh_to_sdf_amd/csrc/tuning.h lists them; DESIGN.md §9 says what each default rests on).  They are read from the
 * environment variables of the same names ONCE, at the library's first use; m2s_tuning_set changes one afterwards (value NULL or "" =
 * back to the default) and returns M2S_ERR_BAD_ARG for an unknown name or an unparsable value.  None of them changes a result — they
 * choose between code paths that produce the same bits, which is what the tests use them for.  Not synchronised with calls in flight
 * on other threads.  m2s_tuning_describe writes "NAME=value" lines (NUL-terminated, truncated to `capacity`) and returns the length
 * the full text needs. */
int m2s_tuning_set(const char* name, const char* value);
int m2s_tuning_describe(char* buffer, int capacity);

#ifdef __cplusplus
}
#endif
#endif /* M2S_H */
