// capi_features.hip — the C ABI of include/m2s.h, the query features: closest points, winding numbers, ray casting, surface sampling,
// voxelization and narrow bands, each as a one-shot call (the caller's mesh, built for the call) and as a resident call (an m2s_mesh,
// capi_mesh.h).  No kernel lives here: per family an *Args struct, its argument checks, the run_* that enqueues the passes on a built
// mesh and the finish_* that ends a synchronous call; then the sixteen entry points, each a top-to-bottom sequence of the shared call
// steps below.  Contexts, staging, finish_call and the distance entry points are in capi.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "capi_mesh.h"
#include "tuning.h"

namespace {

using namespace m2s;

// ---- the steps every feature call shares ---------------------------------------------------------------------------------------------
// A one-shot call's mesh as the caller passed it; n_tris is what m2s_triangle_count makes of it, `dev` where the build reads it from.
struct MeshInput {
  const float* vertices;
  size_t n_vertices;
  const void* indices;
  size_t n_indices;
  int index_bytes, topology;
  size_t n_tris;
  StagedMesh dev;
};

// The mesh arguments of a one-shot call into `in`, checked.
int mesh_input(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes, int topology, MeshInput* in) {
  *in = MeshInput{vertices, n_vertices, indices, n_indices, index_bytes, topology, m2s_triangle_count(n_vertices, n_indices, indices != nullptr, topology), {}};
  return check_mesh_args(vertices, n_vertices, indices, n_indices, index_bytes, topology);
}

// Host-memory indices are range-checked before the device is touched (device-memory calls: by the build, as in every call).
int check_host_indices(const m2s_opts* opts, const MeshInput& in) {
  if ((opts && opts->mem_kind != M2S_MEM_HOST) || !in.indices || in.n_tris == 0) return 0;
  const size_t used = in.topology == M2S_TRIANGLE_LIST ? 3 * in.n_tris : in.n_indices;   // a trailing partial triple is never read
  for (size_t i = 0; i < used; ++i) {
    const uint64_t v = in.index_bytes == 2 ? static_cast<const uint16_t*>(in.indices)[i] : static_cast<const uint32_t*>(in.indices)[i];
    if (v >= in.n_vertices)
      return fail(M2S_ERR_BAD_ARG, "vertex index %llu out of range (%zu vertices; the reference panics indexing `vertices`)", (unsigned long long)v, in.n_vertices);
  }
  return 0;
}

int check_queries(const float* queries, size_t n_queries) {
  if (n_queries && !queries) return fail(M2S_ERR_BAD_ARG, "queries is NULL");
  if (n_queries >= 0xffffffc0ull) return fail(M2S_ERR_BAD_ARG, "too many queries for one call");
  return 0;
}

// Workspace a host-memory call needs to stage its mesh (with the 1024 bytes of slack every host-memory call adds once) ...
size_t mesh_staging_bytes(const CallCtx& c, const MeshInput& in) {
  return c.mem_kind != M2S_MEM_HOST ? 0 : align_up(in.n_vertices * 12) + align_up(in.n_indices * (size_t)(in.indices ? in.index_bytes : 0)) + 1024;
}
// ... and its n x 3 floats of queries.
size_t query_staging_bytes(const CallCtx& c, size_t n) { return c.mem_kind == M2S_MEM_HOST ? align_up(n * 12) : 0; }

// A call's workspace block and the device error word the call reports through.
struct Workspace : Arena {
  int* d_err = nullptr;
};

// Opens the call's workspace: a block of at least `need` bytes with the call's 16-int error word at its start, cleared.  A call on a
// mesh that may be asynchronous passes the mesh: such a call reports through the mesh's error word instead, which
// m2s_mesh_drain_timings reads and clears, and first folds the mesh's finished earlier calls into its sums.
int open_workspace(const CallCtx& c, DeviceState& st, size_t need, m2s_mesh* async_mesh, Workspace* ws) {
  if (const int rc = ensure_capacity(st, need)) return rc;
  static_cast<Arena&>(*ws) = Arena{st.base, st.cap, 0};
  ws->d_err = ws->take<int>(16);
  if (c.sync || !async_mesh) {
    M2S_HIP_CHECK(hipMemsetAsync(ws->d_err, 0, 64, c.stream));
  } else {
    ws->d_err = async_mesh->d_err_async;
    reap_pending(async_mesh, false);
  }
  return 0;
}

int stage_mesh_input(Arena& ws, const CallCtx& c, MeshInput* in) {
  return stage_mesh(ws, c, in->vertices, in->n_vertices, in->indices, in->n_indices, in->index_bytes, &in->dev);
}

// n x 3 floats of queries where the kernels can read them: the caller's array (device memory) or a copy in the workspace.
int stage_queries(Arena& ws, const CallCtx& c, DeviceState& st, const float* queries, size_t n, const float** d_q) {
  *d_q = queries;
  if (c.mem_kind != M2S_MEM_HOST) return 0;
  float* dq = ws.take<float>(n * 3);
  if (!dq) return fail(M2S_ERR_HIP, "internal: workspace");
  if (const int rc = staged_h2d(st, c.stream, reinterpret_cast<char*>(dq), reinterpret_cast<const char*>(queries), n * 12)) return rc;
  *d_q = dq;
  return 0;
}

// The tree of a one-shot call's staged mesh with leaves of leaf_max (records_only: the triangle records and nothing else).
int build_mesh(Workspace& ws, const CallCtx& c, const MeshInput& in, DeviceMesh* mesh, bool records_only, uint32_t leaf_max,
               uint64_t job_cells = ~0ull) {
  return build_device_mesh(ws, c.stream, in.dev.d_verts, in.n_vertices, in.dev.d_indices, in.n_indices, in.index_bytes, in.topology, in.n_tris,
                           ws.d_err, mesh, nullptr, records_only, leaf_max, job_cells);
}

// Records ev[first] .. ev[last] at one point of the call's stream: spans of finish_call that are empty for this call.
int record_events(DeviceState& st, hipStream_t stream, int first, int last) {
  for (int k = first; k <= last; ++k) M2S_HIP_CHECK(hipEventRecord(st.ev[k], stream));
  return 0;
}

// finish_call for every family but the closest points: with the seed span ev[2] .. ev[4], and `launches` dominant launches.
int finish_feature(const CallCtx& c, DeviceState& st, int* d_err, size_t n_tris, uint64_t units, uint32_t launches) {
  const int rc = finish_call(c, st, d_err, c.timings, n_tris, units, false, true);
  if (rc == M2S_OK && c.sync && c.timings) c.timings->distance_launches = launches;
  return rc;
}

// Ends a call on a mesh: an asynchronous one parks its event pair ev[4] .. ev[3] with the mesh, a synchronous one finishes as above.
int end_mesh_call(m2s_mesh* m, const CallCtx& c, DeviceState& st, int* d_err, uint64_t units, uint32_t launches) {
  if (!c.sync) return park_async_events(m, st, units, launches);
  return finish_feature(c, st, d_err, m->n_tris, units, launches);
}

// ---- closest points (m2s_closest_points and its three siblings) ---------------------------------------------------------------
// Two passes on the call's stream: the unsigned distance walk of the matching m2s_generate_* call, unchanged, into a workspace buffer,
// then k_closest (closest.hip), which finds the triangle that attains each distance.  ev[0] .. ev[1] is the build (one-shot calls),
// ev[2] .. ev[3] both passes, so finish_call reports them as accel_build_ms and distance_ms.
struct ClosestArgs {
  uint32_t* tri;
  float* point;
  float* dist;
};

int check_closest_outputs(const ClosestArgs& o) {
  if (!o.tri && !o.point && !o.dist) return fail(M2S_ERR_BAD_ARG, "triangle_out, point_out and distance_out are all NULL");
  return 0;
}

// Grid parameters of a closest-point call: an x-slab as for m2s_generate_grid_sdf; x_period and peer_out are grid-distance features only.
int closest_grid_params(const m2s_grid* grid, const m2s_opts* opts, GridParams* g, size_t* slab_cells) {
  if (!grid) return fail(M2S_ERR_BAD_ARG, "grid is NULL");
  if (grid->cell_count[0] == 0 || grid->cell_count[1] == 0 || grid->cell_count[2] == 0) return fail(M2S_ERR_BAD_ARG, "grid without cells");
  if (opts && opts->struct_size >= sizeof(m2s_opts) && (opts->x_period != 0 || opts->n_peer_out != 0))
    return fail(M2S_ERR_BAD_ARG, "m2s_opts.x_period / peer_out do not apply to closest-point calls");
  return fill_grid_params(grid, opts, g, slab_cells);
}

// Device-side outputs of a call: the caller's arrays (device memory) or workspace slabs copied out afterwards (host memory).
int closest_outputs(Arena& ws, const CallCtx& c, const ClosestArgs& o, size_t n, uint64_t first, ClosestOut* d) {
  *d = ClosestOut{o.tri, o.point, o.dist, 0};
  if (c.mem_kind == M2S_MEM_DEVICE) return 0;
  d->tri = o.tri ? ws.take<uint32_t>(n) : nullptr;
  d->point = o.point ? ws.take<float>(3 * n) : nullptr;
  d->dist = o.dist ? ws.take<float>(n) : nullptr;
  d->off = first;
  if ((o.tri && !d->tri) || (o.point && !d->point) || (o.dist && !d->dist)) return fail(M2S_ERR_HIP, "internal: workspace");
  return 0;
}
int closest_copy_out(DeviceState& st, const CallCtx& c, const ClosestArgs& o, const ClosestOut& d, size_t n, uint64_t first) {
  if (c.mem_kind == M2S_MEM_DEVICE) return 0;
  int rc = 0;
  if (o.tri && (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.tri + first), reinterpret_cast<const char*>(d.tri), n * 4))) return rc;
  if (o.point && (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.point + 3 * first), reinterpret_cast<const char*>(d.point), n * 12))) return rc;
  if (o.dist && (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.dist + first), reinterpret_cast<const char*>(d.dist), n * 4))) return rc;
  return 0;
}
size_t closest_workspace_bytes(const CallCtx& c, size_t n) {
  return align_up(n * 4) + (c.mem_kind == M2S_MEM_HOST ? align_up(n * 4) + align_up(n * 12) + align_up(n * 4) : 0) + 1024;
}

// Both passes over the slab of g on a built mesh.
int run_grid_closest(Arena& ws, const CallCtx& c, DeviceState& st, const DeviceMesh& mesh, const GridParams& g, size_t slab_cells,
                     const ClosestArgs& o, int* d_err) {
  const uint64_t first = (uint64_t)g.xb * g.n[1] * g.n[2];
  float* d_dist = ws.take<float>(slab_cells);
  ClosestOut d;
  if (!d_dist) return fail(M2S_ERR_HIP, "internal: workspace");
  int rc = closest_outputs(ws, c, o, slab_cells, first, &d);
  if (rc) return rc;
  GridParams gd = g;
  gd.out_off = first;                                  // the first pass writes the slab into d_dist
  rc = launch_grid_distance(ws, c.stream, mesh, gd, MODE_UNSIGNED, nullptr, c.algorithm, d_dist, d_err, nullptr, nullptr, !c.sync);
  if (rc) return rc;
  M2S_HIP_CHECK(hipEventRecord(st.ev[4], c.stream));
  rc = launch_closest_grid(c.stream, mesh, g, d_dist, first, c.algorithm, d);
  if (rc) return rc;
  M2S_HIP_CHECK(hipEventRecord(st.ev[3], c.stream));
  return closest_copy_out(st, c, o, d, slab_cells, first);
}

// Both passes over a query set on a built mesh; d_q on the device.
int run_query_closest(Arena& ws, const CallCtx& c, DeviceState& st, const DeviceMesh& mesh, const float* d_q, size_t n_q,
                      const ClosestArgs& o, int* d_err) {
  float* d_dist = ws.take<float>(n_q);
  ClosestOut d;
  if (!d_dist) return fail(M2S_ERR_HIP, "internal: workspace");
  int rc = closest_outputs(ws, c, o, n_q, 0, &d);
  if (rc) return rc;
  QueryPlan plan;   // the Morton order (perm) serves the second pass too; algorithm 1 has none (input order)
  rc = prepare_query_walk(ws, c.stream, d_q, n_q, mesh.n_tris, SIGN_NONE, c.algorithm, &plan);
  if (rc) return rc;
  if (query_is_tiny(n_q, mesh.n_tris, c.algorithm, SIGN_NONE))
    rc = launch_query_brute_split(ws, c.stream, mesh, d_q, n_q, MODE_UNSIGNED, SIGN_NONE, d_dist, d_err);
  else
    rc = launch_query_walk(ws, c.stream, mesh, d_q, plan, MODE_UNSIGNED, SIGN_NONE, c.algorithm, d_dist, d_err);
  if (rc) return rc;
  M2S_HIP_CHECK(hipEventRecord(st.ev[4], c.stream));
  rc = launch_closest_queries(c.stream, mesh, d_q, plan.perm, n_q, d_dist, c.algorithm, d);
  if (rc) return rc;
  M2S_HIP_CHECK(hipEventRecord(st.ev[3], c.stream));
  return closest_copy_out(st, c, o, d, n_q, 0);
}

// finish_call for a closest-point call: distance_ms = both passes (ev[2] .. ev[3]); seed_ms = the first pass alone (ev[2] .. ev[4]), the
// exact distances that seed k_closest.
int finish_closest(const CallCtx& c, DeviceState& st, int* d_err, size_t n_tris, size_t n_units) {
  const int rc = finish_call(c, st, d_err, c.timings, n_tris, n_units, false, false);
  if (rc == M2S_OK && c.sync && c.timings) {
    float first = 0.0f;
    (void)hipEventElapsedTime(&first, st.ev[2], st.ev[4]);
    c.timings->seed_ms = first;
    c.timings->distance_launches = 2;
  }
  return rc;
}

// ---- winding numbers (m2s_winding_numbers and its three siblings) --------------------------------------------------------------
// The moments of the tree's nodes (winding.hip k_moments; ev[2] .. ev[4] = seed_ms), then — only where signed distances are asked
// for — the unsigned distance walk of the closest-point calls, unchanged, into a workspace buffer, then the Barnes-Hut walk, which
// writes w and / or (w >= threshold ? -d : d).  ev[4] .. ev[3] = distance_ms.
struct WindingArgs {
  float* w;
  float* sdf;
  float beta, threshold;
};

int check_winding_args(const WindingArgs& o) {
  if (!o.w && !o.sdf) return fail(M2S_ERR_BAD_ARG, "winding_out and sdf_out are both NULL");
  if (!(o.beta >= 1.0f)) return fail(M2S_ERR_BAD_ARG, "beta must be >= 1 (or +inf: no expansion is ever used), got %g", (double)o.beta);
  return 0;
}

int winding_outputs(Arena& ws, const CallCtx& c, const WindingArgs& o, size_t n, uint64_t first, WindingOut* d) {
  *d = WindingOut{o.w, o.sdf, 0};
  if (c.mem_kind == M2S_MEM_DEVICE) return 0;
  d->w = o.w ? ws.take<float>(n) : nullptr;
  d->sdf = o.sdf ? ws.take<float>(n) : nullptr;
  d->off = first;
  if ((o.w && !d->w) || (o.sdf && !d->sdf)) return fail(M2S_ERR_HIP, "internal: workspace");
  return 0;
}
int winding_copy_out(DeviceState& st, const CallCtx& c, const WindingArgs& o, const WindingOut& d, size_t n, uint64_t first) {
  if (c.mem_kind == M2S_MEM_DEVICE) return 0;
  int rc = 0;
  if (o.w && (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.w + first), reinterpret_cast<const char*>(d.w), n * 4))) return rc;
  if (o.sdf && (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.sdf + first), reinterpret_cast<const char*>(d.sdf), n * 4))) return rc;
  return 0;
}
size_t winding_workspace_bytes(const CallCtx& c, size_t n) {
  return align_up(n * 4) + (c.mem_kind == M2S_MEM_HOST ? 2 * align_up(n * 4) : 0) + 1024;
}

// A mesh without triangles: w = 0 everywhere (entries [first, first + n) of winding_out); no distance exists.
int winding_of_nothing(const m2s_opts* opts, const WindingArgs& o, size_t first, size_t n) {
  if (o.sdf) return fail(M2S_ERR_EMPTY_MESH, "signed distances on a mesh without triangles");
  if (n == 0) return M2S_OK;
  if (!opts || opts->mem_kind == M2S_MEM_HOST) { memset(o.w + first, 0, n * 4); return M2S_OK; }
  CallCtx c;
  DeviceState* st = nullptr;
  if (const int rc = resolve_ctx(opts, &c, &st)) return rc;
  M2S_HIP_CHECK(hipMemsetAsync(o.w + first, 0, n * 4, c.stream));
  if (c.sync) M2S_HIP_CHECK(hipStreamSynchronize(c.stream));
  return M2S_OK;
}

// The moments of a one-shot call's tree, in its workspace; ev[4] closes the span.
int winding_moments(Arena& ws, const CallCtx& c, DeviceState& st, const DeviceMesh& mesh, const NodeMom** moms) {
  *moms = nullptr;
  if (c.algorithm != 1) {
    NodeMom* m = ws.take<NodeMom>(mesh.n_nodes);
    if (!m) return fail(M2S_ERR_HIP, "internal: workspace");
    if (const int rc = launch_winding_moments(c.stream, mesh, m)) return rc;
    *moms = m;
  }
  M2S_HIP_CHECK(hipEventRecord(st.ev[4], c.stream));
  return 0;
}

// The moments of a persistent mesh: made by its first winding call, kept in a block of their own until m2s_mesh_destroy.
int mesh_winding_moments(m2s_mesh* m, const CallCtx& c, DeviceState& st, const NodeMom** moms) {
  *moms = nullptr;
  if (c.algorithm != 1) {
    if (!m->mom_mem) {
      M2S_HIP_CHECK(hipMalloc((void**)&m->mom_mem, (size_t)m->dm.n_nodes * sizeof(NodeMom)));
      if (const int rc = launch_winding_moments(c.stream, m->dm, reinterpret_cast<NodeMom*>(m->mom_mem))) return rc;
      if (!m->mom_ready) M2S_HIP_CHECK(hipEventCreateWithFlags(&m->mom_ready, hipEventDisableTiming));
      M2S_HIP_CHECK(hipEventRecord(m->mom_ready, c.stream));
      m->mom_stream = c.stream;
    } else if (c.stream != m->mom_stream) {   // made (perhaps still being made) on another stream
      M2S_HIP_CHECK(hipStreamWaitEvent(c.stream, m->mom_ready, 0));
    }
    *moms = reinterpret_cast<const NodeMom*>(m->mom_mem);
  }
  M2S_HIP_CHECK(hipEventRecord(st.ev[4], c.stream));
  return 0;
}

int run_grid_winding(Arena& ws, const CallCtx& c, DeviceState& st, const DeviceMesh& mesh, const NodeMom* moms, const GridParams& g,
                     size_t slab_cells, const WindingArgs& o, int* d_err) {
  const uint64_t first = (uint64_t)g.xb * g.n[1] * g.n[2];
  float* d_dist = o.sdf ? ws.take<float>(slab_cells) : nullptr;
  WindingOut d;
  if (o.sdf && !d_dist) return fail(M2S_ERR_HIP, "internal: workspace");
  int rc = winding_outputs(ws, c, o, slab_cells, first, &d);
  if (rc) return rc;
  if (o.sdf) {
    GridParams gd = g;
    gd.out_off = first;                                  // the distance pass writes the slab into d_dist
    rc = launch_grid_distance(ws, c.stream, mesh, gd, MODE_UNSIGNED, nullptr, c.algorithm, d_dist, d_err, nullptr, nullptr, !c.sync);
    if (rc) return rc;
  }
  rc = launch_winding_grid(c.stream, mesh, moms, g, o.beta, o.threshold, d_dist, first, c.algorithm, d);
  if (rc) return rc;
  M2S_HIP_CHECK(hipEventRecord(st.ev[3], c.stream));
  return winding_copy_out(st, c, o, d, slab_cells, first);
}

int run_query_winding(Arena& ws, const CallCtx& c, DeviceState& st, const DeviceMesh& mesh, const NodeMom* moms, const float* d_q, size_t n_q,
                      const WindingArgs& o, int* d_err) {
  float* d_dist = o.sdf ? ws.take<float>(n_q) : nullptr;
  WindingOut d;
  if (o.sdf && !d_dist) return fail(M2S_ERR_HIP, "internal: workspace");
  int rc = winding_outputs(ws, c, o, n_q, 0, &d);
  if (rc) return rc;
  QueryPlan plan;   // the Morton order (perm) makes the packets coherent; algorithm 1 has none (input order)
  rc = prepare_query_walk(ws, c.stream, d_q, n_q, mesh.n_tris, SIGN_NONE, c.algorithm, &plan);
  if (rc) return rc;
  if (o.sdf) {
    if (query_is_tiny(n_q, mesh.n_tris, c.algorithm, SIGN_NONE))
      rc = launch_query_brute_split(ws, c.stream, mesh, d_q, n_q, MODE_UNSIGNED, SIGN_NONE, d_dist, d_err);
    else
      rc = launch_query_walk(ws, c.stream, mesh, d_q, plan, MODE_UNSIGNED, SIGN_NONE, c.algorithm, d_dist, d_err);
    if (rc) return rc;
  }
  rc = launch_winding_queries(c.stream, mesh, moms, d_q, plan.perm, n_q, o.beta, o.threshold, d_dist, c.algorithm, d);
  if (rc) return rc;
  M2S_HIP_CHECK(hipEventRecord(st.ev[3], c.stream));
  return winding_copy_out(st, c, o, d, n_q, 0);
}

// ---- ray casting (m2s_cast_rays, m2s_mesh_cast_rays) ---------------------------------------------------------------------------------
// One kernel on the call's stream (rays.hip), ev[4] .. ev[3] = distance_ms.
struct RayArgs {
  float* t;
  uint32_t* tri;
  float* uv;
  uint32_t* count;
  uint8_t* occluded;
  float t_min, t_max;
};

int check_ray_args(const m2s_ray_opts* ropts, const float* origins, const float* directions, size_t n_rays, const m2s_opts* opts, RayArgs* o) {
  if (ropts) {
    if (ropts->struct_size < sizeof(m2s_ray_opts)) return fail(M2S_ERR_BAD_ARG, "m2s_ray_opts.struct_size too small");
    o->t_min = ropts->t_min;
    o->t_max = ropts->t_max;
  }
  if (!(o->t_min <= o->t_max)) return fail(M2S_ERR_BAD_ARG, "ray range needs t_min <= t_max, neither NaN (got %g, %g)", (double)o->t_min, (double)o->t_max);
  // (without rays nothing is written, so callers whose empty arrays have no address pass)
  if (n_rays && !o->t && !o->tri && !o->uv && !o->count && !o->occluded) return fail(M2S_ERR_BAD_ARG, "every ray output is NULL");
  if (n_rays && (!origins || !directions)) return fail(M2S_ERR_BAD_ARG, "origins / directions is NULL");
  if (n_rays >= 0xffffffc0ull) return fail(M2S_ERR_BAD_ARG, "too many rays for one call");
  if (opts && (opts->x_begin != 0 || opts->x_end != 0)) return fail(M2S_ERR_BAD_ARG, "m2s_opts.x_begin / x_end do not apply to ray calls");
  if (opts && opts->struct_size >= sizeof(m2s_opts) && (opts->x_period != 0 || opts->n_peer_out != 0 || opts->peer_out != nullptr))
    return fail(M2S_ERR_BAD_ARG, "m2s_opts.x_period / peer_out do not apply to ray calls");
  if (opts && opts->mem_kind != M2S_MEM_HOST && opts->mem_kind != M2S_MEM_DEVICE) return fail(M2S_ERR_BAD_ARG, "bad mem_kind");
  if (opts && opts->algorithm != 0 && opts->algorithm != 1) return fail(M2S_ERR_BAD_ARG, "bad algorithm");
  return 0;
}

size_t ray_workspace_bytes(const CallCtx& c, size_t n) {
  return (c.mem_kind == M2S_MEM_HOST ? 2 * align_up(n * 12) + 3 * align_up(n * 4) + align_up(n * 8) + align_up(n) : 0) + 2048;
}

// Rays to the device (host memory), the kernel, results back.  `mesh` may be empty (n_tris == 0): every ray then reports no hit.
int run_cast_rays(Arena& ws, const CallCtx& c, DeviceState& st, const DeviceMesh& mesh, const float* origins, const float* directions, size_t n,
                  const RayArgs& o) {
  const float *d_org = origins, *d_dir = directions;
  RayOut d{o.t, o.tri, o.uv, o.count, o.occluded};
  int rc = 0;
  if (c.mem_kind == M2S_MEM_HOST) {
    float* org = ws.take<float>(3 * n);
    float* dir = ws.take<float>(3 * n);
    d.t = o.t ? ws.take<float>(n) : nullptr;
    d.tri = o.tri ? ws.take<uint32_t>(n) : nullptr;
    d.uv = o.uv ? ws.take<float>(2 * n) : nullptr;
    d.count = o.count ? ws.take<uint32_t>(n) : nullptr;
    d.occluded = o.occluded ? ws.take<uint8_t>(n) : nullptr;
    if (!org || !dir || (o.t && !d.t) || (o.tri && !d.tri) || (o.uv && !d.uv) || (o.count && !d.count) || (o.occluded && !d.occluded))
      return fail(M2S_ERR_HIP, "internal: workspace");
    if ((rc = staged_h2d(st, c.stream, reinterpret_cast<char*>(org), reinterpret_cast<const char*>(origins), n * 12))) return rc;
    if ((rc = staged_h2d(st, c.stream, reinterpret_cast<char*>(dir), reinterpret_cast<const char*>(directions), n * 12))) return rc;
    d_org = org;
    d_dir = dir;
  }
  M2S_HIP_CHECK(hipEventRecord(st.ev[4], c.stream));
  if ((rc = launch_cast_rays(c.stream, mesh, d_org, d_dir, n, o.t_min, o.t_max, c.algorithm, d))) return rc;
  M2S_HIP_CHECK(hipEventRecord(st.ev[3], c.stream));
  if (c.mem_kind == M2S_MEM_DEVICE) return 0;
  if (o.t && (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.t), reinterpret_cast<const char*>(d.t), n * 4))) return rc;
  if (o.tri && (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.tri), reinterpret_cast<const char*>(d.tri), n * 4))) return rc;
  if (o.uv && (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.uv), reinterpret_cast<const char*>(d.uv), n * 8))) return rc;
  if (o.count && (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.count), reinterpret_cast<const char*>(d.count), n * 4))) return rc;
  if (o.occluded && (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.occluded), reinterpret_cast<const char*>(d.occluded), n))) return rc;
  return 0;
}

// ---- surface sampling (m2s_sample_surface, m2s_mesh_sample_surface) -------------------------------------------------------------------
// The weight table (sample.hip; ev[2] .. ev[4] = seed_ms, its header's trip to the host included), then one kernel (ev[4] .. ev[3] =
// distance_ms).
struct SampleArgs {
  float* point;
  uint32_t* tri;
  float* uv;
  float* normal;
  double* area;
  uint64_t seed, first;
};

int check_sample_args(const m2s_surface_sample_opts* sopts, size_t n_samples, const m2s_opts* opts, SampleArgs* o) {
  if (!o->point && !o->tri && !o->uv && !o->normal && !o->area) return fail(M2S_ERR_BAD_ARG, "every sampling output is NULL, area_out included");
  if (sopts) {
    if (sopts->struct_size != sizeof(m2s_surface_sample_opts)) return fail(M2S_ERR_BAD_ARG, "m2s_surface_sample_opts.struct_size is not sizeof(m2s_surface_sample_opts)");
    if (sopts->reserved != 0) return fail(M2S_ERR_BAD_ARG, "m2s_surface_sample_opts.reserved must be 0");
    o->seed = sopts->seed;
    o->first = sopts->first_sample;
  }
  if (o->first > UINT64_MAX - (uint64_t)n_samples) return fail(M2S_ERR_BAD_ARG, "first_sample + n_samples overflows 64 bits");
  if (n_samples >= 0xffffffc0ull) return fail(M2S_ERR_BAD_ARG, "too many samples for one call");
  if (opts && (opts->x_begin != 0 || opts->x_end != 0)) return fail(M2S_ERR_BAD_ARG, "m2s_opts.x_begin / x_end do not apply to sampling calls");
  if (opts && opts->struct_size >= sizeof(m2s_opts) && (opts->x_period != 0 || opts->n_peer_out != 0 || opts->peer_out != nullptr))
    return fail(M2S_ERR_BAD_ARG, "m2s_opts.x_period / peer_out do not apply to sampling calls");
  if (opts && opts->mem_kind != M2S_MEM_HOST && opts->mem_kind != M2S_MEM_DEVICE) return fail(M2S_ERR_BAD_ARG, "bad mem_kind");
  if (opts && opts->algorithm != 0 && opts->algorithm != 1) return fail(M2S_ERR_BAD_ARG, "bad algorithm");
  return 0;
}

// No triangle the sampler can reach: the area is 0 and there is nothing to draw from.
int sample_of_nothing(const SampleArgs& o, size_t n_samples) {
  if (o.area) *o.area = 0.0;
  return n_samples ? fail(M2S_ERR_EMPTY_MESH, "surface samples of a mesh without area") : M2S_OK;
}

size_t sample_workspace_bytes(const CallCtx& c, size_t n) {
  return (c.mem_kind == M2S_MEM_HOST ? 2 * align_up(n * 12) + align_up(n * 4) + align_up(n * 8) : 0) + 2048;
}

// Makes the table of `src` and brings its header to the host (the stream is synchronised): Amax decides whether there is anything to
// sample, W feeds the pick and *area_out.  d_err (optional): the call's device error word, for a one-shot call's vertex indices.
int make_sample_table(const CallCtx& c, DeviceState& st, const SampleSrc& src, const SampleTable& tb, int* d_err, uint32_t* amax_bits, uint64_t* W) {
  int rc = launch_sample_table(c.stream, src, tb, d_err);
  if (rc) return rc;
  uint32_t* h = reinterpret_cast<uint32_t*>(st.h_err);   // 64 pinned bytes
  h[4] = 0;
  M2S_HIP_CHECK(hipMemcpyAsync(h, tb.hdr, 16, hipMemcpyDeviceToHost, c.stream));
  if (d_err) M2S_HIP_CHECK(hipMemcpyAsync(h + 4, d_err, sizeof(int), hipMemcpyDeviceToHost, c.stream));
  M2S_HIP_CHECK(hipStreamSynchronize(c.stream));
  if (h[4] & ERRF_INDEX_OOB) return fail(M2S_ERR_BAD_ARG, "vertex index out of range (the reference panics indexing `vertices`)");
  *amax_bits = h[0];
  memcpy(W, h + 2, 8);
  return 0;
}

double sample_total_area(uint32_t amax_bits, uint64_t W) {
  float amax;
  memcpy(&amax, &amax_bits, 4);
  return ldexp((double)W, sample_exponent(amax) - 38);
}

// The sampling kernel over a finished table, results back (host memory).  Records ev[4] and ev[3] also when there is nothing to launch.
int run_sample_surface(Arena& ws, const CallCtx& c, DeviceState& st, const SampleSrc& src, const SampleTable& tb, uint64_t W, size_t n,
                       const SampleArgs& o) {
  SampleOut d{o.point, o.tri, o.uv, o.normal};
  int rc = 0;
  if (c.mem_kind == M2S_MEM_HOST && n) {
    d.point = o.point ? ws.take<float>(3 * n) : nullptr;
    d.tri = o.tri ? ws.take<uint32_t>(n) : nullptr;
    d.uv = o.uv ? ws.take<float>(2 * n) : nullptr;
    d.normal = o.normal ? ws.take<float>(3 * n) : nullptr;
    if ((o.point && !d.point) || (o.tri && !d.tri) || (o.uv && !d.uv) || (o.normal && !d.normal)) return fail(M2S_ERR_HIP, "internal: workspace");
  }
  M2S_HIP_CHECK(hipEventRecord(st.ev[4], c.stream));
  if ((rc = launch_sample_surface(c.stream, src, tb, W, o.seed, o.first, n, c.algorithm, d))) return rc;
  M2S_HIP_CHECK(hipEventRecord(st.ev[3], c.stream));
  if (c.mem_kind == M2S_MEM_DEVICE || n == 0) return 0;
  if (o.point && (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.point), reinterpret_cast<const char*>(d.point), n * 12))) return rc;
  if (o.tri && (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.tri), reinterpret_cast<const char*>(d.tri), n * 4))) return rc;
  if (o.uv && (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.uv), reinterpret_cast<const char*>(d.uv), n * 8))) return rc;
  if (o.normal && (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.normal), reinterpret_cast<const char*>(d.normal), n * 12))) return rc;
  return 0;
}

// ---- voxelization (m2s_voxelize, m2s_mesh_voxelize) ------------------------------------------------------------------------------------
// ev[0] .. ev[1] the triangle records (one-shot), ev[2] .. ev[4] the sign planes (SOLID; seed_ms), ev[4] .. ev[3] the voxelization
// kernels (distance_ms).  The mask is made in the caller's bits_out (device memory) or in the workspace; everything else derives from it.
struct VoxelArgs {
  uint32_t* bits;
  uint8_t* occ;
  uint64_t* cells;
  uint64_t capacity;
  uint64_t* n_set;
  uint32_t mode;
};

// What every whole-grid mask call (voxelization, narrow bands) asks of its grid and of m2s_opts: no slabs, no peers, a grid the mask layout and
// the sign planes can address.
int check_whole_grid_args(const char* what, const m2s_grid* grid, const m2s_opts* opts, GridParams* g, size_t* cells) {
  if (!grid) return fail(M2S_ERR_BAD_ARG, "grid is NULL");
  if (opts && (opts->x_begin != 0 || opts->x_end != 0)) return fail(M2S_ERR_BAD_ARG, "m2s_opts.x_begin / x_end do not apply to %s calls", what);
  if (opts && opts->struct_size >= sizeof(m2s_opts) && (opts->x_period != 0 || opts->n_peer_out != 0 || opts->peer_out != nullptr))
    return fail(M2S_ERR_BAD_ARG, "m2s_opts.x_period / peer_out do not apply to %s calls", what);
  if (opts && opts->mem_kind != M2S_MEM_HOST && opts->mem_kind != M2S_MEM_DEVICE) return fail(M2S_ERR_BAD_ARG, "bad mem_kind");
  if (opts && opts->algorithm != 0 && opts->algorithm != 1) return fail(M2S_ERR_BAD_ARG, "bad algorithm");
  for (int k = 0; k < 3; ++k) {
    if (grid->cell_count[k] == 0) return fail(M2S_ERR_BAD_ARG, "cell_count[%d] is 0", k);
    if (!(grid->cell_size[k] > 0.0f) || !std::isfinite(grid->cell_size[k])) return fail(M2S_ERR_BAD_ARG, "cell_size[%d] must be positive and finite", k);
    if (!std::isfinite(grid->first_cell[k])) return fail(M2S_ERR_BAD_ARG, "first_cell[%d] is not finite", k);
  }
  const int rc = fill_grid_params(grid, nullptr, g, cells);
  if (rc) return rc;
  if ((uint64_t)grid->cell_count[0] * grid->cell_count[1] * grid->cell_count[2] >= (1ull << 36)) return fail(M2S_ERR_BAD_ARG, "2^36 or more cells");
  return 0;
}

int check_voxel_args(const m2s_grid* grid, const m2s_voxelize_opts* vopts, const m2s_opts* opts, VoxelArgs* o, GridParams* g, size_t* cells) {
  if (!grid) return fail(M2S_ERR_BAD_ARG, "grid is NULL");
  if (!o->bits && !o->occ && !o->cells && !o->n_set) return fail(M2S_ERR_BAD_ARG, "bits_out, occupancy_out, cells_out and n_set_out are all NULL");
  if (vopts) {
    if (vopts->struct_size != sizeof(m2s_voxelize_opts)) return fail(M2S_ERR_BAD_ARG, "m2s_voxelize_opts.struct_size is not sizeof(m2s_voxelize_opts)");
    if (vopts->mode != M2S_VOXELIZE_SURFACE && vopts->mode != M2S_VOXELIZE_SOLID) return fail(M2S_ERR_BAD_ARG, "bad m2s_voxelize_opts.mode %u", vopts->mode);
    o->mode = vopts->mode;
  }
  return check_whole_grid_args("voxelization", grid, opts, g, cells);
}

size_t voxel_workspace_bytes(const CallCtx& c, const GridParams& g, size_t n_tris, size_t cells, const VoxelArgs& o) {
  const size_t words = (size_t)g.n[0] * g.n[1] * g.nzw;
  size_t b = voxel_scratch_bytes(g, n_tris) + align_up(words * 4) + 4096;
  if (o.mode == M2S_VOXELIZE_SOLID) b += sign_workspace_bytes(g, n_tris);
  if (c.mem_kind == M2S_MEM_HOST) b += (o.occ ? align_up(cells) : 0) + (o.cells ? align_up((size_t)std::min<uint64_t>(o.capacity, cells) * 8) : 0);
  return b;
}

// Everything after the triangle records exist.  Records ev[2], ev[4], ev[3]; *short_capacity: cell_capacity is below the count
// (bits_out and occupancy_out are complete, cells_out untouched).
int run_voxelize(Arena& ws, const CallCtx& c, DeviceState& st, const DeviceMesh& mesh, const GridParams& g, size_t cells, const VoxelArgs& o,
                 bool* short_capacity) {
  *short_capacity = false;
  const size_t words = (size_t)g.n[0] * g.n[1] * g.nzw;
  const bool host = c.mem_kind == M2S_MEM_HOST;
  VoxelScratch vs;
  if (voxel_scratch_carve(ws, g, mesh.n_tris, &vs)) return fail(M2S_ERR_HIP, "internal: workspace");
  uint32_t* d_bits = (!host && o.bits) ? o.bits : ws.take<uint32_t>(words);
  uint8_t* d_occ = (!host || !o.occ) ? o.occ : ws.take<uint8_t>(cells);
  if (!d_bits || (o.occ && !d_occ)) return fail(M2S_ERR_HIP, "internal: workspace");
  int rc = 0;
  M2S_HIP_CHECK(hipEventRecord(st.ev[2], c.stream));
  st.planes_done = nullptr;
  const uint32_t* plane = nullptr;
  if (o.mode == M2S_VOXELIZE_SOLID && (rc = build_grid_sign_plane(ws, c.stream, mesh, g, &plane, false))) return rc;
  M2S_HIP_CHECK(hipEventRecord(st.ev[4], c.stream));
  if ((rc = launch_voxelize_surface(c.stream, mesh.tris, mesh.n_tris, g, c.algorithm, vs, d_bits))) return rc;
  if (plane && mesh.n_tris && (rc = launch_voxel_or_plane(c.stream, g, plane, d_bits))) return rc;
  if (o.occ && (rc = launch_voxel_expand(c.stream, g, d_bits, d_occ))) return rc;
  uint64_t count = 0;
  if (o.cells || o.n_set) {
    if ((rc = launch_voxel_count(c.stream, g, d_bits, vs))) return rc;
    uint64_t* h = reinterpret_cast<uint64_t*>(st.h_err) + 1;   // 64 pinned bytes; the first word stays the call's error flags
    M2S_HIP_CHECK(hipMemcpyAsync(h, vs.hdr, 8, hipMemcpyDeviceToHost, c.stream));
    M2S_HIP_CHECK(hipStreamSynchronize(c.stream));
    count = *h;
    if (o.n_set) *o.n_set = count;
    *short_capacity = o.cells && o.capacity < count;
  }
  uint64_t* d_cells = o.cells;
  if (o.cells && !*short_capacity && count) {
    if (host && !(d_cells = ws.take<uint64_t>(count))) return fail(M2S_ERR_HIP, "internal: workspace");
    if ((rc = launch_voxel_cells(c.stream, g, d_bits, vs, count, d_cells))) return rc;
  }
  M2S_HIP_CHECK(hipEventRecord(st.ev[3], c.stream));
  if (!host) return 0;
  if (o.bits && (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.bits), reinterpret_cast<const char*>(d_bits), words * 4))) return rc;
  if (o.occ && (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.occ), reinterpret_cast<const char*>(d_occ), cells))) return rc;
  if (o.cells && !*short_capacity && count &&
      (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.cells), reinterpret_cast<const char*>(d_cells), count * 8)))
    return rc;
  return 0;
}

// What a voxelization call returns once finish_feature (one-shot) or end_mesh_call has ended it with `rc`.
int voxelize_result(const CallCtx& c, const VoxelArgs& o, int rc, bool short_capacity) {
  if (c.sync && c.timings && o.mode != M2S_VOXELIZE_SOLID) c.timings->seed_ms = 0.0f;
  if (rc) return rc;
  if (short_capacity) return fail(M2S_ERR_BAD_ARG, "cell_capacity %llu is below the number of set cells (*n_set_out)", (unsigned long long)o.capacity);
  return M2S_OK;
}

// ---- narrow bands (m2s_narrow_band_sdf, m2s_mesh_narrow_band_sdf) -------------------------------------------------------------------------
// ev[0] .. ev[1] the build (one-shot), ev[2] .. ev[4] the sign planes and the candidate pass (seed_ms), ev[4] .. ev[3] the query walks, filter
// and compaction of every chunk (distance_ms).  Active cells and distances are compacted into the workspace and copied out once the count is
// known to fit: counting first would walk every candidate twice, and writing straight into the caller's arrays would leave them half
// filled when the capacity turns out short.
struct BandArgs {
  uint64_t* cells;
  float* dist;
  uint64_t capacity;
  uint32_t* bits;
  uint64_t* n_active;
  float exterior, interior;
  int sign_method;
};

int check_band_args(const m2s_grid* grid, const m2s_band_opts* bopts, const m2s_opts* opts, BandArgs* o, GridParams* g, size_t* cells) {
  if (!grid) return fail(M2S_ERR_BAD_ARG, "grid is NULL");
  if (o->sign_method != M2S_SIGN_RAYCAST && o->sign_method != M2S_SIGN_NORMAL) return fail(M2S_ERR_BAD_ARG, "bad sign_method %d", o->sign_method);
  if (!bopts) return fail(M2S_ERR_BAD_ARG, "bopts is NULL");
  if (bopts->struct_size != sizeof(m2s_band_opts)) return fail(M2S_ERR_BAD_ARG, "m2s_band_opts.struct_size is not sizeof(m2s_band_opts)");
  if (!(bopts->exterior >= 0.0f) || !(bopts->interior >= 0.0f)) return fail(M2S_ERR_BAD_ARG, "m2s_band_opts.exterior / interior must be >= 0 (+inf allowed)");
  if (!o->cells && !o->dist && !o->bits && !o->n_active) return fail(M2S_ERR_BAD_ARG, "cells_out, distances_out, bits_out and n_active_out are all NULL");
  o->exterior = bopts->exterior;
  o->interior = bopts->interior;
  return check_whole_grid_args("narrow-band", grid, opts, g, cells);
}

size_t band_stage_entries(size_t cells, const BandArgs& o) { return (o.cells || o.dist) ? (size_t)std::min<uint64_t>(o.capacity, cells) : 0; }
size_t band_chunk_of(size_t cells) { return std::min<size_t>(tuning().band_chunk, cells); }

size_t band_workspace_bytes(const CallCtx& c, const GridParams& g, size_t n_tris, size_t cells, const BandArgs& o) {
  const size_t words = (size_t)g.n[0] * g.n[1] * g.nzw, stage = band_stage_entries(cells, o);
  size_t b = voxel_scratch_bytes(g, n_tris) + 2 * align_up(words * 4) + align_up(stage * 8) + align_up(stage * 4) + 8192;
  if (o.sign_method == M2S_SIGN_RAYCAST) b += sign_workspace_bytes(g, n_tris);
  if (c.algorithm == 1) b += grid_distance_workspace_bytes(g, n_tris) + align_up(cells * 4);
  else b += band_chunk_bytes(band_chunk_of(cells)) + query_workspace_bytes(band_chunk_of(cells));
  return b;
}

// Everything after the tree exists.  Records ev[2], ev[4], ev[3]; *n_cand: the candidates evaluated; *short_capacity: capacity is below the
// count (bits_out is complete, cells_out and distances_out untouched).
int run_narrow_band(Arena& ws, const CallCtx& c, DeviceState& st, const DeviceMesh& mesh, const GridParams& g, size_t cells, const BandArgs& o,
                    int* d_err, uint64_t* n_cand, bool* short_capacity) {
  *short_capacity = false;
  *n_cand = 0;
  const size_t words = (size_t)g.n[0] * g.n[1] * g.nzw, stage = band_stage_entries(cells, o);
  const bool host = c.mem_kind == M2S_MEM_HOST, raycast = o.sign_method == M2S_SIGN_RAYCAST;
  VoxelScratch vs;
  if (voxel_scratch_carve(ws, g, mesh.n_tris, &vs)) return fail(M2S_ERR_HIP, "internal: workspace");
  uint32_t* d_bits = (!host && o.bits) ? o.bits : ws.take<uint32_t>(words);
  uint64_t* s_cells = (o.cells && stage) ? ws.take<uint64_t>(stage) : nullptr;
  float* s_dist = (o.dist && stage) ? ws.take<float>(stage) : nullptr;
  uint64_t* running = ws.take<uint64_t>(4);
  if (!d_bits || !running || (o.cells && stage && !s_cells) || (o.dist && stage && !s_dist)) return fail(M2S_ERR_HIP, "internal: workspace");
  uint64_t* h = reinterpret_cast<uint64_t*>(st.h_err) + 1;   // 64 pinned bytes; the first word stays the call's error flags
  int rc = 0;
  M2S_HIP_CHECK(hipEventRecord(st.ev[2], c.stream));
  st.planes_done = nullptr;
  const uint32_t* plane = nullptr;
  if (raycast && mesh.n_tris && (rc = build_grid_sign_plane(ws, c.stream, mesh, g, &plane, false))) return rc;
  uint64_t count = 0;
  if (c.algorithm == 1) {
    // the definition: the dense call's walk (its default path) into the workspace, the filter over every cell, the cells from the mask
    float* dense = ws.take<float>(cells);
    if (!dense) return fail(M2S_ERR_HIP, "internal: workspace");
    M2S_HIP_CHECK(hipEventRecord(st.ev[4], c.stream));
    if ((rc = launch_grid_distance(ws, c.stream, mesh, g, raycast ? MODE_UNSIGNED : MODE_NORMAL_FOLD, plane, 0, dense, d_err, nullptr))) return rc;
    if ((rc = launch_band_dense_mask(c.stream, g, dense, o.interior, o.exterior, d_bits))) return rc;
    if ((rc = launch_voxel_count(c.stream, g, d_bits, vs))) return rc;
    M2S_HIP_CHECK(hipMemcpyAsync(h, vs.hdr, 8, hipMemcpyDeviceToHost, c.stream));
    M2S_HIP_CHECK(hipStreamSynchronize(c.stream));
    count = *h;
    *n_cand = cells;
    if (stage && count <= o.capacity && count) {
      uint64_t* cl = s_cells ? s_cells : ws.take<uint64_t>(count);
      if (!cl) return fail(M2S_ERR_HIP, "internal: workspace");
      if ((rc = launch_voxel_cells(c.stream, g, d_bits, vs, count, cl))) return rc;
      if (s_dist && (rc = launch_band_gather(c.stream, dense, cl, count, s_dist))) return rc;
    }
  } else {
    uint32_t* cand = ws.take<uint32_t>(words);
    BandChunk ch;
    const size_t chunk = band_chunk_of(cells);
    if (!cand || band_chunk_carve(ws, chunk, &ch)) return fail(M2S_ERR_HIP, "internal: workspace");
    if ((rc = launch_band_candidates(c.stream, mesh.tris, mesh.n_tris, g, std::max(o.exterior, o.interior), vs, cand))) return rc;
    if ((rc = launch_voxel_count(c.stream, g, cand, vs))) return rc;
    M2S_HIP_CHECK(hipMemsetAsync(d_bits, 0, words * 4, c.stream));
    M2S_HIP_CHECK(hipMemsetAsync(running, 0, 32, c.stream));
    M2S_HIP_CHECK(hipMemcpyAsync(h, vs.hdr, 8, hipMemcpyDeviceToHost, c.stream));
    M2S_HIP_CHECK(hipEventRecord(st.ev[4], c.stream));
    M2S_HIP_CHECK(hipStreamSynchronize(c.stream));
    const uint64_t total = *h;
    *n_cand = total;
    for (uint64_t begin = 0; begin < total; begin += chunk) {
      const uint32_t n = (uint32_t)std::min<uint64_t>(chunk, total - begin);
      if ((rc = launch_band_emit(c.stream, g, cand, vs, begin, begin + n, ch))) return rc;
      Arena qw = ws;   // the query walk's scratch: the same bytes for every chunk
      if ((rc = launch_query_distance(qw, c.stream, mesh, ch.centres, n, raycast ? MODE_UNSIGNED : MODE_NORMAL_FOLD, SIGN_NONE, 0, ch.dist, d_err))) return rc;
      if ((rc = launch_band_filter(c.stream, g, ch, n, plane, o.interior, o.exterior, d_bits, running, stage, s_cells, s_dist))) return rc;
    }
    M2S_HIP_CHECK(hipMemcpyAsync(h, running, 8, hipMemcpyDeviceToHost, c.stream));
    M2S_HIP_CHECK(hipStreamSynchronize(c.stream));
    count = *h;
  }
  if (o.n_active) *o.n_active = count;
  *short_capacity = (o.cells || o.dist) && o.capacity < count;
  const bool copy = (o.cells || o.dist) && !*short_capacity && count;
  if (copy && !host) {
    if (o.cells) M2S_HIP_CHECK(hipMemcpyAsync(o.cells, s_cells, count * 8, hipMemcpyDeviceToDevice, c.stream));
    if (o.dist) M2S_HIP_CHECK(hipMemcpyAsync(o.dist, s_dist, count * 4, hipMemcpyDeviceToDevice, c.stream));
  }
  M2S_HIP_CHECK(hipEventRecord(st.ev[3], c.stream));
  if (!host) return 0;
  if (o.bits && (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.bits), reinterpret_cast<const char*>(d_bits), words * 4))) return rc;
  if (copy && o.cells && (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.cells), reinterpret_cast<const char*>(s_cells), count * 8))) return rc;
  if (copy && o.dist && (rc = staged_d2h(st, c.stream, reinterpret_cast<char*>(o.dist), reinterpret_cast<const char*>(s_dist), count * 4))) return rc;
  return 0;
}

// What a narrow-band call returns once finish_feature (one-shot) or end_mesh_call has ended it with `rc`.
int narrow_band_result(const BandArgs& o, int rc, bool short_capacity) {
  if (rc) return rc;
  if (short_capacity) return fail(M2S_ERR_BAD_ARG, "capacity %llu is below the number of active cells (*n_active_out)", (unsigned long long)o.capacity);
  return M2S_OK;
}

}  // namespace

using namespace m2s;

extern "C" {

int m2s_closest_points(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes, int topology,
                       const float* queries, size_t n_queries, uint32_t* triangle_out, float* point_out, float* distance_out,
                       const m2s_opts* opts) {
  clear_error();
  const ClosestArgs o{triangle_out, point_out, distance_out};
  MeshInput in;
  int rc = mesh_input(vertices, n_vertices, indices, n_indices, index_bytes, topology, &in);
  if (rc) return rc;
  if ((rc = check_closest_outputs(o))) return rc;
  if ((rc = check_queries(queries, n_queries))) return rc;
  if (in.n_tris == 0) return fail(M2S_ERR_EMPTY_MESH, "closest points on a mesh without triangles");
  if ((rc = check_host_indices(opts, in))) return rc;
  if (n_queries == 0) return M2S_OK;
  CallCtx c;
  DeviceState* st = nullptr;
  if ((rc = resolve_ctx(opts, &c, &st))) return rc;
  const size_t need = bvh_workspace_bytes(in.n_tris) + query_workspace_bytes(n_queries) + align_up(n_queries * 16) +
                      closest_workspace_bytes(c, n_queries) + 4096 + mesh_staging_bytes(c, in) + query_staging_bytes(c, n_queries);
  Workspace ws;
  if ((rc = open_workspace(c, *st, need, nullptr, &ws))) return rc;
  if ((rc = stage_mesh_input(ws, c, &in))) return rc;
  const float* d_q = nullptr;
  if ((rc = stage_queries(ws, c, *st, queries, n_queries, &d_q))) return rc;
  M2S_HIP_CHECK(hipEventRecord(st->ev[0], c.stream));
  DeviceMesh mesh;
  if ((rc = build_mesh(ws, c, in, &mesh, false, query_leaf_max(n_queries, in.n_tris, SIGN_NONE)))) return rc;
  if ((rc = record_events(*st, c.stream, 1, 2))) return rc;
  if ((rc = run_query_closest(ws, c, *st, mesh, d_q, n_queries, o, ws.d_err))) return rc;
  return finish_closest(c, *st, ws.d_err, in.n_tris, n_queries);
}

int m2s_grid_closest_points(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes, int topology,
                            const m2s_grid* grid, uint32_t* triangle_out, float* point_out, float* distance_out, const m2s_opts* opts) {
  clear_error();
  const ClosestArgs o{triangle_out, point_out, distance_out};
  MeshInput in;
  int rc = mesh_input(vertices, n_vertices, indices, n_indices, index_bytes, topology, &in);
  if (rc) return rc;
  if ((rc = check_closest_outputs(o))) return rc;
  GridParams g;
  size_t slab_cells = 0;
  if ((rc = closest_grid_params(grid, opts, &g, &slab_cells))) return rc;
  if (in.n_tris == 0) return fail(M2S_ERR_EMPTY_MESH, "closest points on a mesh without triangles");
  if ((rc = check_host_indices(opts, in))) return rc;
  if (slab_cells == 0) return M2S_OK;   // an empty slab [x, x)
  CallCtx c;
  DeviceState* st = nullptr;
  if ((rc = resolve_ctx(opts, &c, &st))) return rc;
  const size_t need = bvh_workspace_bytes(in.n_tris) + grid_distance_workspace_bytes(g, in.n_tris) + closest_workspace_bytes(c, slab_cells) + 4096 +
                      mesh_staging_bytes(c, in);
  Workspace ws;
  if ((rc = open_workspace(c, *st, need, nullptr, &ws))) return rc;
  if ((rc = stage_mesh_input(ws, c, &in))) return rc;
  M2S_HIP_CHECK(hipEventRecord(st->ev[0], c.stream));
  DeviceMesh mesh;
  if ((rc = build_mesh(ws, c, in, &mesh, false, grid_leaf_max(g, in.n_tris), (uint64_t)slab_cells))) return rc;
  if ((rc = record_events(*st, c.stream, 1, 2))) return rc;
  st->planes_done = nullptr;
  st->have_raw_seeds = false;
  if ((rc = run_grid_closest(ws, c, *st, mesh, g, slab_cells, o, ws.d_err))) return rc;
  return finish_closest(c, *st, ws.d_err, in.n_tris, slab_cells);
}

// The resident closest-point calls have no asynchronous form: they always clear the workspace's error word and end in finish_closest,
// where their six sibling resident calls hand open_workspace the mesh and end in end_mesh_call.  (Looks like an omission; kept as it is.)
int m2s_mesh_closest_points(m2s_mesh* m, const float* queries, size_t n_queries, uint32_t* triangle_out, float* point_out,
                            float* distance_out, const m2s_opts* opts) {
  clear_error();
  if (!m) return fail(M2S_ERR_BAD_ARG, "mesh is NULL");
  std::lock_guard<std::mutex> mlk(m->mu);
  const ClosestArgs o{triangle_out, point_out, distance_out};
  int rc = check_closest_outputs(o);
  if (rc) return rc;
  if ((rc = check_queries(queries, n_queries))) return rc;
  if (m->n_tris == 0) return fail(M2S_ERR_EMPTY_MESH, "closest points on a mesh without triangles");
  if (n_queries == 0) return M2S_OK;
  m2s_opts mo;
  if ((rc = mesh_call_opts(m, opts, &mo))) return rc;   // (after the early returns here, before them in the winding calls; kept)
  CallCtx c;
  DeviceState* st = nullptr;
  if ((rc = resolve_ctx(&mo, &c, &st))) return rc;
  size_t need = query_workspace_bytes(n_queries) + align_up(n_queries * 16) + closest_workspace_bytes(c, n_queries) + 8192 +
                query_staging_bytes(c, n_queries);
  if (c.mem_kind == M2S_MEM_HOST) need += 1024;   // the slack that mesh_staging_bytes carries in a one-shot call
  Workspace ws;
  if ((rc = open_workspace(c, *st, need, nullptr, &ws))) return rc;
  const float* d_q = nullptr;
  if ((rc = stage_queries(ws, c, *st, queries, n_queries, &d_q))) return rc;
  if ((rc = record_events(*st, c.stream, 0, 2))) return rc;   // no build: its span is empty
  if ((rc = remark_leaves(m, c, m->dm.leaf_max))) return rc;   // the tree as it is (any leaf size serves); keeps the mesh's stream bookkeeping
  if ((rc = run_query_closest(ws, c, *st, m->dm, d_q, n_queries, o, ws.d_err))) return rc;
  return finish_closest(c, *st, ws.d_err, m->n_tris, n_queries);
}

int m2s_mesh_grid_closest_points(m2s_mesh* m, const m2s_grid* grid, uint32_t* triangle_out, float* point_out, float* distance_out,
                                 const m2s_opts* opts) {
  clear_error();
  if (!m) return fail(M2S_ERR_BAD_ARG, "mesh is NULL");
  std::lock_guard<std::mutex> mlk(m->mu);
  const ClosestArgs o{triangle_out, point_out, distance_out};
  int rc = check_closest_outputs(o);
  if (rc) return rc;
  GridParams g;
  size_t slab_cells = 0;
  if ((rc = closest_grid_params(grid, opts, &g, &slab_cells))) return rc;
  if (m->n_tris == 0) return fail(M2S_ERR_EMPTY_MESH, "closest points on a mesh without triangles");
  if (slab_cells == 0) return M2S_OK;
  m2s_opts mo;
  if ((rc = mesh_call_opts(m, opts, &mo))) return rc;
  CallCtx c;
  DeviceState* st = nullptr;
  if ((rc = resolve_ctx(&mo, &c, &st))) return rc;
  const size_t need = grid_distance_workspace_bytes(g, m->n_tris) + closest_workspace_bytes(c, slab_cells) + 8192;
  Workspace ws;
  if ((rc = open_workspace(c, *st, need, nullptr, &ws))) return rc;
  if ((rc = record_events(*st, c.stream, 0, 2))) return rc;   // no build: its span is empty
  st->planes_done = nullptr;
  st->have_raw_seeds = false;
  if ((rc = remark_leaves(m, c, m->dm.leaf_max))) return rc;
  if ((rc = run_grid_closest(ws, c, *st, m->dm, g, slab_cells, o, ws.d_err))) return rc;
  return finish_closest(c, *st, ws.d_err, m->n_tris, slab_cells);
}

int m2s_winding_numbers(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes, int topology,
                        const float* queries, size_t n_queries, float beta, float threshold, float* winding_out, float* sdf_out,
                        const m2s_opts* opts) {
  clear_error();
  const WindingArgs o{winding_out, sdf_out, beta, threshold};
  MeshInput in;
  int rc = mesh_input(vertices, n_vertices, indices, n_indices, index_bytes, topology, &in);
  if (rc) return rc;
  if ((rc = check_winding_args(o))) return rc;
  if ((rc = check_queries(queries, n_queries))) return rc;
  if (in.n_tris == 0) return winding_of_nothing(opts, o, 0, n_queries);
  if ((rc = check_host_indices(opts, in))) return rc;
  if (n_queries == 0) return M2S_OK;
  CallCtx c;
  DeviceState* st = nullptr;
  if ((rc = resolve_ctx(opts, &c, &st))) return rc;
  const size_t need = bvh_workspace_bytes(in.n_tris) + align_up(2 * in.n_tris * sizeof(NodeMom)) + query_workspace_bytes(n_queries) +
                      align_up(n_queries * 16) + winding_workspace_bytes(c, n_queries) + 4096 + mesh_staging_bytes(c, in) +
                      query_staging_bytes(c, n_queries);
  Workspace ws;
  if ((rc = open_workspace(c, *st, need, nullptr, &ws))) return rc;
  if ((rc = stage_mesh_input(ws, c, &in))) return rc;
  const float* d_q = nullptr;
  if ((rc = stage_queries(ws, c, *st, queries, n_queries, &d_q))) return rc;
  M2S_HIP_CHECK(hipEventRecord(st->ev[0], c.stream));
  DeviceMesh mesh;
  if ((rc = build_mesh(ws, c, in, &mesh, false, query_leaf_max(n_queries, in.n_tris, SIGN_NONE)))) return rc;
  if ((rc = record_events(*st, c.stream, 1, 2))) return rc;
  st->planes_done = nullptr;   // (the query forms of the winding calls reset this and the closest-point ones do not; kept)
  const NodeMom* moms = nullptr;
  if ((rc = winding_moments(ws, c, *st, mesh, &moms))) return rc;
  if ((rc = run_query_winding(ws, c, *st, mesh, moms, d_q, n_queries, o, ws.d_err))) return rc;
  return finish_feature(c, *st, ws.d_err, in.n_tris, n_queries, o.sdf ? 2 : 1);
}

int m2s_grid_winding_numbers(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes, int topology,
                             const m2s_grid* grid, float beta, float threshold, float* winding_out, float* sdf_out, const m2s_opts* opts) {
  clear_error();
  const WindingArgs o{winding_out, sdf_out, beta, threshold};
  MeshInput in;
  int rc = mesh_input(vertices, n_vertices, indices, n_indices, index_bytes, topology, &in);
  if (rc) return rc;
  if ((rc = check_winding_args(o))) return rc;
  GridParams g;
  size_t slab_cells = 0;
  if ((rc = closest_grid_params(grid, opts, &g, &slab_cells))) return rc;
  if (in.n_tris == 0) return winding_of_nothing(opts, o, (size_t)g.xb * g.n[1] * g.n[2], slab_cells);
  if ((rc = check_host_indices(opts, in))) return rc;
  if (slab_cells == 0) return M2S_OK;   // an empty slab [x, x)
  CallCtx c;
  DeviceState* st = nullptr;
  if ((rc = resolve_ctx(opts, &c, &st))) return rc;
  const size_t need = bvh_workspace_bytes(in.n_tris) + align_up(2 * in.n_tris * sizeof(NodeMom)) + grid_distance_workspace_bytes(g, in.n_tris) +
                      winding_workspace_bytes(c, slab_cells) + 4096 + mesh_staging_bytes(c, in);
  Workspace ws;
  if ((rc = open_workspace(c, *st, need, nullptr, &ws))) return rc;
  if ((rc = stage_mesh_input(ws, c, &in))) return rc;
  M2S_HIP_CHECK(hipEventRecord(st->ev[0], c.stream));
  DeviceMesh mesh;
  if ((rc = build_mesh(ws, c, in, &mesh, false, grid_leaf_max(g, in.n_tris), (uint64_t)slab_cells))) return rc;
  if ((rc = record_events(*st, c.stream, 1, 2))) return rc;
  st->planes_done = nullptr;
  st->have_raw_seeds = false;
  const NodeMom* moms = nullptr;
  if ((rc = winding_moments(ws, c, *st, mesh, &moms))) return rc;
  if ((rc = run_grid_winding(ws, c, *st, mesh, moms, g, slab_cells, o, ws.d_err))) return rc;
  return finish_feature(c, *st, ws.d_err, in.n_tris, slab_cells, o.sdf ? 2 : 1);
}

int m2s_mesh_winding_numbers(m2s_mesh* m, const float* queries, size_t n_queries, float beta, float threshold, float* winding_out,
                             float* sdf_out, const m2s_opts* opts) {
  clear_error();
  if (!m) return fail(M2S_ERR_BAD_ARG, "mesh is NULL");
  std::lock_guard<std::mutex> mlk(m->mu);
  const WindingArgs o{winding_out, sdf_out, beta, threshold};
  int rc = check_winding_args(o);
  if (rc) return rc;
  if ((rc = check_queries(queries, n_queries))) return rc;
  m2s_opts mo;
  if ((rc = mesh_call_opts(m, opts, &mo))) return rc;   // (before the early returns here, after them in the closest-point calls; kept)
  if (m->n_tris == 0) return winding_of_nothing(&mo, o, 0, n_queries);
  if (n_queries == 0) return M2S_OK;
  CallCtx c;
  DeviceState* st = nullptr;
  if ((rc = resolve_ctx(&mo, &c, &st))) return rc;
  size_t need = query_workspace_bytes(n_queries) + align_up(n_queries * 16) + winding_workspace_bytes(c, n_queries) + 8192 +
                query_staging_bytes(c, n_queries);
  if (c.mem_kind == M2S_MEM_HOST) need += 1024;   // the slack that mesh_staging_bytes carries in a one-shot call
  Workspace ws;
  if ((rc = open_workspace(c, *st, need, m, &ws))) return rc;
  const float* d_q = nullptr;
  if ((rc = stage_queries(ws, c, *st, queries, n_queries, &d_q))) return rc;
  if ((rc = record_events(*st, c.stream, 0, 2))) return rc;   // no build: its span is empty
  st->planes_done = nullptr;
  if ((rc = remark_leaves(m, c, m->dm.leaf_max))) return rc;   // the tree as it is: the walk reads no leaf marks; keeps the mesh's stream bookkeeping
  const NodeMom* moms = nullptr;
  if ((rc = mesh_winding_moments(m, c, *st, &moms))) return rc;
  if ((rc = run_query_winding(ws, c, *st, m->dm, moms, d_q, n_queries, o, ws.d_err))) return rc;
  return end_mesh_call(m, c, *st, ws.d_err, n_queries, o.sdf ? 2 : 1);
}

int m2s_mesh_grid_winding_numbers(m2s_mesh* m, const m2s_grid* grid, float beta, float threshold, float* winding_out, float* sdf_out,
                                  const m2s_opts* opts) {
  clear_error();
  if (!m) return fail(M2S_ERR_BAD_ARG, "mesh is NULL");
  std::lock_guard<std::mutex> mlk(m->mu);
  const WindingArgs o{winding_out, sdf_out, beta, threshold};
  int rc = check_winding_args(o);
  if (rc) return rc;
  GridParams g;
  size_t slab_cells = 0;
  if ((rc = closest_grid_params(grid, opts, &g, &slab_cells))) return rc;
  m2s_opts mo;
  if ((rc = mesh_call_opts(m, opts, &mo))) return rc;
  if (m->n_tris == 0) return winding_of_nothing(&mo, o, (size_t)g.xb * g.n[1] * g.n[2], slab_cells);
  if (slab_cells == 0) return M2S_OK;
  CallCtx c;
  DeviceState* st = nullptr;
  if ((rc = resolve_ctx(&mo, &c, &st))) return rc;
  const size_t need = grid_distance_workspace_bytes(g, m->n_tris) + winding_workspace_bytes(c, slab_cells) + 8192;
  Workspace ws;
  if ((rc = open_workspace(c, *st, need, m, &ws))) return rc;
  if ((rc = record_events(*st, c.stream, 0, 2))) return rc;   // no build: its span is empty
  st->planes_done = nullptr;
  st->have_raw_seeds = false;
  if ((rc = remark_leaves(m, c, m->dm.leaf_max))) return rc;
  const NodeMom* moms = nullptr;
  if ((rc = mesh_winding_moments(m, c, *st, &moms))) return rc;
  if ((rc = run_grid_winding(ws, c, *st, m->dm, moms, g, slab_cells, o, ws.d_err))) return rc;
  return end_mesh_call(m, c, *st, ws.d_err, slab_cells, o.sdf ? 2 : 1);
}

// Ray casting (include/m2s.h): the one-shot call builds the tree, the mesh call walks the resident one as it is marked.
int m2s_cast_rays(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes, int topology,
                  const float* origins, const float* directions, size_t n_rays, const m2s_ray_opts* ropts, float* t_out, uint32_t* triangle_out,
                  float* uv_out, uint32_t* count_out, uint8_t* occluded_out, const m2s_opts* opts) {
  clear_error();
  RayArgs o{t_out, triangle_out, uv_out, count_out, occluded_out, 0.0f, __builtin_inff()};
  MeshInput in;
  int rc = mesh_input(vertices, n_vertices, indices, n_indices, index_bytes, topology, &in);
  if (rc) return rc;
  if ((rc = check_ray_args(ropts, origins, directions, n_rays, opts, &o))) return rc;
  if ((rc = check_host_indices(opts, in))) return rc;
  if (n_rays == 0) return M2S_OK;
  CallCtx c;
  DeviceState* st = nullptr;
  if ((rc = resolve_ctx(opts, &c, &st))) return rc;
  const size_t need = (in.n_tris ? bvh_workspace_bytes(in.n_tris) : 0) + ray_workspace_bytes(c, n_rays) + 4096 + mesh_staging_bytes(c, in);
  Workspace ws;
  if ((rc = open_workspace(c, *st, need, nullptr, &ws))) return rc;
  M2S_HIP_CHECK(hipEventRecord(st->ev[0], c.stream));
  DeviceMesh mesh{};   // without triangles: no tree, and every ray reports no hit
  if (in.n_tris) {
    if ((rc = stage_mesh_input(ws, c, &in))) return rc;
    M2S_HIP_CHECK(hipEventRecord(st->ev[0], c.stream));   // (a second time, now behind the staging as in the other calls; kept)
    if ((rc = build_mesh(ws, c, in, &mesh, false, query_leaf_max(n_rays, in.n_tris, SIGN_NONE)))) return rc;
  }
  if ((rc = record_events(*st, c.stream, 1, 2))) return rc;
  st->planes_done = nullptr;
  if ((rc = run_cast_rays(ws, c, *st, mesh, origins, directions, n_rays, o))) return rc;
  return finish_feature(c, *st, ws.d_err, in.n_tris, n_rays, 1);
}

int m2s_mesh_cast_rays(m2s_mesh* m, const float* origins, const float* directions, size_t n_rays, const m2s_ray_opts* ropts, float* t_out,
                       uint32_t* triangle_out, float* uv_out, uint32_t* count_out, uint8_t* occluded_out, const m2s_opts* opts) {
  clear_error();
  if (!m) return fail(M2S_ERR_BAD_ARG, "mesh is NULL");
  std::lock_guard<std::mutex> mlk(m->mu);
  RayArgs o{t_out, triangle_out, uv_out, count_out, occluded_out, 0.0f, __builtin_inff()};
  int rc = check_ray_args(ropts, origins, directions, n_rays, opts, &o);
  if (rc) return rc;
  m2s_opts mo;
  if ((rc = mesh_call_opts(m, opts, &mo))) return rc;
  if (n_rays == 0) return M2S_OK;
  CallCtx c;
  DeviceState* st = nullptr;
  if ((rc = resolve_ctx(&mo, &c, &st))) return rc;
  Workspace ws;
  if ((rc = open_workspace(c, *st, ray_workspace_bytes(c, n_rays) + 8192, m, &ws))) return rc;
  if ((rc = record_events(*st, c.stream, 0, 2))) return rc;   // no build: its span is empty
  st->planes_done = nullptr;
  DeviceMesh none{};
  if (m->n_tris && (rc = remark_leaves(m, c, m->dm.leaf_max))) return rc;   // the tree as it is marked; keeps the mesh's stream bookkeeping
  if ((rc = run_cast_rays(ws, c, *st, m->n_tris ? m->dm : none, origins, directions, n_rays, o))) return rc;
  return end_mesh_call(m, c, *st, ws.d_err, n_rays, 1);
}

// Surface sampling (include/m2s.h): the one-shot call reads the caller's triangles and builds no tree; the mesh call keeps the table.
int m2s_sample_surface(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes, int topology,
                       size_t n_samples, const m2s_surface_sample_opts* sopts, float* point_out, uint32_t* triangle_out, float* uv_out,
                       float* normal_out, double* area_out, const m2s_opts* opts) {
  clear_error();
  SampleArgs o{point_out, triangle_out, uv_out, normal_out, area_out, 0, 0};
  MeshInput in;
  int rc = mesh_input(vertices, n_vertices, indices, n_indices, index_bytes, topology, &in);
  if (rc) return rc;
  if ((rc = check_sample_args(sopts, n_samples, opts, &o))) return rc;
  if (in.n_tris > ((size_t)1 << 25)) return fail(M2S_ERR_BAD_ARG, "more than 2^25 triangles");
  if ((rc = check_host_indices(opts, in))) return rc;
  if (in.n_tris == 0) return sample_of_nothing(o, n_samples);
  CallCtx c;
  DeviceState* st = nullptr;
  if ((rc = resolve_ctx(opts, &c, &st))) return rc;
  const size_t need = sample_table_bytes(in.n_tris) + sample_scratch_bytes(in.n_tris) + sample_workspace_bytes(c, n_samples) + 4096 +
                      mesh_staging_bytes(c, in);
  Workspace ws;
  if ((rc = open_workspace(c, *st, need, nullptr, &ws))) return rc;
  if ((rc = stage_mesh_input(ws, c, &in))) return rc;
  if ((rc = record_events(*st, c.stream, 0, 2))) return rc;   // no tree: the build's span is empty
  st->planes_done = nullptr;
  SampleTable tb;
  if (sample_table_carve(ws, ws, in.n_tris, &tb)) return fail(M2S_ERR_HIP, "internal: workspace");
  const SampleSrc src{in.dev.d_verts, in.dev.d_indices, (uint32_t)n_vertices, index_bytes, topology, nullptr, nullptr, (uint32_t)in.n_tris};
  uint32_t amax_bits = 0;
  uint64_t W = 0;
  if ((rc = make_sample_table(c, *st, src, tb, ws.d_err, &amax_bits, &W))) return rc;
  if (amax_bits == 0 || W == 0) return sample_of_nothing(o, n_samples);
  if (o.area) *o.area = sample_total_area(amax_bits, W);
  if ((rc = run_sample_surface(ws, c, *st, src, tb, W, n_samples, o))) return rc;
  return finish_feature(c, *st, ws.d_err, in.n_tris, n_samples, 1);
}

int m2s_mesh_sample_surface(m2s_mesh* m, size_t n_samples, const m2s_surface_sample_opts* sopts, float* point_out, uint32_t* triangle_out,
                            float* uv_out, float* normal_out, double* area_out, const m2s_opts* opts) {
  clear_error();
  if (!m) return fail(M2S_ERR_BAD_ARG, "mesh is NULL");
  std::lock_guard<std::mutex> mlk(m->mu);
  SampleArgs o{point_out, triangle_out, uv_out, normal_out, area_out, 0, 0};
  int rc = check_sample_args(sopts, n_samples, opts, &o);
  if (rc) return rc;
  m2s_opts mo;
  if ((rc = mesh_call_opts(m, opts, &mo))) return rc;
  if (m->n_tris == 0) return sample_of_nothing(o, n_samples);
  CallCtx c;
  DeviceState* st = nullptr;
  if ((rc = resolve_ctx(&mo, &c, &st))) return rc;
  const size_t need = (m->samp_mem ? 0 : sample_scratch_bytes(m->n_tris)) + sample_workspace_bytes(c, n_samples) + 8192;
  Workspace ws;
  if ((rc = open_workspace(c, *st, need, m, &ws))) return rc;
  if ((rc = record_events(*st, c.stream, 0, 2))) return rc;   // no build: its span is empty
  st->planes_done = nullptr;
  if ((rc = remark_leaves(m, c, m->dm.leaf_max))) return rc;   // no mark is read or moved; keeps the mesh's stream bookkeeping (`corners` is read)
  const SampleSrc src{nullptr, nullptr, 0, 4, M2S_TRIANGLE_LIST, m->dm.corners, m->dm.slot_of, (uint32_t)m->n_tris};
  if (!m->samp_mem) {
    char* block = nullptr;
    const size_t bytes = sample_table_bytes(m->n_tris);
    M2S_HIP_CHECK(hipMalloc((void**)&block, bytes));
    Arena table{block, bytes, 0};
    SampleTable tb;
    rc = sample_table_carve(table, ws, m->n_tris, &tb) ? fail(M2S_ERR_HIP, "internal: workspace") : 0;
    if (!rc) rc = make_sample_table(c, *st, src, tb, nullptr, &m->samp_amax_bits, &m->samp_W);
    if (rc) { (void)hipFree(block); return rc; }
    m->samp_mem = block;
    m->samp = tb;
    m->samp.A = nullptr;          // scratch of the build: gone with this call's workspace
    m->samp.tile_sum = nullptr;
  }
  if (m->samp_amax_bits == 0 || m->samp_W == 0) return sample_of_nothing(o, n_samples);
  if (o.area) *o.area = sample_total_area(m->samp_amax_bits, m->samp_W);
  if ((rc = run_sample_surface(ws, c, *st, src, m->samp, m->samp_W, n_samples, o))) return rc;
  return end_mesh_call(m, c, *st, ws.d_err, n_samples, 1);
}

// Voxelization (include/m2s.h): the one-shot call builds the triangle records and nothing else; the mesh call reads its resident records.
// (Voxelization and the narrow bands check the grid and their options before the mesh, the other four families the mesh first; kept.)
int m2s_voxelize(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes, int topology,
                 const m2s_grid* grid, const m2s_voxelize_opts* vopts, uint32_t* bits_out, uint8_t* occupancy_out, uint64_t* cells_out,
                 uint64_t cell_capacity, uint64_t* n_set_out, const m2s_opts* opts) {
  clear_error();
  VoxelArgs o{bits_out, occupancy_out, cells_out, cell_capacity, n_set_out, M2S_VOXELIZE_SURFACE};
  GridParams g;
  size_t cells = 0;
  int rc = check_voxel_args(grid, vopts, opts, &o, &g, &cells);
  if (rc) return rc;
  MeshInput in;
  if ((rc = mesh_input(vertices, n_vertices, indices, n_indices, index_bytes, topology, &in))) return rc;
  if (in.n_tris > ((size_t)1 << 25)) return fail(M2S_ERR_BAD_ARG, "more than 2^25 triangles");
  if ((rc = check_host_indices(opts, in))) return rc;
  CallCtx c;
  DeviceState* st = nullptr;
  if ((rc = resolve_ctx(opts, &c, &st))) return rc;
  const size_t need = bvh_workspace_bytes(in.n_tris) + voxel_workspace_bytes(c, g, in.n_tris, cells, o) + 4096 + mesh_staging_bytes(c, in);
  Workspace ws;
  if ((rc = open_workspace(c, *st, need, nullptr, &ws))) return rc;
  if ((rc = stage_mesh_input(ws, c, &in))) return rc;
  M2S_HIP_CHECK(hipEventRecord(st->ev[0], c.stream));
  DeviceMesh mesh;
  if ((rc = build_mesh(ws, c, in, &mesh, true, 2))) return rc;
  M2S_HIP_CHECK(hipEventRecord(st->ev[1], c.stream));
  bool short_capacity = false;
  if ((rc = run_voxelize(ws, c, *st, mesh, g, cells, o, &short_capacity))) return rc;
  return voxelize_result(c, o, finish_feature(c, *st, ws.d_err, in.n_tris, cells, 1), short_capacity);
}

int m2s_mesh_voxelize(m2s_mesh* m, const m2s_grid* grid, const m2s_voxelize_opts* vopts, uint32_t* bits_out, uint8_t* occupancy_out,
                      uint64_t* cells_out, uint64_t cell_capacity, uint64_t* n_set_out, const m2s_opts* opts) {
  clear_error();
  if (!m) return fail(M2S_ERR_BAD_ARG, "mesh is NULL");
  std::lock_guard<std::mutex> mlk(m->mu);
  VoxelArgs o{bits_out, occupancy_out, cells_out, cell_capacity, n_set_out, M2S_VOXELIZE_SURFACE};
  GridParams g;
  size_t cells = 0;
  int rc = check_voxel_args(grid, vopts, opts, &o, &g, &cells);
  if (rc) return rc;
  m2s_opts mo;
  if ((rc = mesh_call_opts(m, opts, &mo))) return rc;
  CallCtx c;
  DeviceState* st = nullptr;
  if ((rc = resolve_ctx(&mo, &c, &st))) return rc;
  Workspace ws;
  if ((rc = open_workspace(c, *st, voxel_workspace_bytes(c, g, m->n_tris, cells, o) + 8192, m, &ws))) return rc;
  if ((rc = record_events(*st, c.stream, 0, 1))) return rc;   // no build: its span is empty
  if ((rc = remark_leaves(m, c, m->dm.leaf_max))) return rc;   // no mark is read or moved; keeps the mesh's stream bookkeeping (the records are read)
  bool short_capacity = false;
  if ((rc = run_voxelize(ws, c, *st, m->dm, g, cells, o, &short_capacity))) return rc;
  return voxelize_result(c, o, end_mesh_call(m, c, *st, ws.d_err, cells, 1), short_capacity);
}

// Narrow bands (include/m2s.h): the one-shot call builds the whole tree, with the leaf size the query walk of a chunk asks for (algorithm 1:
// the dense grid call's).
int m2s_narrow_band_sdf(const float* vertices, size_t n_vertices, const void* indices, size_t n_indices, int index_bytes, int topology,
                        const m2s_grid* grid, int sign_method, const m2s_band_opts* bopts, uint64_t* cells_out, float* distances_out,
                        uint64_t capacity, uint32_t* bits_out, uint64_t* n_active_out, const m2s_opts* opts) {
  clear_error();
  BandArgs o{cells_out, distances_out, capacity, bits_out, n_active_out, 0.0f, 0.0f, sign_method};
  GridParams g;
  size_t cells = 0;
  int rc = check_band_args(grid, bopts, opts, &o, &g, &cells);
  if (rc) return rc;
  MeshInput in;
  if ((rc = mesh_input(vertices, n_vertices, indices, n_indices, index_bytes, topology, &in))) return rc;
  if (in.n_tris > ((size_t)1 << 25)) return fail(M2S_ERR_BAD_ARG, "more than 2^25 triangles");
  if ((rc = check_host_indices(opts, in))) return rc;
  CallCtx c;
  DeviceState* st = nullptr;
  if ((rc = resolve_ctx(opts, &c, &st))) return rc;
  const size_t need = bvh_workspace_bytes(in.n_tris) + band_workspace_bytes(c, g, in.n_tris, cells, o) + 4096 + mesh_staging_bytes(c, in);
  Workspace ws;
  if ((rc = open_workspace(c, *st, need, nullptr, &ws))) return rc;
  if ((rc = stage_mesh_input(ws, c, &in))) return rc;
  M2S_HIP_CHECK(hipEventRecord(st->ev[0], c.stream));
  DeviceMesh mesh;
  const uint32_t leaf = c.algorithm == 1 ? grid_leaf_max(g, in.n_tris) : query_leaf_max(band_chunk_of(cells), in.n_tris, SIGN_NONE);
  if ((rc = build_mesh(ws, c, in, &mesh, false, leaf))) return rc;
  M2S_HIP_CHECK(hipEventRecord(st->ev[1], c.stream));
  uint64_t n_cand = 0;
  bool short_capacity = false;
  if ((rc = run_narrow_band(ws, c, *st, mesh, g, cells, o, ws.d_err, &n_cand, &short_capacity))) return rc;
  return narrow_band_result(o, finish_feature(c, *st, ws.d_err, in.n_tris, n_cand, 1), short_capacity);
}

int m2s_mesh_narrow_band_sdf(m2s_mesh* m, const m2s_grid* grid, int sign_method, const m2s_band_opts* bopts, uint64_t* cells_out,
                             float* distances_out, uint64_t capacity, uint32_t* bits_out, uint64_t* n_active_out, const m2s_opts* opts) {
  clear_error();
  if (!m) return fail(M2S_ERR_BAD_ARG, "mesh is NULL");
  std::lock_guard<std::mutex> mlk(m->mu);
  BandArgs o{cells_out, distances_out, capacity, bits_out, n_active_out, 0.0f, 0.0f, sign_method};
  GridParams g;
  size_t cells = 0;
  int rc = check_band_args(grid, bopts, opts, &o, &g, &cells);
  if (rc) return rc;
  m2s_opts mo;
  if ((rc = mesh_call_opts(m, opts, &mo))) return rc;
  CallCtx c;
  DeviceState* st = nullptr;
  if ((rc = resolve_ctx(&mo, &c, &st))) return rc;
  Workspace ws;
  if ((rc = open_workspace(c, *st, band_workspace_bytes(c, g, m->n_tris, cells, o) + 8192, m, &ws))) return rc;
  if ((rc = record_events(*st, c.stream, 0, 1))) return rc;   // no build: its span is empty
  const size_t chunk = band_chunk_of(cells);
  const uint32_t leaf = c.algorithm == 1 ? grid_leaf_max(g, m->n_tris)
                        : query_is_tiny(chunk, m->n_tris, 0, SIGN_NONE) ? m->dm.leaf_max : query_leaf_max(chunk, m->n_tris, SIGN_NONE);
  if ((rc = remark_leaves(m, c, leaf))) return rc;
  uint64_t n_cand = 0;
  bool short_capacity = false;
  if ((rc = run_narrow_band(ws, c, *st, m->dm, g, cells, o, ws.d_err, &n_cand, &short_capacity))) return rc;
  return narrow_band_result(o, end_mesh_call(m, c, *st, ws.d_err, n_cand, 1), short_capacity);
}

}  // extern "C"
