// bounds_probe.hip — test hook m2s_debug_eval (not part of include/m2s.h): the walks' lower bounds, the exact evaluation's d2 and the
// pruning threshold, evaluated ON THE DEVICE, element by element, on records the caller supplies.  tests/test_gpu_bounds.py compares
// them with an f64 model on the host (tests/bounds_model.py): what a walk may skip is decided by these functions alone, and they cannot
// be probed on the host (__builtin_amdgcn_sqrtf, explicit FMAs).
//
// Nothing of walk.hip.h is restated here: the kernel calls its inline functions.  One thread per element, one record per element, no
// index into anything: element i reads points[3 i ..], records[i], aux[2 i ..] and writes out[i].  No kernel of a distance call lives
// in this unit, and none of theirs changes by it.
#include <hip/hip_runtime.h>

#include "../../include/m2s.h"
#include "capi_internal.h"
#include "common.h"
#include "walk.hip.h"

namespace m2s {

namespace {

enum : int { EVAL_EXT = 0, EVAL_PLANES = 1, EVAL_DIST2 = 2, EVAL_SLACK = 3, EVAL_PRUNE = 4, EVAL_KINDS = 5 };

// The slack of a walk over a mesh of scale `mesh_scale` for the point p, written as the walks write it: distance.hip k_packet, k_group,
// k_lane, k_lane_q and the split walk's rounds ("const float scale = fmaxf(mesh_scale(mesh), ...); const float slack = 4.0e-6f * scale
// + (MODE == MODE_NORMAL_FOLD ? 2.5e-6f : 0.0f);"), and closest.hip closest_search ("4.0e-6f * scale": the MODE_UNSIGNED value).
template <int MODE>
__device__ __forceinline__ float walk_slack(float mesh_scale, f3 p) {
  const float scale = fmaxf(mesh_scale, fmaxf(fabsf(p.x), fmaxf(fabsf(p.y), fabsf(p.z))));
  const float slack = 4.0e-6f * scale + (MODE == MODE_NORMAL_FOLD ? 2.5e-6f : 0.0f);
  return slack;
}

__global__ __launch_bounds__(256) void k_bounds_eval(int kind, size_t n, const float* __restrict__ points, const void* __restrict__ records,
                                                     const float* __restrict__ aux, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  f3 p = mk3(0.0f, 0.0f, 0.0f);
  if (points) p = mk3(points[3 * i], points[3 * i + 1], points[3 * i + 2]);
  float r;
  if (kind == EVAL_EXT) {
    r = ext_dist2(p, static_cast<const NodeExt*>(records)[i]);
  } else if (kind == EVAL_PLANES) {
    r = planes_dist2(p, static_cast<const TriPlanes*>(records)[i]);
  } else if (kind == EVAL_DIST2) {
    Best<MODE_UNSIGNED> best;
    eval_triangle<MODE_UNSIGNED>(best, p, static_cast<const TriRec*>(records)[i]);
    r = best.d2;
  } else if (kind == EVAL_SLACK) {
    r = aux[2 * i + 1] != 0.0f ? walk_slack<MODE_NORMAL_FOLD>(aux[2 * i], p) : walk_slack<MODE_UNSIGNED>(aux[2 * i], p);
  } else {
    r = prune_bound(aux[2 * i], aux[2 * i + 1]);
  }
  out[i] = r;
}

struct DeviceBuffers {
  void* p[4] = {nullptr, nullptr, nullptr, nullptr};
  ~DeviceBuffers() {
    for (void* q : p)
      if (q) (void)hipFree(q);
  }
};

}  // namespace

}  // namespace m2s

using namespace m2s;

extern "C" {

// kind: 0 ext_dist2(p, NodeExt), 1 planes_dist2(p, TriPlanes), 2 the d2 of eval_triangle<MODE_UNSIGNED> on a fresh Best (TriRec),
// 3 the walks' slack for p (aux[2 i] = the mesh's scale, aux[2 i + 1] != 0: with the Normal fold's term), 4 prune_bound(aux[2 i], aux[2 i + 1]).
// Host pointers, n elements each; synchronous, on the current device.  An argument a kind does not read may be NULL.
int m2s_debug_eval(int kind, size_t n, const float* points, const void* records, const float* aux, float* out) {
  clear_error();
  if (kind < 0 || kind >= EVAL_KINDS) return fail(M2S_ERR_BAD_ARG, "m2s_debug_eval: kind = %d (0 .. %d)", kind, EVAL_KINDS - 1);
  if (n > ((size_t)1 << 26)) return fail(M2S_ERR_BAD_ARG, "m2s_debug_eval: more than 2^26 elements");
  const bool wants_points = kind != EVAL_PRUNE, wants_records = kind <= EVAL_DIST2, wants_aux = kind >= EVAL_SLACK;
  if (n && (!out || (wants_points && !points) || (wants_records && !records) || (wants_aux && !aux)))
    return fail(M2S_ERR_BAD_ARG, "m2s_debug_eval: NULL argument");
  if (n == 0) return M2S_OK;
  const size_t rec_bytes = kind == EVAL_EXT ? sizeof(NodeExt) : kind == EVAL_PLANES ? sizeof(TriPlanes) : sizeof(TriRec);
  DeviceBuffers d;
  if (wants_points) {
    M2S_HIP_CHECK(hipMalloc(&d.p[0], n * 12));
    M2S_HIP_CHECK(hipMemcpy(d.p[0], points, n * 12, hipMemcpyHostToDevice));
  }
  if (wants_records) {
    M2S_HIP_CHECK(hipMalloc(&d.p[1], n * rec_bytes));
    M2S_HIP_CHECK(hipMemcpy(d.p[1], records, n * rec_bytes, hipMemcpyHostToDevice));
  }
  if (wants_aux) {
    M2S_HIP_CHECK(hipMalloc(&d.p[2], n * 8));
    M2S_HIP_CHECK(hipMemcpy(d.p[2], aux, n * 8, hipMemcpyHostToDevice));
  }
  M2S_HIP_CHECK(hipMalloc(&d.p[3], n * 4));
  hipLaunchKernelGGL(k_bounds_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, kind, n, (const float*)d.p[0], (const void*)d.p[1],
                     (const float*)d.p[2], (float*)d.p[3]);
  M2S_HIP_CHECK(hipGetLastError());
  M2S_HIP_CHECK(hipDeviceSynchronize());
  M2S_HIP_CHECK(hipMemcpy(out, d.p[3], n * 4, hipMemcpyDeviceToHost));
  return M2S_OK;
}

}  // extern "C"
