// peer_push.hip — the two copy kernels that deliver a slab to the other devices' whole-grid buffers (gfx950): k_push_cells after a
// piece is finished (M2S_PEER_PUSH), k_push_trailing beside the walk, unit by unit as it counts them finished (M2S_PEER_TRAIL).
#include <algorithm>

#include "common.h"
#include "tuning.h"
#include "walk.hip.h"

namespace m2s {

namespace {

// M2S_PEER_TRAIL: pushes the slab to the peers unit by unit while the walk is still running.  Unit u = the x-layers of
// 2^unit_log bricks; it is complete when progress[u] has reached the number of packets that lie in it.  Every workgroup waits
// for the unit (one lane polls, s_sleep between polls), then copies its share of it with 16 B per lane to every peer.
// A walk that never finishes (a fault on its stream) would leave this kernel spinning: after ~2 s without progress it
// raises ERRF_TRAIL_TIMEOUT and leaves.
__global__ __launch_bounds__(256) void k_push_trailing(const float* __restrict__ src, PeerOut peers, uint64_t slab_first, uint64_t row_cells,
                                                       uint32_t layers, uint32_t layers_per_unit, uint32_t n_units, int* __restrict__ err) {
  __shared__ int ok;
  for (uint32_t u = 0; u < n_units; ++u) {
    if (threadIdx.x == 0) {
      int good = 1;
      uint32_t spins = 0;
      while (__hip_atomic_load(&peers.progress[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < peers.rows) {   // all brick rows of the unit
        __builtin_amdgcn_s_sleep(127);
        if (++spins > 10000000u) { good = 0; atomicOr(err, ERRF_TRAIL_TIMEOUT); break; }
      }
      ok = good;
    }
    __syncthreads();
    if (!ok) return;
    const uint32_t x0 = u * layers_per_unit, x1 = min(layers, x0 + layers_per_unit);
    const uint64_t first = slab_first + (uint64_t)x0 * row_cells, count = (uint64_t)(x1 - x0) * row_cells;
    // row_cells * 4 B and the slab start need not be 16-byte multiples: head / body / tail as in k_push_cells
    const uint64_t head = min(count, (uint64_t)((4u - (uint32_t)(first & 3u)) & 3u));
    const uint64_t n4 = (count - head) >> 2, tail0 = head + (n4 << 2);
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
    // the values were written by waves on other XCDs: read them past this XCD's L2 (device-scope loads; they only exist in 32 bits)
    const float* s1 = src + first + head;
    for (uint64_t i = tid; i < n4; i += stride) {
      float4 v;
      v.x = __hip_atomic_load(s1 + 4 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      v.y = __hip_atomic_load(s1 + 4 * i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      v.z = __hip_atomic_load(s1 + 4 * i + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      v.w = __hip_atomic_load(s1 + 4 * i + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (uint32_t k = 0; k < peers.n; ++k) reinterpret_cast<float4*>(peers.p[k] + first + head)[i] = v;
    }
    if (tid < head) {
      const float v = __hip_atomic_load(src + first + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (uint32_t k = 0; k < peers.n; ++k) peers.p[k][first + tid] = v;
    }
    if (tid < count - tail0) {
      const float v = __hip_atomic_load(src + first + tail0 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (uint32_t k = 0; k < peers.n; ++k) peers.p[k][first + tail0 + tid] = v;
    }
    __syncthreads();                                         // `ok` is rewritten for the next unit
  }
}

// M2S_PEER_PUSH: one slab piece of the finished whole-grid buffer to every peer, 16 B per lane.
__global__ __launch_bounds__(256) void k_push_cells(const float* __restrict__ src, PeerOut peers, uint64_t first, uint64_t count) {
  // head: up to the next 16-byte boundary; body: float4; tail: the rest
  const uint64_t head = min(count, (uint64_t)((4u - (uint32_t)(first & 3u)) & 3u));
  const uint64_t n4 = (count - head) >> 2, tail0 = head + (n4 << 2);
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
  const float4* s4 = reinterpret_cast<const float4*>(src + first + head);
  for (uint64_t i = tid; i < n4; i += stride) {
    const float4 v = s4[i];
    for (uint32_t k = 0; k < peers.n; ++k) reinterpret_cast<float4*>(peers.p[k] + first + head)[i] = v;
  }
  if (tid < head) {
    const float v = src[first + tid];
    for (uint32_t k = 0; k < peers.n; ++k) peers.p[k][first + tid] = v;
  }
  if (tid < count - tail0) {
    const float v = src[first + tail0 + tid];
    for (uint32_t k = 0; k < peers.n; ++k) peers.p[k][first + tail0 + tid] = v;
  }
}

}  // namespace

int launch_push_cells(hipStream_t st, const float* src, const PeerOut& peers, uint64_t first, uint64_t count) {
  if (peers.n == 0 || count == 0) return 0;
  // a bandwidth-bound copy next to the walk of the following piece: enough workgroups to keep every xGMI link busy,
  // few enough to leave the CUs to the walk (M2S_PUSH_BLOCKS)
  const unsigned max_blocks = tuning().push_blocks ? tuning().push_blocks : 256u;
  const uint64_t want = (count / 4 + 255) / 256 + 1;
  const unsigned blocks = (unsigned)std::min<uint64_t>(max_blocks, want);
  hipLaunchKernelGGL(k_push_cells, dim3(blocks), dim3(256), 0, st, src, peers, first, count);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

uint32_t trail_unit_log(const GridParams& g) {
  (void)g;
  return 2u;   // 4 bricks = 16 layers of a 4^3-brick grid (16 MB per peer and unit at 512^2 rows): 2-brick units stream finer but
               // their packet order (super-bricks 2 bricks wide) costs the walk 20 % of its locality
}
uint32_t trail_units(const GridParams& g) {
  const uint32_t nbx = bricks_along(g.xe - g.xb, g.bl[0]), ul = trail_unit_log(g);
  return (nbx + (1u << ul) - 1u) >> ul;
}
uint32_t trail_rows(const GridParams& g) { return bricks_along(g.n[1], g.bl[1]); }
int launch_push_trailing(hipStream_t st, const float* src, const PeerOut& peers, const GridParams& g, int* d_err) {
  if (peers.n == 0 || g.xe <= g.xb) return 0;
  const unsigned blocks = tuning().push_blocks ? tuning().push_blocks : 64u;
  const uint64_t row = (uint64_t)g.n[1] * g.n[2];
  hipLaunchKernelGGL(k_push_trailing, dim3(blocks), dim3(256), 0, st, src, peers, (uint64_t)g.xb * row - g.out_off, row, g.xe - g.xb,
                     (1u << g.bl[0]) << peers.unit_log, trail_units(g), d_err);
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

// m2s_warmup: this unit's code object, and the kernel functions of it that a first call uses (see warm_distance).
__global__ void k_warm_peer_push() {}
void warm_peer_push(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_peer_push, dim3(1), dim3(64), 0, st);
  const void* fns[] = {
      (const void*)k_push_cells};
  hipFuncAttributes attr;
  for (const void* f : fns) (void)hipFuncGetAttributes(&attr, f);
  (void)hipGetLastError();
}

}  // namespace m2s
