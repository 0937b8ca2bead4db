// grid_query.hip — queries on a finished grid SDF: the reference client's ray-marching shader
// (mesh_to_sdf_client/shaders/draw_raymarching.wgsl) restated for gfx950.
//   sdf_grid        :118-200   sample a point: snap, trilinear or tetrahedral over clamped cell reads (get_distance :92-99)
//   estimate_normal :202-209   central differences of six samples, normalised
//   sdf_3d          :265-287   enter the grid box (intersectAABB :245-253) and sphere-trace
//   compute_tetrahedral_barycenter :585-640
// Numerics: IEEE binary32 in the shader's operation order, no FMA (-ffp-contract=off and the pragma below); `/` and
// sqrtf are the correctly rounded forms.  tests/grid_query_model.py is the same arithmetic in numpy, and the GPU tests
// compare the two bit for bit.
//
// One lane per point or ray, grid-stride over 64-bit indices.  A sample computes all its corner offsets before the
// first load (8 trilinear, 4 tetrahedral, 1 snap), and a normal prepares its six samples before any of their loads,
// so a lane has up to 48 independent loads in flight instead of six dependent rounds.
#include "../../include/m2s.h"
#include "common.h"

#pragma clang fp contract(off)

namespace m2s {

namespace {

constexpr uint32_t kQNaN = 0x7fc00000u;   // the NaN every NaN input produces (the model uses the same bits)

__device__ __forceinline__ float qnan() { return __uint_as_float(kQNaN); }

template <int MODE>
struct Corners { static constexpr int K = MODE == M2S_SAMPLE_SNAP ? 1 : MODE == M2S_SAMPLE_TRILINEAR ? 8 : 4; };

// One sample prepared: the clamped cell offsets it reads and its interpolation weights.
// state: 0 inside the box, 1 outside (the result is `outside`), 2 a NaN coordinate (the result is NaN).
template <int MODE>
struct Prep {
  uint64_t off[Corners<MODE>::K];
  float w[4];   // trilinear: fx, fy, fz; tetrahedral: bary
  int state;
};

__device__ __forceinline__ int64_t clamp_cell(int64_t i, int64_t n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// get_distance (:92-99) without the load: each index clamped to [0, count - 1], offset z + y*nz + x*ny*nz in 64 bits.
__device__ __forceinline__ uint64_t cell_off(const GridQuery& q, int64_t x, int64_t y, int64_t z) {
  return (uint64_t)clamp_cell(z, q.n[2]) + (uint64_t)clamp_cell(y, q.n[1]) * (uint64_t)q.n[2] +
         (uint64_t)clamp_cell(x, q.n[0]) * q.nyz;
}

template <int MODE>
__device__ __forceinline__ Prep<MODE> prepare(const GridQuery& q, float px, float py, float pz) {
  Prep<MODE> r;
  const bool nan = px != px || py != py || pz != pz;
  // :121 any(position < start) || any(position > end); a NaN coordinate fails every comparison and is caught above
  const bool out = px < q.start[0] || py < q.start[1] || pz < q.start[2] || px > q.end[0] || py > q.end[1] || pz > q.end[2];
  r.state = nan ? 2 : (out ? 1 : 0);
  if (r.state) { px = q.start[0]; py = q.start[1]; pz = q.start[2]; }   // keeps the conversions below defined and the reads in the grid
  if (MODE == M2S_SAMPLE_SNAP) {
    // :129-134 start_grid = start - cell_size * 0.5; cell_index = floor((position - start_grid) / cell_size)
    const float gx = q.start[0] - q.cs[0] * 0.5f, gy = q.start[1] - q.cs[1] * 0.5f, gz = q.start[2] - q.cs[2] * 0.5f;
    const int64_t ix = (int64_t)floorf((px - gx) / q.cs[0]);
    const int64_t iy = (int64_t)floorf((py - gy) / q.cs[1]);
    const int64_t iz = (int64_t)floorf((pz - gz) / q.cs[2]);
    r.off[0] = cell_off(q, ix, iy, iz);
  } else {
    // :159-161 / :181-183 cell_index = (position - start) / cell_size; fract = c - floor(c); idx = floor(c)
    const float cx = (px - q.start[0]) / q.cs[0], cy = (py - q.start[1]) / q.cs[1], cz = (pz - q.start[2]) / q.cs[2];
    const float flx = floorf(cx), fly = floorf(cy), flz = floorf(cz);
    const float fx = cx - flx, fy = cy - fly, fz = cz - flz;
    const int64_t ix = (int64_t)flx, iy = (int64_t)fly, iz = (int64_t)flz;
    if (MODE == M2S_SAMPLE_TRILINEAR) {
      r.w[0] = fx; r.w[1] = fy; r.w[2] = fz; r.w[3] = 0.0f;
#pragma unroll
      for (int k = 0; k < 8; ++k) r.off[k] = cell_off(q, ix + (k & 1), iy + ((k >> 1) & 1), iz + (k >> 2));
    } else {
      // compute_tetrahedral_barycenter (:585-640): the six cases in the shader's order, the LAST matching one wins
      // (r, g, b) = (x, y, z); vert2 / vert3 are the two middle vertices of the tetrahedron
      float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, b3 = 0.0f;
      int v2 = 0, v3 = 0;   // bits: x = 1, y = 2, z = 4
      if (fy >= fz && fz >= fx) { b0 = 1.0f - fy; b1 = fy - fz; b2 = fz - fx; b3 = fx; v2 = 2; v3 = 6; }
      if (fz > fx && fx > fy)   { b0 = 1.0f - fz; b1 = fz - fx; b2 = fx - fy; b3 = fy; v2 = 4; v3 = 5; }
      if (fz > fy && fy >= fx)  { b0 = 1.0f - fz; b1 = fz - fy; b2 = fy - fx; b3 = fx; v2 = 4; v3 = 6; }
      if (fx >= fy && fy > fz)  { b0 = 1.0f - fx; b1 = fx - fy; b2 = fy - fz; b3 = fz; v2 = 1; v3 = 3; }
      if (fy > fx && fx >= fz)  { b0 = 1.0f - fy; b1 = fy - fx; b2 = fx - fz; b3 = fz; v2 = 2; v3 = 3; }
      if (fx >= fz && fz >= fy) { b0 = 1.0f - fx; b1 = fx - fz; b2 = fz - fy; b3 = fy; v2 = 1; v3 = 5; }
      r.w[0] = b0; r.w[1] = b1; r.w[2] = b2; r.w[3] = b3;
      r.off[0] = cell_off(q, ix, iy, iz);
      r.off[1] = cell_off(q, ix + (v2 & 1), iy + ((v2 >> 1) & 1), iz + (v2 >> 2));
      r.off[2] = cell_off(q, ix + (v3 & 1), iy + ((v3 >> 1) & 1), iz + (v3 >> 2));
      r.off[3] = cell_off(q, ix + 1, iy + 1, iz + 1);
    }
  }
  return r;
}

template <int MODE>
__device__ __forceinline__ void load(const float* __restrict__ d, const Prep<MODE>& p, float* v) {
#pragma unroll
  for (int k = 0; k < Corners<MODE>::K; ++k) v[k] = d[p.off[k]];   // unconditional: a point off the box reads its start cell
}

// The arithmetic of sdf_grid after the reads; v[k] are the raw cell values (get_distance subtracts iso from each).
template <int MODE>
__device__ __forceinline__ float combine(const GridQuery& q, const Prep<MODE>& p, const float* v) {
  const float iso = q.iso;
  float val;
  if (MODE == M2S_SAMPLE_SNAP) {
    val = v[0] - iso;
  } else if (MODE == M2S_SAMPLE_TRILINEAR) {
    // :164-172; v[dx + 2 dy + 4 dz]
    const float fx = p.w[0], fy = p.w[1], fz = p.w[2];
    const float gx = 1.0f - fx, gy = 1.0f - fy, gz = 1.0f - fz;
    const float c_x00 = (v[0] - iso) * gx + (v[1] - iso) * fx;
    const float c_x01 = (v[4] - iso) * gx + (v[5] - iso) * fx;
    const float c_x10 = (v[2] - iso) * gx + (v[3] - iso) * fx;
    const float c_x11 = (v[6] - iso) * gx + (v[7] - iso) * fx;
    const float c_xy0 = c_x00 * gy + c_x10 * fy;
    const float c_xy1 = c_x01 * gy + c_x11 * fy;
    val = c_xy0 * gz + c_xy1 * fz;
  } else {
    // :187-196 dot(bary, samples), left to right
    val = p.w[0] * (v[0] - iso) + p.w[1] * (v[1] - iso) + p.w[2] * (v[2] - iso) + p.w[3] * (v[3] - iso);
  }
  // selected at the end, not branched on: a branch lets the compiler sink the reads into it and wait on them one pair at a time
  return p.state == 2 ? qnan() : (p.state == 1 ? q.outside : val);
}

template <int MODE>
__device__ __forceinline__ float sample(const GridQuery& q, const float* __restrict__ d, float px, float py, float pz) {
  const Prep<MODE> p = prepare<MODE>(q, px, py, pz);
  float v[Corners<MODE>::K];
  load<MODE>(d, p, v);
  return combine<MODE>(q, p, v);
}

// estimate_normal (:202-209): the six samples are prepared first and their reads issued as one batch.
// normalize(v) = v / sqrtf(dot(v, v)); a vector of length 0 gives (0, 0, 0), a NaN point NaN x 3.
template <int MODE>
__device__ __forceinline__ void normal(const GridQuery& q, const float* __restrict__ d, float px, float py, float pz, float* nrm) {
  const float e = q.eps;
  Prep<MODE> p[6];
  p[0] = prepare<MODE>(q, px + e, py, pz);
  p[1] = prepare<MODE>(q, px - e, py, pz);
  p[2] = prepare<MODE>(q, px, py + e, pz);
  p[3] = prepare<MODE>(q, px, py - e, pz);
  p[4] = prepare<MODE>(q, px, py, pz + e);
  p[5] = prepare<MODE>(q, px, py, pz - e);
  float v[6][Corners<MODE>::K];
#pragma unroll
  for (int j = 0; j < 6; ++j) load<MODE>(d, p[j], v[j]);
  float s[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) s[j] = combine<MODE>(q, p[j], v[j]);
  const float nx = s[0] - s[1], ny = s[2] - s[3], nz = s[4] - s[5];
  const float len = sqrtf(nx * nx + ny * ny + nz * nz);
  if (px != px || py != py || pz != pz) {
    nrm[0] = nrm[1] = nrm[2] = qnan();
  } else if (len == 0.0f) {
    nrm[0] = nrm[1] = nrm[2] = 0.0f;
  } else {
    nrm[0] = nx / len; nrm[1] = ny / len; nrm[2] = nz / len;
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_sample_grid(GridQuery q, const float* __restrict__ d, const float* __restrict__ pts, uint64_t n,
                                                     float* __restrict__ value_out, float* __restrict__ normal_out) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    if (value_out) value_out[i] = sample<MODE>(q, d, px, py, pz);
    if (normal_out) {
      float nrm[3];
      normal<MODE>(q, d, px, py, pz, nrm);
      normal_out[3 * i] = nrm[0]; normal_out[3 * i + 1] = nrm[1]; normal_out[3 * i + 2] = nrm[2];
    }
  }
}

// sdf_3d (:265-287) with `iso` for surface_iso and max_steps for MAX_STEPS.  Outside the box the ray enters it through
// intersectAABB (:245-253) with fminf / fmaxf (the non-NaN operand wins: a zero direction component is well defined).
template <int MODE>
__global__ __launch_bounds__(256) void k_raymarch_grid(GridQuery q, const float* __restrict__ d, const float* __restrict__ org,
                                                       const float* __restrict__ dir, uint64_t n, float* __restrict__ hit_out,
                                                       uint32_t* __restrict__ steps_out, float* __restrict__ normal_out) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const float ox = org[3 * i], oy = org[3 * i + 1], oz = org[3 * i + 2];
    const float dx = dir[3 * i], dy = dir[3 * i + 1], dz = dir[3 * i + 2];
    float px = ox, py = oy, pz = oz, dist = 0.0f;
    uint32_t steps = 0;
    bool march = true;
    if (ox != ox || oy != oy || oz != oz || dx != dx || dy != dy || dz != dz) {
      px = py = pz = dist = qnan();
      march = false;
    } else if (ox < q.start[0] || oy < q.start[1] || oz < q.start[2] || ox > q.end[0] || oy > q.end[1] || oz > q.end[2]) {
      const float t0x = (q.start[0] - ox) / dx, t0y = (q.start[1] - oy) / dy, t0z = (q.start[2] - oz) / dz;
      const float t1x = (q.end[0] - ox) / dx, t1y = (q.end[1] - oy) / dy, t1z = (q.end[2] - oz) / dz;
      const float nx = fminf(t0x, t1x), ny = fminf(t0y, t1y), nz = fminf(t0z, t1z);
      const float fx = fmaxf(t0x, t1x), fy = fmaxf(t0y, t1y), fz = fmaxf(t0z, t1z);
      const float t_near = fmaxf(fmaxf(nx, ny), nz);
      const float t_far = fminf(fminf(fx, fy), fz);
      if (t_near > t_far) {   // :275-278 outside the box
        px = py = pz = 0.0f;
        dist = 1.0f;
        march = false;
      } else {
        const float t = t_near + q.eps;   // :280 eye + (box_hit.x + epsilon) * ray
        px = ox + t * dx; py = oy + t * dy; pz = oz + t * dz;
      }
    }
    if (march) {
      for (uint32_t s = 0; s < q.max_steps; ++s) {   // :283-289
        dist = sample<MODE>(q, d, px, py, pz);
        if (dist < q.eps) break;
        px = px + dx * dist; py = py + dy * dist; pz = pz + dz * dist;
        ++steps;
      }
    }
    if (hit_out) { hit_out[4 * i] = px; hit_out[4 * i + 1] = py; hit_out[4 * i + 2] = pz; hit_out[4 * i + 3] = dist; }
    if (steps_out) steps_out[i] = steps;
    if (normal_out) {
      float nrm[3] = {0.0f, 0.0f, 0.0f};
      if (march && dist < q.eps) normal<MODE>(q, d, px, py, pz, nrm);   // a hit: the ray entered the box and got closer than eps
      normal_out[3 * i] = nrm[0]; normal_out[3 * i + 1] = nrm[1]; normal_out[3 * i + 2] = nrm[2];
    }
  }
}

constexpr uint64_t kMaxBlocks = 1u << 20;   // beyond 2^28 lanes the grid-stride loop takes over

unsigned blocks_for(uint64_t n) { return (unsigned)std::min<uint64_t>(kMaxBlocks, (n + 255) / 256); }

}  // namespace

int launch_sample_grid(hipStream_t st, const GridQuery& q, int mode, const float* d, const float* pts, uint64_t n, float* value_out,
                       float* normal_out) {
  if (n == 0) return 0;
  const dim3 grid(blocks_for(n)), block(256);
  switch (mode) {
    case M2S_SAMPLE_SNAP: hipLaunchKernelGGL(k_sample_grid<M2S_SAMPLE_SNAP>, grid, block, 0, st, q, d, pts, n, value_out, normal_out); break;
    case M2S_SAMPLE_TRILINEAR: hipLaunchKernelGGL(k_sample_grid<M2S_SAMPLE_TRILINEAR>, grid, block, 0, st, q, d, pts, n, value_out, normal_out); break;
    default: hipLaunchKernelGGL(k_sample_grid<M2S_SAMPLE_TETRAHEDRAL>, grid, block, 0, st, q, d, pts, n, value_out, normal_out); break;
  }
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_raymarch_grid(hipStream_t st, const GridQuery& q, int mode, const float* d, const float* org, const float* dir, uint64_t n,
                         float* hit_out, uint32_t* steps_out, float* normal_out) {
  if (n == 0) return 0;
  const dim3 grid(blocks_for(n)), block(256);
  switch (mode) {
    case M2S_SAMPLE_SNAP: hipLaunchKernelGGL(k_raymarch_grid<M2S_SAMPLE_SNAP>, grid, block, 0, st, q, d, org, dir, n, hit_out, steps_out, normal_out); break;
    case M2S_SAMPLE_TRILINEAR: hipLaunchKernelGGL(k_raymarch_grid<M2S_SAMPLE_TRILINEAR>, grid, block, 0, st, q, d, org, dir, n, hit_out, steps_out, normal_out); break;
    default: hipLaunchKernelGGL(k_raymarch_grid<M2S_SAMPLE_TETRAHEDRAL>, grid, block, 0, st, q, d, org, dir, n, hit_out, steps_out, normal_out); break;
  }
  M2S_HIP_CHECK(hipGetLastError());
  return 0;
}

// m2s_warmup: the first launch of a kernel of this translation unit makes the runtime load its code object (all its kernels).
__global__ void k_warm_grid_query() {}
void warm_grid_query(hipStream_t st) { hipLaunchKernelGGL(k_warm_grid_query, dim3(1), dim3(64), 0, st); }

}  // namespace m2s
