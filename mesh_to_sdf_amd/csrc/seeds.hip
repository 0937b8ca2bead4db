// seeds.hip — the seed lattices of a distance call (gfx950): jump flooding over triangle centroids, for the packet bricks of a grid
// slab (launch_grid_seeds) and for the lattice over a query set's bounding box (launch_query_seeds).  A walk starts from its seed.
#include "common.h"
#include "geo.hip.h"
#include "dist.hip.h"

namespace m2s {

namespace {

// ---- jump-flooding seed pass ------------------------------------------------------------------
// Seeds only have to be GOOD, never exact (they bound the first prune, nothing else), so the seed
// lattice (one point per 4^3 brick) is filled by jump flooding (Rong & Tan 2006) over triangle
// CENTROIDS instead of a second exact tree walk: fully data parallel, cost proportional to the
// lattice (no long-running waves), ~10 ops per candidate.  k_jfa_splat drops every triangle into
// the lattice cell of its centroid (clamped, so triangles outside an x-slab still enter at the
// border); each k_jfa_pass lets a cell adopt the best candidate of its 26 neighbours at +-step.
__device__ __forceinline__ f3 lattice_point(const GridParams& g, uint32_t x, uint32_t y, uint32_t z) {
  // x is numbered along the virtual slab (interleaved chunks laid end to end); g.xb of a lattice is 0
  return {cell_center(g.first[0], g.size[0], slab_x(g, x)), cell_center(g.first[1], g.size[1], y), cell_center(g.first[2], g.size[2], z)};
}
// Lattice index along x (virtual numbering) of the point nearest to real position index `ir` (lattice units from the
// slab's first point): inside another rank's chunks it is the nearer end of the neighbouring own chunk.
__device__ __forceinline__ uint32_t lattice_x_from_real(const GridParams& g, float fr) {
  if (g.chunk_log >= 31u) return min((uint32_t)fminf(fmaxf(fr, 0.0f), (float)(g.n[0] - 1u)), g.n[0] - 1u);
  const float C = (float)(1u << g.chunk_log), P = (float)g.period;
  fr = fmaxf(fr, 0.0f);
  float j = floorf(fr / P), o = fr - j * P;                         // period, offset inside it
  if (o >= C) {                                                      // between two own chunks
    if (o - C < P - o) o = C - 1.0f;                                 // nearer to the end of chunk j
    else { j += 1.0f; o = 0.0f; }                                    // nearer to the start of chunk j + 1
  }
  const float v = j * C + o;
  return min((uint32_t)fminf(v, (float)(g.n[0] - 1u)), g.n[0] - 1u);
}

// `gp` (device pointer) overrides `g0` when the lattice is only known on the device (generic queries).
__global__ __launch_bounds__(256) void k_jfa_splat(DeviceMesh mesh, GridParams g0, const GridParams* __restrict__ gp,
                                                   unsigned long long* __restrict__ keys) {
  const GridParams g = gp ? *gp : g0;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= mesh.n_tris) return;
  const float4 c = mesh.cen[t];
  const float cc[3] = {c.x, c.y, c.z};
  uint32_t cell[3];
  for (int k = 0; k < 3; ++k) {
    float f = (cc[k] - g.first[k]) / g.size[k] + 0.5f;
    if (!(f == f)) return;                                   // NaN centroid: not a useful seed
    if (k == 0) { cell[0] = lattice_x_from_real(g, f); continue; }
    f = fminf(fmaxf(f, 0.0f), (float)(g.n[k] - 1));
    cell[k] = min((uint32_t)f, g.n[k] - 1);
  }
  // several triangles land in one cell (all those clamped onto a border cell in particular): keep the one
  // whose centroid is nearest to the cell centre — 64-bit min over (distance bits, slot)
  const f3 p = lattice_point(g, cell[0], cell[1], cell[2]);
  const float ex = p.x - c.x, ey = p.y - c.y, ez = p.z - c.z;
  const float d2 = __builtin_fmaf(ex, ex, __builtin_fmaf(ey, ey, ez * ez));
  if (!(d2 == d2)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | t;
  atomicMin(&keys[((size_t)cell[0] * g.n[1] + cell[1]) * g.n[2] + cell[2]], key);
}

// The lattice carries the candidate's centroid beside its id (xyz, id bits in w): a pass then reads 27 neighbouring 16-byte
// records — structured, cache-friendly reads — instead of 27 ids plus a dependent random gather of each candidate's centroid.
__global__ __launch_bounds__(256) void k_jfa_load(DeviceMesh mesh, const unsigned long long* __restrict__ keys, size_t n,
                                                  float4* __restrict__ lat) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t id = (uint32_t)(keys[i] & 0xffffffffull);    // untouched cells hold ~0: id 0xffffffff = none
  float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (id != 0xffffffffu) c = mesh.cen[id];
  c.w = __uint_as_float(id);
  lat[i] = c;
}

__global__ __launch_bounds__(256) void k_jfa_pass(GridParams g0, const GridParams* __restrict__ gp, const float4* __restrict__ in,
                                                  float4* __restrict__ out, int step, uint32_t* __restrict__ ids_out) {
  const GridParams g = gp ? *gp : g0;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)g.n[0] * g.n[1] * g.n[2];
  if (i >= total) return;
  const int z = (int)(i % g.n[2]), y = (int)((i / g.n[2]) % g.n[1]), x = (int)(i / ((size_t)g.n[2] * g.n[1]));
  const f3 p = lattice_point(g, (uint32_t)x, (uint32_t)y, (uint32_t)z);
  uint32_t best = 0xffffffffu;
  float4 bc = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xffffffffu));
  float bd = __builtin_inff();
  // Nine records per x-plane are requested TOGETHER (clamped addresses, validity as a flag) and only then compared.  Written with a
  // `continue` per out-of-range or empty neighbour the loop was a chain of 27 dependent memory round trips per point — 56 us per pass of
  // the 512^3 call's lattice, 400 us for 1024^3, whatever the cache hit rate (an LDS-tiled form was no faster for the same reason).
  const int n0 = (int)g.n[0], n1 = (int)g.n[1], n2 = (int)g.n[2];
#pragma unroll
  for (int dx = -1; dx <= 1; ++dx) {
    const int xx = x + dx * step;
    const bool okx = xx >= 0 && xx < n0;
    const size_t xbase = (size_t)min(max(xx, 0), n0 - 1) * (size_t)n1;
    float4 c[9];
    bool ok[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int yy = y + (k / 3 - 1) * step, zz = z + (k % 3 - 1) * step;
      ok[k] = okx && yy >= 0 && yy < n1 && zz >= 0 && zz < n2;
      c[k] = in[(xbase + (size_t)min(max(yy, 0), n1 - 1)) * (size_t)n2 + (size_t)min(max(zz, 0), n2 - 1)];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const uint32_t cand = __float_as_uint(c[k].w);
      const float ex = p.x - c[k].x, ey = p.y - c[k].y, ez = p.z - c[k].z;
      const float d = __builtin_fmaf(ex, ex, __builtin_fmaf(ey, ey, ez * ez));
      const bool take = ok[k] && cand != 0xffffffffu && (d < bd || (d == bd && cand < best));
      bd = take ? d : bd;
      best = take ? cand : best;
      bc.x = take ? c[k].x : bc.x;
      bc.y = take ? c[k].y : bc.y;
      bc.z = take ? c[k].z : bc.z;
      bc.w = take ? c[k].w : bc.w;
    }
  }
  out[i] = bc;
  if (ids_out) ids_out[i] = best;
}

// The pass for lattices of fewer than 2^31 points, written for the VALU: the kernel above spends ~900 vector instructions per point —
// 64-bit index arithmetic per neighbour, three compares and six selects per candidate — and is bound by exactly that (an LDS-tiled form
// and one with all 27 loads in flight took the same 56 us per pass of the 512^3 call's lattice, 390 us for 1024^3).  Here a neighbour's
// index is the point's own 32-bit index plus a wave-uniform offset, (distance bits, id) is one 64-bit key so that "nearer, or as near
// with the smaller id" is one unsigned compare, only the key and the neighbour's number are carried (the winner's record is fetched
// again at the end), and out-of-range neighbours are bits of a precomputed mask.  Same candidates, same tie rule: the same seeds.
__global__ __launch_bounds__(256) void k_jfa_pass32(GridParams g, const float4* __restrict__ in, float4* __restrict__ out, int step,
                                                    uint32_t* __restrict__ ids_out) {
  const uint32_t n0 = g.n[0], n1 = g.n[1], n2 = g.n[2];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n0 * n1 * n2) return;
  const uint32_t z = i % n2, xy = i / n2, y = xy % n1, x = xy / n1;
  const f3 p = lattice_point(g, x, y, z);
  const uint32_t s = (uint32_t)step;
  // bit (3 a + b) of m[axis]... one flag per axis and direction: is the neighbour at -step / 0 / +step inside the lattice?
  const bool okx[3] = {x >= s, true, x + s < n0}, oky[3] = {y >= s, true, y + s < n1}, okz[3] = {z >= s, true, z + s < n2};
  const int sx = (int)(s * n1 * n2), sy = (int)(s * n2), sz = (int)s;
  unsigned long long key = 0x7f800000ffffffffull;             // (+inf, no triangle)
  uint32_t kbest = 13u;                                      // the point itself
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float4 c[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const bool ok = okx[a] && oky[k / 3] && okz[k % 3];
      const int off = (a - 1) * sx + (k / 3 - 1) * sy + (k % 3 - 1) * sz;
      c[k] = in[ok ? (uint32_t)((int)i + off) : i];            // an out-of-range neighbour reads the point's own record and is masked below
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const bool ok = okx[a] && oky[k / 3] && okz[k % 3];
      const uint32_t cand = __float_as_uint(c[k].w);
      const float ex = p.x - c[k].x, ey = p.y - c[k].y, ez = p.z - c[k].z;
      const float d = __builtin_fmaf(ex, ex, __builtin_fmaf(ey, ey, ez * ez));
      // d >= +0 orders like its bit pattern; NaN (bits above +inf's) never wins, as `d < bd || d == bd` never held for it
      const unsigned long long kk = ((unsigned long long)__float_as_uint(d) << 32) | cand;
      const bool take = ok && cand != 0xffffffffu && kk < key;
      key = take ? kk : key;
      kbest = take ? (uint32_t)(9 * a + k) : kbest;
    }
  }
  const uint32_t best = (uint32_t)key;
  float4 bc = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xffffffffu));
  if (best != 0xffffffffu) {
    const int a = (int)(kbest / 9u), k = (int)(kbest % 9u);
    bc = in[(uint32_t)((int)i + (a - 1) * sx + (k / 3 - 1) * sy + (k % 3 - 1) * sz)];
  }
  out[i] = bc;
  if (ids_out) ids_out[i] = best;
}
// Lattices of at most JFA_SMALL_MAX points (a 64^3 grid: 16^3 brick centres): the whole flood — clear, splat, load, every pass — in ONE
// workgroup with the lattice in LDS.  Seven to nine launches of 2 - 4 us kernels cost the host ~45 us to enqueue, during which the caller's
// stream sat idle behind the build's sort (suzanne, 968 triangles, 64^3: hierarchy started 55 us after the sort had ended; timeline in
// profiles/r06_small_calls.txt).  Same candidates, same tie rule as k_jfa_splat / k_jfa_pass32: the same seeds.
constexpr uint32_t JFA_SMALL_MAX = 4096, JFA_SMALL_THREADS = 1024;
__global__ __launch_bounds__(JFA_SMALL_THREADS) void k_jfa_small(DeviceMesh mesh, GridParams g, uint32_t* __restrict__ ids_out) {
  __shared__ float4 lat_a[JFA_SMALL_MAX], lat_b[JFA_SMALL_MAX];
  unsigned long long* const keys = reinterpret_cast<unsigned long long*>(lat_b);   // the splat's keys live in the second buffer until the load
  const uint32_t n0 = g.n[0], n1 = g.n[1], n2 = g.n[2], n = n0 * n1 * n2, tid = threadIdx.x;
  for (uint32_t i = tid; i < n; i += JFA_SMALL_THREADS) keys[i] = ~0ull;
  __syncthreads();
  for (uint32_t t = tid; t < mesh.n_tris; t += JFA_SMALL_THREADS) {          // k_jfa_splat
    const float4 c = mesh.cen[t];
    const float cc[3] = {c.x, c.y, c.z};
    uint32_t cell[3];
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
      float f = (cc[k] - g.first[k]) / g.size[k] + 0.5f;
      if (!(f == f)) { ok = false; break; }                                  // NaN centroid: not a useful seed
      if (k == 0) { cell[0] = lattice_x_from_real(g, f); continue; }
      f = fminf(fmaxf(f, 0.0f), (float)(g.n[k] - 1));
      cell[k] = min((uint32_t)f, g.n[k] - 1);
    }
    if (!ok) continue;
    const f3 p = lattice_point(g, cell[0], cell[1], cell[2]);
    const float ex = p.x - c.x, ey = p.y - c.y, ez = p.z - c.z;
    const float d2 = __builtin_fmaf(ex, ex, __builtin_fmaf(ey, ey, ez * ez));
    if (!(d2 == d2)) continue;
    atomicMin(&keys[(cell[0] * n1 + cell[1]) * n2 + cell[2]], ((unsigned long long)__float_as_uint(d2) << 32) | t);
  }
  __syncthreads();
  for (uint32_t i = tid; i < n; i += JFA_SMALL_THREADS) {                    // k_jfa_load
    const uint32_t id = (uint32_t)(keys[i] & 0xffffffffull);
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (id != 0xffffffffu) c = mesh.cen[id];
    c.w = __uint_as_float(id);
    lat_a[i] = c;
  }
  __syncthreads();
  const uint32_t maxdim = max(n0, max(n1, n2));
  uint32_t step = 1;
  while (step * 2u < maxdim) step *= 2u;
  float4* in = lat_a;
  float4* out = lat_b;
  for (bool last = false;; ) {                                                // steps ... 2, 1, then one more unit pass (launch_grid_seeds)
    for (uint32_t i = tid; i < n; i += JFA_SMALL_THREADS) {                  // k_jfa_pass32
      const uint32_t z = i % n2, xy = i / n2, y = xy % n1, x = xy / n1;
      const f3 p = lattice_point(g, x, y, z);
      const bool okx[3] = {x >= step, true, x + step < n0}, oky[3] = {y >= step, true, y + step < n1}, okz[3] = {z >= step, true, z + step < n2};
      const int sx = (int)(step * n1 * n2), sy = (int)(step * n2), sz = (int)step;
      unsigned long long key = 0x7f800000ffffffffull;
      float4 bc = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xffffffffu));
      for (int a = 0; a < 3; ++a)
        for (int k = 0; k < 9; ++k) {
          if (!(okx[a] && oky[k / 3] && okz[k % 3])) continue;
          const float4 c = in[(uint32_t)((int)i + (a - 1) * sx + (k / 3 - 1) * sy + (k % 3 - 1) * sz)];
          const uint32_t cand = __float_as_uint(c.w);
          const float ex = p.x - c.x, ey = p.y - c.y, ez = p.z - c.z;
          const float d = __builtin_fmaf(ex, ex, __builtin_fmaf(ey, ey, ez * ez));
          const unsigned long long kk = ((unsigned long long)__float_as_uint(d) << 32) | cand;
          if (cand != 0xffffffffu && kk < key) { key = kk; bc = c; }
        }
      out[i] = bc;
      if (last) ids_out[i] = (uint32_t)key;
    }
    __syncthreads();
    float4* t = in; in = out; out = t;
    if (last) break;
    if (step == 1u) last = true; else step >>= 1;
  }
}
// One flooding pass over the lattice g.
static void launch_jfa_pass(hipStream_t st, const GridParams& g, const float4* in, float4* out, int step, uint32_t* ids) {
  const size_t total = (size_t)g.n[0] * g.n[1] * g.n[2];
  const unsigned nb = (unsigned)((total + 255) / 256);
  if (total < (1ull << 30) && (unsigned long long)step * g.n[1] * g.n[2] < (1ull << 30))
    hipLaunchKernelGGL(k_jfa_pass32, dim3(nb), dim3(256), 0, st, g, in, out, step, ids);
  else
    hipLaunchKernelGGL(k_jfa_pass, dim3(nb), dim3(256), 0, st, g, (const GridParams*)nullptr, in, out, step, ids);
}

}  // namespace

// Coarse lattice whose points sit at the centres of the `stride`-sized blocks of `fine`.
static GridParams coarse_level(const GridParams& fine, const uint32_t log2_stride[3], uint32_t x_origin) {
  GridParams c = fine;
  for (int k = 0; k < 3; ++k) {
    const uint32_t span = k == 0 ? fine.xe - fine.xb : fine.n[k];
    const uint32_t stride = 1u << log2_stride[k];
    c.n[k] = (span + stride - 1) / stride;
    c.first[k] = fine.first[k] + ((float)(k == 0 ? x_origin : 0u) + 0.5f * (float)(stride - 1u)) * fine.size[k];   // brick centre
    c.size[k] = (float)stride * fine.size[k];
  }
  c.xb = 0;
  c.xe = c.n[0];
  c.out_off = 0;
  if (fine.chunk_log < 31u) {           // interleaved slab: chunk and period in lattice points (whole numbers: capi.hip checks)
    c.chunk_log = fine.chunk_log - log2_stride[0];
    c.period = fine.period >> log2_stride[0];
  }
  return c;
}

__global__ __launch_bounds__(256) void k_seed_remap(uint32_t* __restrict__ ids, size_t n, const uint32_t* __restrict__ slot_of, uint32_t n_tris) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t t = ids[i];
  ids[i] = t < n_tris ? slot_of[t] : 0xffffffffu;
}
// Translates seed ids that name input triangles (a lattice computed while the mesh was being built) to sorted slots.
void launch_seed_remap(hipStream_t st, uint32_t* ids, size_t n, const uint32_t* slot_of, uint32_t n_tris) {
  hipLaunchKernelGGL(k_seed_remap, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ids, n, slot_of, n_tris);
}

// Seeding: every 4^3 brick starts its walk from a triangle near its own centre (jump flooding over the lattice of brick
// centres); that halves the nodes visited compared with a greedy descent.  `cen` are the triangle centroids the ids of
// the result refer to: the sorted array of the finished mesh, or the input-order array while the mesh is still being built.
int launch_grid_seeds(Arena& ws, hipStream_t st, const float4* cen, uint32_t n_tris, const GridParams& g, SeedLattice* out) {
  DeviceMesh mesh{};
  mesh.cen = cen;
  mesh.n_tris = n_tris;
  // one lattice point per packet brick, at its centre (one per 2 x 2 x 2 bricks — shift 1 — costs the headline walk 8.11 -> 9.23 ms)
  constexpr uint32_t seed_shift = 0u;
  const uint32_t stride_log[3] = {g.bl[0] + seed_shift, g.bl[1] + seed_shift, g.bl[2] + seed_shift};
  const GridParams g1 = coarse_level(g, stride_log, g.xb);
  const size_t points1 = (size_t)g1.n[0] * g1.n[1] * g1.n[2];
  uint32_t* ids = ws.take<uint32_t>(points1);
  float4* la = ws.take<float4>(points1);
  float4* lb = ws.take<float4>(points1);
  unsigned long long* keys = ws.take<unsigned long long>(points1);
  if (!ids || !la || !lb || !keys) { set_error("internal: seed workspace too small"); return M2S_ERR_HIP_INTERNAL; }
  const unsigned nb1 = (unsigned)((points1 + 255) / 256);
  if (points1 <= JFA_SMALL_MAX) {                               // the whole flood in one workgroup
    hipLaunchKernelGGL(k_jfa_small, dim3(1), dim3(JFA_SMALL_THREADS), 0, st, mesh, g1, ids);
  } else {
    M2S_HIP_CHECK(hipMemsetAsync(keys, 0xff, points1 * 8, st));
    hipLaunchKernelGGL(k_jfa_splat, dim3((mesh.n_tris + 255) / 256), dim3(256), 0, st, mesh, g1, nullptr, keys);
    // (Round 6, measured and not kept: the flood's long steps on a lattice of half the resolution + a refinement pass — the seeds get worse by
    // a few hundredths of a cell far from the surface, where a packet's candidate set grows with the square root of exactly that: the
    // headline walk 6.44 -> 7.00 ms with every step but the last two at half resolution, 6.76 -> 7.16 with only the steps >= 16 there;
    // profiles/r06_seed_coarse_*.txt.  A bound from the lanes' FINAL minima would take 1.5 % of the node tests, 12 % of the pre-tests and
    // 18 % of the exact evaluations: profiles/r06_stats2_headline.txt.)
    const uint32_t maxdim = max(g1.n[0], max(g1.n[1], g1.n[2]));
    hipLaunchKernelGGL(k_jfa_load, dim3(nb1), dim3(256), 0, st, mesh, keys, points1, la);
    int step = 1;
    while ((uint32_t)step * 2 < maxdim) step *= 2;
    float4 *src = la, *dst = lb;
    for (; step >= 1; step /= 2) {
      launch_jfa_pass(st, g1, src, dst, step, nullptr);
      float4* t = src; src = dst; dst = t;
    }
    launch_jfa_pass(st, g1, src, dst, 1, ids);   // "JFA+1": one more unit pass; leaves the ids
  }
  out->ids = ids;
  out->ny = g1.n[1];
  out->nz = g1.n[2];
  out->points = points1;
  out->shift = seed_shift;
  return 0;
}

// Seed lattice of a query set: jump flooding over the QL^3 cells of plan.lat from the centroids `cen` (the sorted array of the finished
// mesh, or the input-order array while the mesh is being built: `ids` then name input triangles and launch_query_walk translates them).
int launch_query_seeds(Arena& ws, hipStream_t st, const float4* cen, uint32_t n_tris, const QueryPlan& plan, bool raw, QuerySeeds* out) {
  *out = QuerySeeds{};
  if (!plan.seeds || plan.lat == nullptr || n_tris == 0) return 0;
  DeviceMesh mesh{};
  mesh.cen = cen;
  mesh.n_tris = n_tris;
  GridParams g{};
  const size_t cells = (size_t)QL * QL * QL;
  unsigned long long* k64 = ws.take<unsigned long long>(cells);
  uint32_t* ids = ws.take<uint32_t>(cells);
  float4* la = ws.take<float4>(cells);
  float4* lb = ws.take<float4>(cells);
  if (!k64 || !ids || !la || !lb) { set_error("internal: query workspace too small"); return M2S_ERR_HIP_INTERNAL; }
  const GridParams* lat = plan.lat;
  M2S_HIP_CHECK(hipMemsetAsync(k64, 0xff, cells * 8, st));
  hipLaunchKernelGGL(k_jfa_splat, dim3((n_tris + 255) / 256), dim3(256), 0, st, mesh, g, lat, k64);
  const unsigned nbl = (unsigned)((cells + 255) / 256);
  hipLaunchKernelGGL(k_jfa_load, dim3(nbl), dim3(256), 0, st, mesh, k64, cells, la);
  float4 *src = la, *dst = lb;
  for (int step = QL / 2; step >= 1; step /= 2) {
    hipLaunchKernelGGL(k_jfa_pass, dim3(nbl), dim3(256), 0, st, g, lat, src, dst, step, nullptr);
    float4* t = src; src = dst; dst = t;
  }
  hipLaunchKernelGGL(k_jfa_pass, dim3(nbl), dim3(256), 0, st, g, lat, src, dst, 1, ids);
  M2S_HIP_CHECK(hipGetLastError());
  out->ids = ids;
  out->raw = raw;
  return 0;
}

// m2s_warmup: this unit's code object, and the kernel functions of it that a first call uses (see warm_distance).
__global__ void k_warm_seeds() {}
void warm_seeds(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_seeds, dim3(1), dim3(64), 0, st);
  const void* fns[] = {
      (const void*)k_jfa_splat,
      (const void*)k_jfa_load,
      (const void*)k_jfa_pass32,
      (const void*)k_seed_remap};
  hipFuncAttributes attr;
  for (const void* f : fns) (void)hipFuncGetAttributes(&attr, f);
  (void)hipGetLastError();
}

}  // namespace m2s
