// band_measure.hip — m2s_band_measure: area, enclosed volume, first moments and the counts of the level set d = iso of a resident band, per
// group of cells, gfx950.  The surface is the mesh m2s_band_isosurface would extract, but no mesh is built: nothing is sized by the grid,
// by the band or by the triangle count; the workspace is one record of nine 64-bit sums per group.  The contract is include/m2s.h's (every
// integer field to the bit); tests/band_measure_model.py restates it in numpy.
//
// One pass, k_measure, over band_walk.hip.h's units: a wave takes units of mask words (every 4096th, at most) in steps of 64 words, lane l
// loading word 64 * step + l and decomposing its base into (i, j, k).  The active points of a step are then taken in list order 64 at a time,
// one per lane: a prefix sum of the words' popcounts, a binary search along the wave for a point's word (six shuffles) and for its bit
// (six popcounts).  Taking the words one at a time with lane t owning bit t, as the other walks do, was built first and measured 2.5 times
// slower at 256^3: a band's row crosses a word with a dozen cells, so most lanes idled through the corner look-ups.
// A wave keeps its sums across the units it takes; flushing them at the end of every unit cost half the time at 2048^3.
//   corners    the 7 other corners of the point's cell by mask word, word_off and popcount (as band_isosurface.hip's k_biso_info); the +k
//              neighbour of a corner already found is the next list place, and its mask bit is in the word already loaded unless the
//              corner is the word's last bit.
//   counts     from the 8 values: the case, the point's three edge flags (its vertices, and those on a boundary face of the grid), whether
//              its cell is cut but incomplete.
//   triangles  of a complete cell: the twelve t = (iso - d0) / (d1 - d0) go to the lane's column of a table in LDS, which the triangle loop
//              indexes by the case table's edge numbers (a register array indexed at run time would live in scratch).  Per triangle the
//              float32 area weight (sample.hip.h's tri_weight_area, an integer at a power-of-two scale) and the float64 volume and moment
//              terms, each rounded to an integer before it is added: the sums are the same bits in any order of execution.
//   sums       a lane keeps its partial sums while the words the wave takes carry one group; when the group changes or the unit ends the
//              wave reduces them and lane 0 adds them to the group's record by at most nine 64-bit atomics.  64 points that carry
//              several groups are added by their lanes one by one, as a word with several labels is in band_components.hip's k_cc_label.
// A lane's counts fit 32 bits: a wave takes at most 2^22 / 4096 units, a unit gives a lane at most kWalkUnit points, a point at most 5
// triangles and 3 vertices.
// All arithmetic of the definition is add, subtract, multiply, one float32 divide per edge and one float32 sqrt per triangle, not fused.
#include "../../include/m2s.h"
#include "band_handle.h"
#include "band_walk.hip.h"
#include "capi_internal.h"
#include "common.h"
#include "isosurface.hip.h"
#include "sample.hip.h"

#include <cmath>
#include <cstring>
#include <new>

#pragma clang fp contract(off)

namespace m2s {
namespace {

constexpr int kMsSums = 9;   // a group's record: n_triangles, n_vertices, n_open, n_border, area_q, volume_q, moment_q[3]
constexpr uint32_t kMsNoGroup = 0xffffffffu;
constexpr uint64_t kMsMaxBlocks = 1024;   // 4096 waves share the units: every wave's last flush is nine atomics on a few records

struct MsArgs {
  float cs[3];
  float iso;
  double area_scale;   // 2^(24 - E)
  uint64_t n_groups;   // at most 2^32 - 1
};

struct MsAcc {
  uint32_t nt, nv, no, nb;
  uint64_t area, vol, mom[3];   // vol and mom are signed sums: two's complement adds
  __device__ __forceinline__ void reset() {
    nt = nv = no = nb = 0;
    area = vol = mom[0] = mom[1] = mom[2] = 0;
  }
};

__device__ __forceinline__ void ms_add(uint64_t* p, uint64_t v) {
  if (v) atomicAdd((unsigned long long*)p, (unsigned long long)v);
}
__device__ __forceinline__ void ms_publish(uint64_t* rec, const MsAcc& s) {
  ms_add(rec + 0, s.nt);
  ms_add(rec + 1, s.nv);
  ms_add(rec + 2, s.no);
  ms_add(rec + 3, s.nb);
  ms_add(rec + 4, s.area);
  ms_add(rec + 5, s.vol);
  ms_add(rec + 6, s.mom[0]);
  ms_add(rec + 7, s.mom[1]);
  ms_add(rec + 8, s.mom[2]);
}
// Every lane takes part.  cur: wave-uniform.
__device__ __forceinline__ void ms_flush(uint64_t* sums, uint32_t cur, MsAcc& s, int lane) {
  if (cur != kMsNoGroup) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s.nt += __shfl_xor(s.nt, o, 64);
      s.nv += __shfl_xor(s.nv, o, 64);
      s.no += __shfl_xor(s.no, o, 64);
      s.nb += __shfl_xor(s.nb, o, 64);
      s.area += __shfl_xor(s.area, o, 64);
      s.vol += __shfl_xor(s.vol, o, 64);
#pragma unroll
      for (int c = 0; c < 3; ++c) s.mom[c] += __shfl_xor(s.mom[c], o, 64);
    }
    if (lane == 0) ms_publish(sums + (uint64_t)cur * kMsSums, s);
  }
  s.reset();
}

// Round to nearest even; a term that is not finite counts as 0 (no grid within the call's limits gives a finite one at or above 2^62).
__device__ __forceinline__ uint64_t ms_llrint(double x) { return fabs(x) < 0x1p62 ? (uint64_t)__double2ll_rn(x) : 0ull; }

// The lower corner c0 of local edge e = 4 a + r, by isosurface_table.h's rule: the offsets on the two other axes are (r >> 1, r & 1).
__host__ __device__ constexpr int ms_edge_corner(int e) {
  return (e >> 2) == 0 ? 2 * ((e & 3) >> 1) + (e & 1) : ((e >> 2) == 1 ? 4 * ((e & 3) >> 1) + (e & 1) : 4 * ((e & 3) >> 1) + 2 * (e & 1));
}

// What the active point L = (i, j, k) at list place r adds to its group: its vertices, its cell's openness and its cell's triangles.
// mw0: the mask word of L.  tcol: this lane's column of the t table, the entries kWalkThreads floats apart.
__device__ __forceinline__ void ms_point(const BandDev& X, const WalkGrid& g, const MsArgs& a, const WalkIjk& p, uint64_t L, uint64_t r, uint64_t mw0,
                                         float* tcol, MsAcc& o) {
  const bool ex = p.i + 1 < g.nx, ey = p.j + 1 < g.ny, ez = p.k + 1 < g.nz;
  const bool cell = ex && ey && ez;
  // corner c = 4 dx + 2 dy + dz, as in the case; corners 3, 5, 6, 7 matter to a cell only
  const bool exists[8] = {true, ez, ey, cell, ex, cell, cell, cell};
  float d[8];
  uint32_t have = 0;
#pragma unroll
  for (int c = 0; c < 8; c += 2) {
    const uint64_t Lc = L + (c & 4 ? g.si : 0) + (c & 2 ? g.sj : 0);   // inside the grid where exists[c]
    const uint64_t w = Lc >> 6;
    const int b = (int)(Lc & 63);
    uint64_t mw = 0, rc = kNone;
    d[c] = d[c + 1] = 0.0f;
    if (c == 0) {
      mw = mw0;
      rc = r;
    } else if (exists[c]) {
      mw = X.mask[w];
      if ((mw >> b) & 1ull) {
        rc = X.word_off[w] + (uint64_t)__popcll(mw & walk_below(b));
        if (rc >= X.n) rc = kNone;   // never, when the index is sound
      }
    }
    if (rc != kNone) {
      have |= 1u << c;
      d[c] = X.dist[rc];
    }
    if (exists[c + 1]) {   // Lc + 1 is in the same row: the next list place after Lc's, if Lc is active
      const bool on = b < 63 ? ((mw >> (b + 1)) & 1ull) != 0 : (X.mask[w + 1] & 1ull) != 0;
      if (on) {
        uint64_t r1;
        if (rc != kNone) r1 = rc + 1;
        else if (b < 63) r1 = X.word_off[w] + (uint64_t)__popcll(mw & walk_below(b + 1));
        else r1 = X.word_off[w + 1];
        if (r1 < X.n) {
          have |= 1u << (c + 1);
          d[c + 1] = X.dist[r1];
        }
      }
    }
  }
  const float iso = a.iso;
  uint32_t in = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) in |= (uint32_t)(((have >> c) & 1u) && d[c] < iso) << c;
  const uint32_t i000 = in & 1u;
  const bool fx = ((have >> 4) & 1u) && ((in >> 4) & 1u) != i000, fy = ((have >> 2) & 1u) && ((in >> 2) & 1u) != i000,
             fz = ((have >> 1) & 1u) && ((in >> 1) & 1u) != i000;
  const bool bx = p.i == 0 || p.i + 1 == g.nx, by = p.j == 0 || p.j + 1 == g.ny, bz = p.k == 0 || p.k + 1 == g.nz;
  o.nv += (uint32_t)fx + (uint32_t)fy + (uint32_t)fz;
  o.nb += (uint32_t)(fx && (by || bz)) + (uint32_t)(fy && (bx || bz)) + (uint32_t)(fz && (bx || by));
  if (cell && have != 255u && in != 0u && in != have) ++o.no;
  if (have != 255u || in == 0u || in == 255u) return;

#pragma unroll
  for (int e = 0; e < 12; ++e) {
    constexpr int kFar[3] = {4, 2, 1};
    const int c0 = ms_edge_corner(e), c1 = c0 + kFar[e >> 2];   // decided when compiled: d stays in registers
    tcol[e * kWalkThreads] = (iso - d[c0]) / (d[c1] - d[c0]);   // used only where the edge crosses
  }
  const int count = kIsoTriCount[in];
  o.nt += (uint32_t)count;
  // an axis of the grid has fewer than 2^25 points (the moment limit): the low words are the index
  const double bi = (double)(uint32_t)p.i, bj = (double)(uint32_t)p.j, bk = (double)(uint32_t)p.k;
  for (int tri = 0; tri < count; ++tri) {
    float u[3][3];
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      const int e = kIsoTris[in][tri * 3 + v] & 15;
      const int ax = e >> 2, hi = (e >> 1) & 1, lo = e & 1;
      const float t = tcol[(e < 12 ? e : 0) * kWalkThreads];
      u[v][0] = ax == 0 ? t : (float)hi;
      u[v][1] = ax == 1 ? t : (float)(ax == 0 ? hi : lo);
      u[v][2] = ax == 2 ? t : (float)lo;
    }
    f3 n32;
    const float A2 = tri_weight_area(mk3(u[0][0] * a.cs[0], u[0][1] * a.cs[1], u[0][2] * a.cs[2]), mk3(u[1][0] * a.cs[0], u[1][1] * a.cs[1], u[1][2] * a.cs[2]),
                                     mk3(u[2][0] * a.cs[0], u[2][1] * a.cs[1], u[2][2] * a.cs[2]), &n32);
    o.area += (uint64_t)((double)A2 * a.area_scale);   // A2 >= 0 and finite: the conversion is the floor
    const double x0 = bi + (double)u[0][0], y0 = bj + (double)u[0][1], z0 = bk + (double)u[0][2];
    const double x1 = bi + (double)u[1][0], y1 = bj + (double)u[1][1], z1 = bk + (double)u[1][2];
    const double x2 = bi + (double)u[2][0], y2 = bj + (double)u[2][1], z2 = bk + (double)u[2][2];
    const double ax_ = x1 - x0, ay_ = y1 - y0, az_ = z1 - z0, bx_ = x2 - x0, by_ = y2 - y0, bz_ = z2 - z0;
    const double nx = ay_ * bz_ - az_ * by_, ny = az_ * bx_ - ax_ * bz_, nz = ax_ * by_ - ay_ * bx_;
    const double sz = (z0 + z1) + z2;
    o.vol += ms_llrint((nz * sz) * 0x1p20);
    const double sx2 = ((x0 * x0 + x1 * x1) + x2 * x2) + ((x0 * x1 + x1 * x2) + x2 * x0);
    const double sy2 = ((y0 * y0 + y1 * y1) + y2 * y2) + ((y0 * y1 + y1 * y2) + y2 * y0);
    const double sz2 = ((z0 * z0 + z1 * z1) + z2 * z2) + ((z0 * z1 + z1 * z2) + z2 * z0);
    o.mom[0] += ms_llrint((nx * sx2) * 0x1p8);
    o.mom[1] += ms_llrint((ny * sy2) * 0x1p8);
    o.mom[2] += ms_llrint((nz * sz2) * 0x1p8);
  }
}

// sums: n_groups records of kMsSums, zeroed.  labels: list order, or nullptr for one group.  *n_skipped += the places whose label is
// not below n_groups.
__global__ void __launch_bounds__(kWalkThreads) k_measure(BandDev X, WalkGrid g, uint64_t n_units, MsArgs a, const uint32_t* __restrict__ labels,
                                                        uint64_t* __restrict__ sums, uint64_t* __restrict__ n_skipped) {
  __shared__ float s_t[12 * kWalkThreads];
  const int lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * kWalkWaves + (uint64_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t n_waves = (uint64_t)gridDim.x * kWalkWaves;
  float* tcol = s_t + threadIdx.x;
  uint32_t cur = kMsNoGroup, skipped = 0;
  MsAcc acc;
  acc.reset();
  // a wave takes every n_waves-th unit and keeps its sums across them: the records are few, and every flush is nine atomics on one of them
  for (uint64_t unit = wave; unit < n_units; unit += n_waves) {   // wave-uniform
    const uint64_t w0 = unit * kWalkUnit;
    for (int step = 0; step < kWalkSteps; ++step) {
      WALK_STEP_HEAD(g.n_words)
      const uint64_t m = in_range ? X.mask[w] : 0;
      const uint64_t wo = m ? X.word_off[w] : 0;
      WalkIjk base{0, 0, 0};
      if (m) base = walk_base(w << 6, g);
      // the step's active points in list order, 64 at a time: point q of the step is the (q - before[j])-th bit of word j
      const uint32_t cnt = (uint32_t)__popcll(m);
      uint32_t before = cnt;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(before, o, 64);
        if (lane >= o) before += y;
      }
      const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)before, 63);   // at most 4096
      before -= cnt;
      for (uint32_t q0 = 0; q0 < total; q0 += 64) {   // wave-uniform
        const uint32_t q = q0 + (uint32_t)lane;
        int j = 0;   // the last word whose points begin at or before q: words without points share their successor's `before`
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const uint32_t e = __shfl(before, j + o, 64);
          if (e <= q) j += o;
        }
        const uint64_t mj = __shfl(m, j, 64), woj = __shfl(wo, j, 64);
        const WalkIjk bj{__shfl(base.i, j, 64), __shfl(base.j, j, 64), __shfl(base.k, j, 64)};
        uint32_t nth = q - __shfl(before, j, 64);
        bool act = q < total && nth < (uint32_t)__popcll(mj);
        const uint64_t r = woj + nth;
        act = act && r < X.n;   // always, when the index is sound
        int t = 0;   // the nth set bit of mj
        uint64_t rest = mj;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const uint32_t c = (uint32_t)__popcll(rest & ((1ull << o) - 1ull));
          if (nth >= c) {
            nth -= c;
            rest >>= o;
            t += o;
          }
        }
        const WalkIjk p = walk_step(bj, (uint32_t)t, g);
        const uint64_t L = ((wb + (uint64_t)j) << 6) + (uint64_t)t;
        uint32_t lab = 0;
        if (act && labels) {
          lab = labels[r];
          if ((uint64_t)lab >= a.n_groups) {
            ++skipped;
            act = false;
          }
        }
        const uint64_t am = __ballot(act);
        if (!am) continue;
        const uint32_t lab0 = (uint32_t)__builtin_amdgcn_readlane((int)lab, __ffsll((unsigned long long)am) - 1);
        if (__ballot(act && lab != lab0) == 0) {   // one group among the 64 points: the usual case
          if (lab0 != cur) {
            ms_flush(sums, cur, acc, lane);
            cur = lab0;
          }
          if (act) ms_point(X, g, a, p, L, r, mj, tcol, acc);
        } else {   // several: each lane adds its own point
          ms_flush(sums, cur, acc, lane);
          cur = kMsNoGroup;
          if (act) {
            ms_point(X, g, a, p, L, r, mj, tcol, acc);
            ms_publish(sums + (uint64_t)lab * kMsSums, acc);
          }
          acc.reset();
        }
      }
    }
  }
  ms_flush(sums, cur, acc, lane);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) skipped += __shfl_xor(skipped, o, 64);
  if (lane == 0 && skipped) atomicAdd((unsigned long long*)n_skipped, (unsigned long long)skipped);
}

}  // namespace

// m2s_warmup: the first launch of a kernel of this translation unit makes the runtime load its code object (all its kernels).
__global__ void k_warm_band_measure() {}
void warm_band_measure(hipStream_t st) { hipLaunchKernelGGL(k_warm_band_measure, dim3(1), dim3(64), 0, st); }

}  // namespace m2s

using namespace m2s;

extern "C" {

int m2s_band_measure(const m2s_band* band, const m2s_band_measure_opts* mopts, const uint32_t* labels, uint64_t n_groups, const m2s_opts* opts,
                     m2s_band_measure_record* measures_out, m2s_band_measure_info* info_out, m2s_timings* timings) {
  clear_error();
  if (!band) return fail(M2S_ERR_BAD_ARG, "band is NULL");
  if (!measures_out) return fail(M2S_ERR_BAD_ARG, "measures_out is NULL");
  if (mopts && mopts->struct_size != sizeof(m2s_band_measure_opts))
    return fail(M2S_ERR_BAD_ARG, "m2s_band_measure_opts.struct_size is not sizeof(m2s_band_measure_opts)");
  const float iso = mopts ? mopts->iso : 0.0f;
  if (!std::isfinite(iso)) return fail(M2S_ERR_BAD_ARG, "iso = %g is not finite", (double)iso);
  if (info_out && info_out->struct_size != sizeof(m2s_band_measure_info))
    return fail(M2S_ERR_BAD_ARG, "m2s_band_measure_info.struct_size is not sizeof(m2s_band_measure_info)");
  if (labels && n_groups == 0) return fail(M2S_ERR_BAD_ARG, "labels with n_groups = 0");
  if (labels && n_groups > 0xffffffffull)
    return fail(M2S_ERR_BAD_ARG, "n_groups = %llu: labels are 32-bit and M2S_LABEL_NONE names no group", (unsigned long long)n_groups);
  int rc = band_opts_args(opts, "m2s_band_measure");
  if (rc) return rc;
  m2s_opts o;
  rc = band_call_opts(band, opts, &o);
  if (rc) return rc;
  o.synchronous = 1;
  if (timings) o.timings = timings;
  const m2s_grid& grid = band->grid;
  const uint64_t cmax = std::max(grid.cell_count[0], std::max(grid.cell_count[1], grid.cell_count[2]));
  if (cmax && band->total > (((uint64_t)1 << 50) - 1) / cmax)   // total * cmax >= 2^50
    return fail(M2S_ERR_BAD_ARG, "the grid's %llu cells times its longest axis (%llu) reach 2^50: the first moments could leave 64 bits",
                (unsigned long long)band->total, (unsigned long long)cmax);
  const uint64_t n_out = labels ? n_groups : 1;
  const float csmax = std::max(grid.cell_size[0], std::max(grid.cell_size[1], grid.cell_size[2]));
  const int E = sample_exponent(csmax * csmax);
  uint64_t* sums = new (std::nothrow) uint64_t[n_out * kMsSums + 1]();   // [n_out * kMsSums] = n_skipped
  if (!sums) return fail(M2S_ERR_BAD_ARG, "n_groups = %llu: no host memory for the records", (unsigned long long)n_out);
  auto done = [&](int code) {
    delete[] sums;
    return code;
  };
  const uint64_t n = band->n;
  float ms = 0.0f;
  if (n) {
    CallCtx c;
    DeviceState* st = nullptr;
    rc = resolve_ctx(&o, &c, &st);
    if (rc) return done(rc);
    const size_t b_sums = (size_t)(n_out * kMsSums + 1) * 8;
    rc = ensure_capacity(*st, 4096 + align_up(b_sums));
    if (rc) return done(rc);
    Arena ws{st->base, st->cap, 0};
    uint64_t* d_sums = ws.take<uint64_t>(n_out * kMsSums + 1);
    if (!d_sums) return done(fail(M2S_ERR_HIP, "internal: workspace"));
    char* tmp = nullptr;   // a host caller's labels
    auto hip_fail = [&](hipError_t e) {
      (void)hipFree(tmp);
      return done(fail(M2S_ERR_HIP, "HIP error: %s", hipGetErrorString(e)));
    };
    hipStream_t s = c.stream;
    hipError_t e = hipSuccess;
    const uint32_t* d_labels = labels;
    if (labels && c.mem_kind == M2S_MEM_HOST) {
      e = hipMalloc((void**)&tmp, align_up(n * 4));
      if (e == hipSuccess) e = hipMemcpyAsync(tmp, labels, n * 4, hipMemcpyHostToDevice, s);
      if (e != hipSuccess) return hip_fail(e);
      d_labels = reinterpret_cast<const uint32_t*>(tmp);
    }
    const WalkGrid g = walk_grid_of(grid.cell_count, band->total, band->n_words);
    const uint64_t n_units = (g.n_words + kWalkUnit - 1) / kWalkUnit;   // below 2^22: a grid has fewer than 2^36 cells
    const unsigned blocks = (unsigned)std::min<uint64_t>(kMsMaxBlocks, (n_units + kWalkWaves - 1) / kWalkWaves);
    MsArgs a;
    for (int k = 0; k < 3; ++k) a.cs[k] = grid.cell_size[k];
    a.iso = iso;
    a.area_scale = std::ldexp(1.0, 24 - E);
    a.n_groups = n_out;
    if (c.timings) e = hipEventRecord(st->ev[0], s);
    if (e == hipSuccess) e = hipMemsetAsync(d_sums, 0, b_sums, s);
    if (e != hipSuccess) return hip_fail(e);
    hipLaunchKernelGGL(k_measure, dim3(blocks), dim3(kWalkThreads), 0, s, dev_of(band), g, n_units, a, d_labels, d_sums, d_sums + n_out * kMsSums);
    e = hipGetLastError();
    if (e == hipSuccess && c.timings) e = hipEventRecord(st->ev[1], s);
    if (e == hipSuccess) e = hipMemcpyAsync(sums, d_sums, b_sums, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e);
    (void)hipFree(tmp);
    if (c.timings) {
      (void)hipEventElapsedTime(&ms, st->ev[0], st->ev[1]);
      memset(c.timings, 0, sizeof(*c.timings));
      c.timings->distance_ms = ms;
      c.timings->total_ms = ms;
      c.timings->n_units = n;
      c.timings->distance_launches = 1;
    }
  } else if (o.timings) {
    memset(o.timings, 0, sizeof(*o.timings));
  }
  const double cs[3] = {(double)grid.cell_size[0], (double)grid.cell_size[1], (double)grid.cell_size[2]};
  for (uint64_t q = 0; q < n_out; ++q) {
    const uint64_t* r = sums + q * kMsSums;
    m2s_band_measure_record& m = measures_out[q];
    m.n_triangles = r[0];
    m.n_vertices = r[1];
    m.n_open = r[2];
    m.n_border = r[3];
    m.area_q = r[4];
    m.volume_q = (int64_t)r[5];
    for (int k = 0; k < 3; ++k) m.moment_q[k] = (int64_t)r[6 + k];
    m.area = std::ldexp((double)m.area_q, E - 25);
    const double v6 = (double)m.volume_q * 0x1p-20 / 6.0;   // the enclosed index volume
    m.volume = v6 * cs[0] * cs[1] * cs[2];
    for (int k = 0; k < 3; ++k)
      m.centroid[k] = m.volume_q ? (double)grid.first_cell[k] + ((double)m.moment_q[k] * 0x1p-8 / 24.0) / v6 * cs[k] : std::nan("");
  }
  if (info_out) {
    info_out->area_exponent = E;
    info_out->n_groups = n_out;
    info_out->n_skipped = sums[n_out * kMsSums];
  }
  return done(M2S_OK);
}

}  // extern "C"
