// geo_probe.hip — HOST build of the device math in geo.hip.h, ray.hip.h, sample.hip.h, voxel.hip.h, band.hip.h, cut_size.hip.h, sign.hip.h and shape.hip.h, for CPU unit tests only
// (tests/test_device_math_host.py, tests/test_rays_cpu.py, tests/test_sample_cpu.py, tests/test_voxelize_cpu.py, tests/test_narrow_band_cpu.py, tests/test_cut_size_cpu.py, tests/test_walk_leaf_count_cpu.py, tests/test_pair_eval_cpu.py, tests/test_sign_planes_cpu.py, tests/test_band_shapes_cpu.py).  Not linked into libm2s_hip.so.
#include "geo.hip.h"
#include "ray.hip.h"
#include "sample.hip.h"
#include "voxel.hip.h"
#include "band.hip.h"
#include "cut_size.hip.h"
#include "sign.hip.h"
#include "shape.hip.h"

using namespace m2s;

extern "C" {
float probe_dist2(const float* p, const float* a, const float* b, const float* c) {
  f3 A = mk3(a[0], a[1], a[2]), B = mk3(b[0], b[1], b[2]), Cc = mk3(c[0], c[1], c[2]);
  return point_triangle_dist2(mk3(p[0], p[1], p[2]), A, B, Cc, tri_edges(A, B, Cc), tri_class(A, B, Cc));
}
// n cases of 3 floats each: want[i] = point_triangle_dist2 with the edges of tri_edges (what the records store), got[i] = the queued pairs'
// evaluation from the vertices alone
void probe_pair_dist2_n(size_t n, const float* p, const float* a, const float* b, const float* c, float* want, float* got) {
  for (size_t i = 0; i < n; ++i) {
    const f3 P = mk3(p[3 * i], p[3 * i + 1], p[3 * i + 2]), A = mk3(a[3 * i], a[3 * i + 1], a[3 * i + 2]);
    const f3 B = mk3(b[3 * i], b[3 * i + 1], b[3 * i + 2]), Cc = mk3(c[3 * i], c[3 * i + 1], c[3 * i + 2]);
    const uint32_t cls = tri_class(A, B, Cc);
    want[i] = point_triangle_dist2(P, A, B, Cc, tri_edges(A, B, Cc), cls);
    got[i] = point_triangle_pair_dist2(P, A, B, Cc, cls);
  }
}
float probe_dist2_signed(const float* p, const float* a, const float* b, const float* c, int* positive) {
  f3 A = mk3(a[0], a[1], a[2]), B = mk3(b[0], b[1], b[2]), Cc = mk3(c[0], c[1], c[2]);
  bool pos;
  float d2 = point_triangle_dist2_signed(mk3(p[0], p[1], p[2]), A, B, Cc, tri_edges(A, B, Cc), tri_class(A, B, Cc), &pos);
  *positive = pos ? 1 : 0;
  return d2;
}
void probe_closest_point(const float* p, const float* a, const float* b, const float* c, float* out) {
  f3 A = mk3(a[0], a[1], a[2]), B = mk3(b[0], b[1], b[2]), Cc = mk3(c[0], c[1], c[2]);
  const f3 q = closest_point_triangle(mk3(p[0], p[1], p[2]), A, B, Cc, tri_edges(A, B, Cc), tri_class(A, B, Cc));
  out[0] = q.x; out[1] = q.y; out[2] = q.z;
}
int probe_ray(int axis, const float* o, const float* a, const float* b, const float* c, float* t) {
  return ray_triangle_aligned_rt(axis, mk3(o[0], o[1], o[2]), mk3(a[0], a[1], a[2]), mk3(b[0], b[1], b[2]),
                                 mk3(c[0], c[1], c[2]), t) ? 1 : 0;
}
// cut_size.hip.h: k_cut's size test, 1 where the node is small enough for the list
int probe_cut_small_enough(float R, float half, float emit_radius) { return cut_small_enough(R, half, emit_radius) ? 1 : 0; }
// ... for n triples at once (out: one byte each)
void probe_cut_small_enough_n(size_t n, const float* R, const float* half, const float* emit_radius, unsigned char* out) {
  for (size_t i = 0; i < n; ++i) out[i] = cut_small_enough(R[i], half[i], emit_radius[i]) ? 1 : 0;
}
// geo.hip.h: the leaf loop's trip count for n (off, skip) pairs of records of nb bytes
void probe_leaf_cursor_steps_n(size_t n, const uint32_t* off, const uint32_t* skip, uint32_t nb, uint32_t* out) {
  for (size_t i = 0; i < n; ++i) out[i] = leaf_cursor_steps(off[i], skip[i], nb);
}
// geo.hip.h: the packet walk's seed test for n (seed, tri, below, skip) quadruples of records of nb bytes (out: one byte each)
void probe_seed_in_leaf_n(size_t n, const uint32_t* seed, const uint32_t* tri, const uint32_t* below, const uint32_t* skip, uint32_t nb, unsigned char* out) {
  for (size_t i = 0; i < n; ++i) out[i] = seed_in_leaf(seed[i], tri[i], below[i], skip[i], nb) ? 1 : 0;
}
float probe_normal_fold_result(float d2_all, float d2_pos) { return normal_fold_result(d2_all, d2_pos); }
int probe_approx_eq_abs(float a, float b) { return approx_eq_abs(a, b) ? 1 : 0; }
void probe_tri_box(const float* a, const float* b, const float* c, float* mn, float* mx) {
  f3 lo, hi;
  triangle_bounding_box(mk3(a[0], a[1], a[2]), mk3(b[0], b[1], b[2]), mk3(c[0], c[1], c[2]), &lo, &hi);
  mn[0] = lo.x; mn[1] = lo.y; mn[2] = lo.z; mx[0] = hi.x; mx[1] = hi.y; mx[2] = hi.z;
}
// ray.hip.h: k = (kx, ky, kz), s = (Sx, Sy, Sz); returns RaySetup::valid
int probe_ray_setup(const float* o, const float* d, int* k, float* s) {
  const RaySetup r = ray_setup(mk3(o[0], o[1], o[2]), mk3(d[0], d[1], d[2]));
  k[0] = r.kx; k[1] = r.ky; k[2] = r.kz;
  s[0] = r.Sx; s[1] = r.Sy; s[2] = r.Sz;
  return r.valid ? 1 : 0;
}
// tuv = (t, u, v) where the ray's line meets the triangle (det != 0, signs agree), else untouched; returns 1 iff the ray is valid and
// hits within [t_min, t_max]
int probe_ray_triangle(const float* o, const float* d, const float* a, const float* b, const float* c, float t_min, float t_max, float* tuv) {
  const f3 O = mk3(o[0], o[1], o[2]);
  const RaySetup r = ray_setup(O, mk3(d[0], d[1], d[2]));
  const bool hit = ray_triangle_in_range(r, O, mk3(a[0], a[1], a[2]), mk3(b[0], b[1], b[2]), mk3(c[0], c[1], c[2]), t_min, t_max, &tuv[0], &tuv[1], &tuv[2]);
  return (r.valid && hit) ? 1 : 0;
}
// sample.hip.h
void probe_philox(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
  const Philox4 r = philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1]);
  for (int k = 0; k < 4; ++k) out[k] = r.r[k];
}
void probe_sample_random(uint64_t seed, uint64_t g, uint32_t* out) {
  const Philox4 r = sample_random(seed, g);
  for (int k = 0; k < 4; ++k) out[k] = r.r[k];
}
// n = the raw normal; returns A_t (0 when it is not finite)
float probe_tri_weight_area(const float* a, const float* b, const float* c, float* n) {
  f3 nn;
  const float A = tri_weight_area(mk3(a[0], a[1], a[2]), mk3(b[0], b[1], b[2]), mk3(c[0], c[1], c[2]), &nn);
  n[0] = nn.x; n[1] = nn.y; n[2] = nn.z;
  return A;
}
int probe_sample_exponent(float amax) { return sample_exponent(amax); }
uint64_t probe_sample_weight(float A, int e) { return sample_weight(A, e); }
uint64_t probe_sample_target(uint32_t r0, uint32_t r1, uint64_t W) { return sample_target(r0, r1, W); }
uint64_t probe_sample_pick(const uint64_t* C, uint64_t n, uint64_t T) { return sample_upper_bound(C, 0, n, T); }
void probe_sample_fold(uint32_t r2, uint32_t r3, float* uv) { sample_fold(r2, r3, &uv[0], &uv[1]); }
void probe_sample_point(const float* a, const float* b, const float* c, float u, float v, float* out) {
  const f3 p = sample_point(mk3(a[0], a[1], a[2]), mk3(b[0], b[1], b[2]), mk3(c[0], c[1], c[2]), u, v);
  out[0] = p.x; out[1] = p.y; out[2] = p.z;
}
void probe_sample_normal(const float* n, float A, float* out) {
  const f3 q = sample_normal(mk3(n[0], n[1], n[2]), A);
  out[0] = q.x; out[1] = q.y; out[2] = q.z;
}
// voxel.hip.h
// n (triangle, cell) pairs: tris 9 floats each (a, b, c), q and h 3 floats each; out[i] = overlap
void probe_vox_overlap(uint64_t n, const float* tris, const float* q, const float* h, uint8_t* out) {
  for (uint64_t i = 0; i < n; ++i) {
    const float* t = tris + 9 * i;
    const VoxTri tr = vox_tri(mk3(t[0], t[1], t[2]), mk3(t[3], t[4], t[5]), mk3(t[6], t[7], t[8]));
    const float qq[3] = {q[3 * i], q[3 * i + 1], q[3 * i + 2]}, hh[3] = {h[3 * i], h[3 * i + 1], h[3 * i + 2]};
    out[i] = vox_overlap(tr, qq, hh) ? 1 : 0;
  }
}
float probe_vox_centre(float first, float size, uint32_t idx) { return vox_centre(first, size, idx); }
void probe_vox_interval(float pa, float pb, float pc, float first, float size, uint32_t n, uint32_t* lo_hi) {
  vox_interval(pa, pb, pc, first, size, n, &lo_hi[0], &lo_hi[1]);
}
// One triangle over a whole grid the way the raster kernel goes: intervals, column clauses, cell clauses.  occ: n[0] * n[1] * n[2] bytes, OR-ed into.
void probe_vox_raster(const float* t, const float* first, const float* size, const uint32_t* n, uint8_t* occ) {
  const VoxTri tr = vox_tri(mk3(t[0], t[1], t[2]), mk3(t[3], t[4], t[5]), mk3(t[6], t[7], t[8]));
  if (!tr.finite) return;
  uint32_t lo[3], hi[3];
  for (int m = 0; m < 3; ++m) vox_interval(tr.a[m], tr.b[m], tr.c[m], first[m], size[m], n[m], &lo[m], &hi[m]);
  const float h[3] = {size[0] * 0.5f, size[1] * 0.5f, size[2] * 0.5f};
  for (uint32_t i = lo[0]; i < hi[0]; ++i)
    for (uint32_t j = lo[1]; j < hi[1]; ++j) {
      const float qx = vox_centre(first[0], size[0], i), qy = vox_centre(first[1], size[1], j);
      float v0[3] = {tr.a[0] - qx, tr.a[1] - qy, 0.0f}, v1[3] = {tr.b[0] - qx, tr.b[1] - qy, 0.0f}, v2[3] = {tr.c[0] - qx, tr.c[1] - qy, 0.0f};
      if (vox_column_miss(tr, v0, v1, v2, h)) continue;
      for (uint32_t k = lo[2]; k < hi[2]; ++k) {
        const float qz = vox_centre(first[2], size[2], k);
        v0[2] = tr.a[2] - qz; v1[2] = tr.b[2] - qz; v2[2] = tr.c[2] - qz;
        if (!vox_cell_miss(tr, v0, v1, v2, h)) occ[((size_t)i * n[1] + j) * n[2] + k] = 1;
      }
    }
}
// band.hip.h
float probe_band_reach(float r, float scale) { return band_reach(r, scale); }
// out: lo[3], hi[3], amax; returns any
int probe_band_box(const float* t, float* out) {
  const BandBox bx = band_box(mk3(t[0], t[1], t[2]), mk3(t[3], t[4], t[5]), mk3(t[6], t[7], t[8]));
  for (int m = 0; m < 3; ++m) { out[m] = bx.lo[m]; out[3 + m] = bx.hi[m]; }
  out[6] = bx.amax;
  return bx.any ? 1 : 0;
}
// out: n[3], rhs; returns use
int probe_band_plane(const float* t, float reach, const float* first, const float* size, const uint32_t* n, float* out) {
  const BandPlane pl = band_plane(mk3(t[0], t[1], t[2]), mk3(t[3], t[4], t[5]), mk3(t[6], t[7], t[8]), reach, {first[0], first[1], first[2]},
                                  {size[0], size[1], size[2]}, {n[0], n[1], n[2]});
  for (int m = 0; m < 3; ++m) out[m] = pl.n[m];
  out[3] = pl.rhs;
  return pl.use ? 1 : 0;
}
// n_tris triangles over a whole grid the way the kernels of band.hip go: the three axis intervals, the column test, the z interval tightened
// by the x and y gaps and by the plane test.  occ: n[0] * n[1] * n[2] bytes, OR-ed into.
void probe_band_candidates(uint64_t n_tris, const float* tris, const float* first, const float* size, const uint32_t* n, float r, float grid_scale,
                           uint8_t* occ) {
  for (uint64_t ti = 0; ti < n_tris; ++ti) {
    const float* t = tris + 9 * ti;
    const f3 a = mk3(t[0], t[1], t[2]), b = mk3(t[3], t[4], t[5]), c = mk3(t[6], t[7], t[8]);
    const BandBox bx = band_box(a, b, c);
    if (!bx.any) continue;
    const float reach = band_reach(r, bx.amax > grid_scale ? bx.amax : grid_scale), reach2 = reach * reach;
    const BandPlane pl = band_plane(a, b, c, reach, {first[0], first[1], first[2]}, {size[0], size[1], size[2]}, {n[0], n[1], n[2]});
    uint32_t lo[3], hi[3];
    for (int m = 0; m < 3; ++m) band_interval(bx.lo[m], bx.hi[m], first[m], size[m], 0u, n[m], 0.0f, 0.0f, reach2, &lo[m], &hi[m]);
    if (lo[2] >= hi[2]) continue;
    for (uint32_t i = lo[0]; i < hi[0]; ++i)
      for (uint32_t j = lo[1]; j < hi[1]; ++j) {
        const float qx = cell_center(first[0], size[0], i), qy = cell_center(first[1], size[1], j);
        const float gx = band_gap(bx.lo[0], bx.hi[0], qx), gy = band_gap(bx.lo[1], bx.hi[1], qy);
        if (!band_near(gx, gy, 0.0f, reach2)) continue;
        uint32_t klo, khi;
        band_interval(bx.lo[2], bx.hi[2], first[2], size[2], lo[2], hi[2], gx, gy, reach2, &klo, &khi);
        band_plane_interval(pl, band_plane_xy(pl, qx, qy), first[2], size[2], klo, khi, &klo, &khi);
        for (uint32_t k = klo; k < khi; ++k) occ[((size_t)i * n[1] + j) * n[2] + k] = 1;
      }
  }
}
// sign.hip.h
static GridParams probe_sign_grid(const float* first, const float* size, const uint32_t* n) {
  GridParams g = {};
  for (int m = 0; m < 3; ++m) { g.first[m] = first[m]; g.size[m] = size[m]; g.n[m] = n[m]; }
  g.nzw = (n[2] + 31u) / 32u;
  return g;
}
// the f32 centre the marking kernels give cell idx of a line's free axis
float probe_sign_centre(float first, float size, uint32_t idx) { return cell_center(first, size, idx); }
// ... of m cells at once
void probe_sign_centres_n(float first, float size, size_t m, const uint32_t* idx, float* out) {
  for (size_t i = 0; i < m; ++i) out[i] = cell_center(first, size, idx[i]);
}
// lo_hi = the inclusive range (lo > hi: empty)
void probe_sign_axis_range(float bmn, float bmx, float first, float cs, uint32_t n, uint32_t* lo_hi) {
  axis_range(bmn, bmx, first, cs, n, &lo_hi[0], &lo_hi[1]);
}
// ... for m quintuples at once (lo_hi: 2 m words)
void probe_sign_axis_range_n(size_t m, const float* bmn, const float* bmx, const float* first, const float* cs, const uint32_t* n, uint32_t* lo_hi) {
  for (size_t i = 0; i < m; ++i) axis_range(bmn[i], bmx[i], first[i], cs[i], n[i], &lo_hi[2 * i], &lo_hi[2 * i + 1]);
}
// tri: 9 floats (a, b, c); slab: lo, hi, chunk_log, period, all; out = ulo, uhi, wlo, whi of the window of the lines along `axis`.
// Returns window_count.
uint32_t probe_sign_window(const float* tri, const float* first, const float* size, const uint32_t* n, const uint32_t* slab, int axis, uint32_t* out) {
  const GridParams g = probe_sign_grid(first, size, n);
  const SlabX sx = {slab[0], slab[1], slab[2], slab[3], slab[4] != 0u};
  f3 mn, mx;
  triangle_bounding_box(mk3(tri[0], tri[1], tri[2]), mk3(tri[3], tri[4], tri[5]), mk3(tri[6], tri[7], tri[8]), &mn, &mx);
  const Window w = axis == 0 ? make_window<0>(mn, mx, g, sx) : axis == 1 ? make_window<1>(mn, mx, g, sx) : make_window<2>(mn, mx, g, sx);
  out[0] = w.ulo; out[1] = w.uhi; out[2] = w.wlo; out[3] = w.whi;
  return window_count(w);
}
// the largest window_count of n_tris triangles (9 floats each) per axis: out[3]
void probe_sign_max_window(size_t n_tris, const float* tris, const float* first, const float* size, const uint32_t* n, const uint32_t* slab, uint32_t* out) {
  uint32_t w[4];
  out[0] = out[1] = out[2] = 0;
  for (size_t i = 0; i < n_tris; ++i)
    for (int axis = 0; axis < 3; ++axis) {
      const uint32_t c = probe_sign_window(tris + 9 * i, first, size, n, slab, axis, w);
      if (c > out[axis]) out[axis] = c;
    }
}
// slab: lo, hi, chunk_log, period, all; out[x] = x_in_slab for x < nx
void probe_sign_x_in_slab(const uint32_t* slab, uint32_t nx, uint8_t* out) {
  const SlabX sx = {slab[0], slab[1], slab[2], slab[3], slab[4] != 0u};
  for (uint32_t x = 0; x < nx; ++x) out[x] = x_in_slab(sx, x) ? 1 : 0;
}
uint32_t probe_sign_bucket(float t, float cell_size, uint32_t n) { return ray_bucket(t, cell_size, n); }
// out = lanes per triangle, list flag, rows form of the z combine; consts = SMALL_WINDOW, RAY_MARK_SHARED_BELOW, LIST_ABOVE_LINES, BIG_CHUNK
void probe_sign_path(uint32_t n_tris, const uint32_t* n, uint32_t* out, uint64_t* consts) {
  const float zero[3] = {0.0f, 0.0f, 0.0f};
  const SignPath p = sign_path(n_tris, probe_sign_grid(zero, zero, n));
  out[0] = p.lanes; out[1] = p.list ? 1u : 0u; out[2] = p.rows ? 1u : 0u;
  consts[0] = SMALL_WINDOW; consts[1] = RAY_MARK_SHARED_BELOW; consts[2] = LIST_ABOVE_LINES; consts[3] = BIG_CHUNK;
}
// shape.hip.h
static Capsule probe_capsule(const float* s) { return Capsule{{s[0], s[1], s[2]}, {s[3], s[4], s[5]}, s[6]}; }
// n (shape, point) pairs: shapes 7 floats each (a, b, r), points 3 floats each; out[i] = d_s
void probe_shape_dist_n(uint64_t n, const float* shapes, const float* points, float* out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = shape_dist(probe_capsule(shapes + 7 * i), points[3 * i], points[3 * i + 1], points[3 * i + 2]);
}
// lo_hi = lo[3], hi[3] of the shape's index box on the grid; returns shape_sound (0: lo_hi untouched)
int probe_shape_box(const float* shape, const float* first, const float* size, const uint32_t* n, float exterior, uint32_t* lo_hi) {
  const Capsule s = probe_capsule(shape);
  if (!shape_sound(s)) return 0;
  const float f[3] = {first[0], first[1], first[2]}, sz[3] = {size[0], size[1], size[2]};
  const uint32_t cnt[3] = {n[0], n[1], n[2]};
  uint32_t lo[3], hi[3];
  shape_box(s, f, sz, cnt, exterior, shape_grid_scale(f, sz, cnt), lo, hi);
  for (int m = 0; m < 3; ++m) { lo_hi[m] = lo[m]; lo_hi[3 + m] = hi[m]; }
  return 1;
}
uint32_t probe_shape_key(float x) { return shape_key(x); }
float probe_shape_unkey(uint32_t k) { return shape_unkey(k); }
float probe_shape_err_u(void) { return SHAPE_ERR_U; }
}
