// mesh_to_sdf.hpp — C++17 host-side mirror of the reference crate's public interface over the C ABI (m2s.h).
//
// The reference is compiled code (Rust, crate mesh_to_sdf 0.4.0); its toolchain is absent from the build image,
// so this header is the host side a C++ caller — or a maintainer porting call sites — uses: same names, same
// argument meaning, same error behaviour (a reference panic is a mesh_to_sdf::Panic exception here):
//
//   Topology<I>            mesh_to_sdf/src/lib.rs:151-193     TriangleList / TriangleStrip, optional indices
//   SignMethod             lib.rs:204-216                      Raycast (default) | Normal
//   AccelerationMethod     lib.rs:224-239                      None(sign) | Bvh(sign) | Rtree | RtreeBvh (default)
//   generate_sdf           lib.rs:291-311
//   Grid<V>                grid.rs:30-170                      new_ / from_bounding_box / getters / snap_point_to_grid
//   generate_grid_sdf      generate/grid.rs:265-378
//   closest_points / grid_closest_points                       nearest triangle + closest point (no reference counterpart; m2s.h)
//   winding_numbers / grid_winding_numbers / generate_grid_sdf_winding   generalized winding numbers and their sign (m2s.h)
//   cast_rays / count_intersections / test_occlusions   watertight ray casting against the mesh (m2s.h)
//   sample_surface / surface_area   area-weighted surface samples, defined to the bit (m2s.h)
//   voxelize                        surface / solid occupancy of a grid, defined to the bit (m2s.h)
//   narrow_band_sdf                 the cells of a grid within a band of the surface and their distances: the dense result, filtered (m2s.h)
//   sample_grid / raymarch_grid  client draw_raymarching.wgsl  sdf_grid / estimate_normal / sdf_3d on a finished grid (m2s.h)
//   BandField                    (no counterpart)              the same two queries on a narrow band, no dense grid (m2s.h)
//   BandField::csg / export_band (no counterpart)              union, intersection, difference of two band fields on the device; a field's lists back out (m2s.h)
//   grid_isosurface                                            marching-cubes mesh of a level set of a finished grid (no reference counterpart; m2s.h)
//   band_isosurface                                            the same from a narrow band: cells and distances in, mesh and n_open out,
//                                                              work proportional to the band (no reference counterpart; m2s.h)
//   serde::*               serde.rs:75-221                     SerializeSdf / DeserializeSdf / save_to_file / read_from_file
//
// V is any point type with x(), y(), z() | .x .y .z | operator[] (the reference's `Point` trait adapters,
// point/impl_*.rs: [f32;3], glam, cgmath, nalgebra, mint all reduce to three f32).  Header only; link -lm2s_hip.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <variant>
#include <vector>

#include "m2s.h"

namespace mesh_to_sdf {

// ---- errors ------------------------------------------------------------------------------------------
struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error("m2s error " + std::to_string(c) + ": " + m), code(c) {}
};
// The reference would have panicked here: index out of range, "NaN distance" (lib.rs:257), Rtree on an empty mesh.
struct Panic : Error { using Error::Error; };

namespace detail {
inline void check(int rc) {
  if (rc == M2S_OK) return;
  const std::string msg = m2s_last_error();
  if (rc == M2S_ERR_BAD_ARG || rc == M2S_ERR_NAN || rc == M2S_ERR_EMPTY_MESH) throw Panic(rc, msg);
  throw Error(rc, msg);
}

// ---- Point access (point.rs:11-76: the trait needs new / x / y / z) -------------------------------------
template <class V, class = void> struct has_xyz_fn : std::false_type {};
template <class V> struct has_xyz_fn<V, std::void_t<decltype(std::declval<const V&>().x()), decltype(std::declval<const V&>().z())>> : std::true_type {};
template <class V, class = void> struct has_xyz_mem : std::false_type {};
template <class V> struct has_xyz_mem<V, std::void_t<decltype(std::declval<const V&>().x + std::declval<const V&>().z)>> : std::true_type {};

template <class V> float px(const V& v) { if constexpr (has_xyz_fn<V>::value) return v.x(); else if constexpr (has_xyz_mem<V>::value) return v.x; else return v[0]; }
template <class V> float py(const V& v) { if constexpr (has_xyz_fn<V>::value) return v.y(); else if constexpr (has_xyz_mem<V>::value) return v.y; else return v[1]; }
template <class V> float pz(const V& v) { if constexpr (has_xyz_fn<V>::value) return v.z(); else if constexpr (has_xyz_mem<V>::value) return v.z; else return v[2]; }
template <class V> V make_point(float x, float y, float z) {
  if constexpr (std::is_constructible_v<V, float, float, float>) return V(x, y, z);
  else return V{x, y, z};
}

// Packed xyz view of a point array: zero-copy when V already is three consecutive floats.
template <class V>
struct Packed {
  const float* ptr = nullptr;
  std::vector<float> copy;
  Packed(const V* p, size_t n) {
    if constexpr (sizeof(V) == 12 && std::is_trivially_copyable_v<V> && !has_xyz_fn<V>::value) {
      ptr = reinterpret_cast<const float*>(p);
    } else {
      copy.resize(3 * n);
      for (size_t i = 0; i < n; ++i) { copy[3 * i] = px(p[i]); copy[3 * i + 1] = py(p[i]); copy[3 * i + 2] = pz(p[i]); }
      ptr = copy.data();
    }
  }
};
}  // namespace detail

// ---- enums ---------------------------------------------------------------------------------------------
enum class SignMethod : int { Raycast = M2S_SIGN_RAYCAST, Normal = M2S_SIGN_NORMAL };   // default Raycast

struct AccelerationMethod {
  int kind = M2S_ACCEL_RTREE_BVH;                 // default RtreeBvh (lib.rs:233)
  SignMethod sign = SignMethod::Raycast;
  static AccelerationMethod None(SignMethod s = SignMethod::Raycast) { return {M2S_ACCEL_NONE, s}; }
  static AccelerationMethod Bvh(SignMethod s = SignMethod::Raycast) { return {M2S_ACCEL_BVH, s}; }
  static AccelerationMethod Rtree() { return {M2S_ACCEL_RTREE, SignMethod::Normal}; }
  static AccelerationMethod RtreeBvh() { return {M2S_ACCEL_RTREE_BVH, SignMethod::Raycast}; }
};

template <class I = uint32_t>
struct Topology {
  int kind = M2S_TRIANGLE_LIST;
  const I* indices = nullptr;   // nullptr == None: 0..vertices.len()
  size_t count = 0;
  static Topology TriangleList() { return {M2S_TRIANGLE_LIST, nullptr, 0}; }
  static Topology TriangleList(const I* idx, size_t n) { return {M2S_TRIANGLE_LIST, idx, n}; }
  static Topology TriangleList(const std::vector<I>& idx) { return {M2S_TRIANGLE_LIST, idx.data(), idx.size()}; }
  static Topology TriangleStrip() { return {M2S_TRIANGLE_STRIP, nullptr, 0}; }
  static Topology TriangleStrip(const I* idx, size_t n) { return {M2S_TRIANGLE_STRIP, idx, n}; }
  static Topology TriangleStrip(const std::vector<I>& idx) { return {M2S_TRIANGLE_STRIP, idx.data(), idx.size()}; }
  bool has_indices() const { return indices != nullptr || count != 0; }
};

namespace detail {
// I: Copy + Into<u32> — u16 and u32 pass through, anything else is widened once.
template <class I>
struct IndexArg {
  const void* ptr = nullptr;
  int bytes = 4;
  std::vector<uint32_t> widened;
  static uint32_t dummy() { return 0; }
  explicit IndexArg(const Topology<I>& t) {
    static const uint32_t kEmpty = 0;
    if (!t.has_indices()) return;                                  // None
    if (t.count == 0) { ptr = &kEmpty; return; }                   // Some(&[])
    if constexpr (std::is_integral_v<I> && (sizeof(I) == 2 || sizeof(I) == 4) && std::is_unsigned_v<I>) {
      ptr = t.indices;
      bytes = (int)sizeof(I);
    } else {
      widened.resize(t.count);
      for (size_t i = 0; i < t.count; ++i) widened[i] = static_cast<uint32_t>(t.indices[i]);
      ptr = widened.data();
    }
  }
};
}  // namespace detail

// ---- generate_sdf (lib.rs:291-311) ----------------------------------------------------------------------------
template <class V, class I = uint32_t>
std::vector<float> generate_sdf(const V* vertices, size_t n_vertices, const Topology<I>& indices, const V* query_points,
                                size_t n_queries, AccelerationMethod acceleration_method = AccelerationMethod()) {
  detail::Packed<V> v(vertices, n_vertices), q(query_points, n_queries);
  detail::IndexArg<I> ia(indices);
  std::vector<float> out(n_queries);
  size_t n_out = 0;
  detail::check(m2s_generate_sdf(v.ptr, n_vertices, ia.ptr, indices.count, ia.bytes, indices.kind, q.ptr, n_queries,
                                 acceleration_method.kind, (int)acceleration_method.sign, out.data(), &n_out, nullptr));
  out.resize(n_out);   // RtreeBvh on a mesh without triangles returns an empty Vec (generic/rtree_bvh.rs:104-106)
  return out;
}
template <class V, class I = uint32_t>
std::vector<float> generate_sdf(const std::vector<V>& vertices, const Topology<I>& indices, const std::vector<V>& query_points,
                                AccelerationMethod acceleration_method = AccelerationMethod()) {
  return generate_sdf(vertices.data(), vertices.size(), indices, query_points.data(), query_points.size(), acceleration_method);
}

// ---- Grid (grid.rs:30-170) ----------------------------------------------------------------------------------------
enum class SnapKind { Inside, Outside };   // SnapResult, grid.rs:10-17
struct SnapResult {
  SnapKind kind;
  std::array<size_t, 3> cell;
  bool operator==(const SnapResult& o) const { return kind == o.kind && cell == o.cell; }
};

template <class V>
class Grid {
 public:
  Grid() = default;
  static Grid new_(const V& first_cell, const V& cell_size, std::array<size_t, 3> cell_count) {   // grid.rs:43-49
    Grid g;
    const float f[3] = {detail::px(first_cell), detail::py(first_cell), detail::pz(first_cell)};
    const float s[3] = {detail::px(cell_size), detail::py(cell_size), detail::pz(cell_size)};
    for (int k = 0; k < 3; ++k) { g.g_.first_cell[k] = f[k]; g.g_.cell_size[k] = s[k]; g.g_.cell_count[k] = cell_count[k]; }
    return g;
  }
  static Grid from_bounding_box(const V& bbox_min, const V& bbox_max, std::array<size_t, 3> cell_count) {   // grid.rs:59-74
    Grid g;
    const float mn[3] = {detail::px(bbox_min), detail::py(bbox_min), detail::pz(bbox_min)};
    const float mx[3] = {detail::px(bbox_max), detail::py(bbox_max), detail::pz(bbox_max)};
    const uint64_t c[3] = {cell_count[0], cell_count[1], cell_count[2]};
    m2s_grid_from_bounding_box(mn, mx, c, &g.g_);
    return g;
  }
  V get_first_cell() const { return detail::make_point<V>(g_.first_cell[0], g_.first_cell[1], g_.first_cell[2]); }
  V get_cell_size() const { return detail::make_point<V>(g_.cell_size[0], g_.cell_size[1], g_.cell_size[2]); }
  std::array<size_t, 3> get_cell_count() const { return {(size_t)g_.cell_count[0], (size_t)g_.cell_count[1], (size_t)g_.cell_count[2]}; }
  size_t get_total_cell_count() const { return (size_t)(g_.cell_count[0] * g_.cell_count[1] * g_.cell_count[2]); }
  V get_last_cell() const {   // grid.rs:82-88, as written there: first + count * size
    float o[3];
    for (int k = 0; k < 3; ++k) { const float prod = (float)g_.cell_count[k] * g_.cell_size[k]; o[k] = g_.first_cell[k] + prod; }
    return detail::make_point<V>(o[0], o[1], o[2]);
  }
  std::pair<V, V> get_bounding_box() const {   // grid.rs:110-119
    float mn[3], mx[3];
    for (int k = 0; k < 3; ++k) {
      const float half = g_.cell_size[k] * 0.5f;
      mn[k] = g_.first_cell[k] - half;
      const float prod = (float)g_.cell_count[k] * g_.cell_size[k];
      mx[k] = mn[k] + prod;
    }
    return {detail::make_point<V>(mn[0], mn[1], mn[2]), detail::make_point<V>(mx[0], mx[1], mx[2])};
  }
  size_t get_cell_idx(std::array<size_t, 3> cell) const {   // grid.rs:122-124
    const uint64_t c[3] = {cell[0], cell[1], cell[2]};
    return (size_t)m2s_grid_cell_idx(&g_, c);
  }
  std::array<size_t, 3> get_cell_integer_coordinates(size_t cell_idx) const {   // grid.rs:127-132
    const size_t ny = g_.cell_count[1], nz = g_.cell_count[2];
    return {cell_idx / (ny * nz), (cell_idx / nz) % ny, cell_idx % nz};
  }
  V get_cell_center(std::array<size_t, 3> cell) const {   // grid.rs:135-141
    const uint64_t c[3] = {cell[0], cell[1], cell[2]};
    float o[3];
    m2s_grid_cell_center(&g_, c, o);
    return detail::make_point<V>(o[0], o[1], o[2]);
  }
  SnapResult snap_point_to_grid(const V& point) const {   // grid.rs:145-170
    const float p[3] = {detail::px(point), detail::py(point), detail::pz(point)};
    SnapResult r{SnapKind::Inside, {0, 0, 0}};
    for (int k = 0; k < 3; ++k) {
      const float half = g_.cell_size[k] * 0.5f;
      const float mn = g_.first_cell[k] - half;
      const float cell = std::floor((p[k] - mn) / g_.cell_size[k]);
      const long long n = (long long)g_.cell_count[k];
      long long ic = std::isnan(cell) ? 0 : (cell >= 9.2e18f ? n : cell <= -9.2e18f ? -1 : (long long)cell);   // `as isize` saturates
      if (ic < 0 || ic >= n) r.kind = SnapKind::Outside;
      r.cell[k] = (size_t)(ic < 0 ? 0 : ic >= n ? n - 1 : ic);
    }
    return r;
  }
  bool operator==(const Grid& o) const { return std::memcmp(&g_, &o.g_, sizeof(g_)) == 0; }   // #[derive(PartialEq)]
  const m2s_grid& raw() const { return g_; }
  static Grid from_raw(const m2s_grid& g) { Grid r; r.g_ = g; return r; }

 private:
  m2s_grid g_{};
};

// ---- generate_grid_sdf (generate/grid.rs:265-378) --------------------------------------------------------------------
template <class V, class I = uint32_t>
std::vector<float> generate_grid_sdf(const V* vertices, size_t n_vertices, const Topology<I>& indices, const Grid<V>& grid,
                                     SignMethod sign_method = SignMethod::Raycast) {
  detail::Packed<V> v(vertices, n_vertices);
  detail::IndexArg<I> ia(indices);
  std::vector<float> out(grid.get_total_cell_count());
  detail::check(m2s_generate_grid_sdf(v.ptr, n_vertices, ia.ptr, indices.count, ia.bytes, indices.kind, &grid.raw(), (int)sign_method,
                                      out.data(), nullptr));
  return out;
}
template <class V, class I = uint32_t>
std::vector<float> generate_grid_sdf(const std::vector<V>& vertices, const Topology<I>& indices, const Grid<V>& grid,
                                     SignMethod sign_method = SignMethod::Raycast) {
  return generate_grid_sdf(vertices.data(), vertices.size(), indices, grid, sign_method);
}

// ---- closest points (m2s_closest_points, m2s_grid_closest_points) --------------------------------------------------------
// Nearest triangle (Topology order, lowest index on ties, UINT32_MAX if none is comparable), the closest point on it and the unsigned
// distance, per query point or per grid cell (grid order).  The distances are bit-equal to |generate_sdf(.., RtreeBvh)|.
struct ClosestPoints {
  std::vector<uint32_t> triangle;
  std::vector<std::array<float, 3>> point;
  std::vector<float> distance;
};
template <class V, class I = uint32_t>
ClosestPoints closest_points(const V* vertices, size_t n_vertices, const Topology<I>& indices, const V* query_points, size_t n_queries) {
  detail::Packed<V> v(vertices, n_vertices), q(query_points, n_queries);
  detail::IndexArg<I> ia(indices);
  ClosestPoints r;
  r.triangle.resize(n_queries);
  r.point.resize(n_queries);
  r.distance.resize(n_queries);
  static_assert(sizeof(std::array<float, 3>) == 12, "packed xyz");
  detail::check(m2s_closest_points(v.ptr, n_vertices, ia.ptr, indices.count, ia.bytes, indices.kind, q.ptr, n_queries, r.triangle.data(),
                                   reinterpret_cast<float*>(r.point.data()), r.distance.data(), nullptr));
  return r;
}
template <class V, class I = uint32_t>
ClosestPoints closest_points(const std::vector<V>& vertices, const Topology<I>& indices, const std::vector<V>& query_points) {
  return closest_points(vertices.data(), vertices.size(), indices, query_points.data(), query_points.size());
}
template <class V, class I = uint32_t>
ClosestPoints grid_closest_points(const V* vertices, size_t n_vertices, const Topology<I>& indices, const Grid<V>& grid) {
  detail::Packed<V> v(vertices, n_vertices);
  detail::IndexArg<I> ia(indices);
  const size_t n = grid.get_total_cell_count();
  ClosestPoints r;
  r.triangle.resize(n);
  r.point.resize(n);
  r.distance.resize(n);
  detail::check(m2s_grid_closest_points(v.ptr, n_vertices, ia.ptr, indices.count, ia.bytes, indices.kind, &grid.raw(), r.triangle.data(),
                                        reinterpret_cast<float*>(r.point.data()), r.distance.data(), nullptr));
  return r;
}
template <class V, class I = uint32_t>
ClosestPoints grid_closest_points(const std::vector<V>& vertices, const Topology<I>& indices, const Grid<V>& grid) {
  return grid_closest_points(vertices.data(), vertices.size(), indices, grid);
}

// ---- generalized winding numbers (m2s_winding_numbers, m2s_grid_winding_numbers) ------------------------------------------
// w per query point or per grid cell (grid order): 1 inside, 0 outside a closed mesh whose right-hand normals point outward, smooth
// across holes; w >= 0.5 is the robust inside test.  beta: the Barnes-Hut opening parameter (>= 1, +inf = exact).
template <class V, class I = uint32_t>
std::vector<float> winding_numbers(const V* vertices, size_t n_vertices, const Topology<I>& indices, const V* query_points, size_t n_queries,
                                   float beta = M2S_WINDING_BETA_DEFAULT) {
  detail::Packed<V> v(vertices, n_vertices), q(query_points, n_queries);
  detail::IndexArg<I> ia(indices);
  std::vector<float> w(n_queries);
  detail::check(m2s_winding_numbers(v.ptr, n_vertices, ia.ptr, indices.count, ia.bytes, indices.kind, q.ptr, n_queries, beta, 0.5f, w.data(),
                                    nullptr, nullptr));
  return w;
}
template <class V, class I = uint32_t>
std::vector<float> winding_numbers(const std::vector<V>& vertices, const Topology<I>& indices, const std::vector<V>& query_points,
                                   float beta = M2S_WINDING_BETA_DEFAULT) {
  return winding_numbers(vertices.data(), vertices.size(), indices, query_points.data(), query_points.size(), beta);
}
template <class V, class I = uint32_t>
std::vector<float> grid_winding_numbers(const V* vertices, size_t n_vertices, const Topology<I>& indices, const Grid<V>& grid,
                                        float beta = M2S_WINDING_BETA_DEFAULT) {
  detail::Packed<V> v(vertices, n_vertices);
  detail::IndexArg<I> ia(indices);
  std::vector<float> w(grid.get_total_cell_count());
  detail::check(m2s_grid_winding_numbers(v.ptr, n_vertices, ia.ptr, indices.count, ia.bytes, indices.kind, &grid.raw(), beta, 0.5f, w.data(),
                                         nullptr, nullptr));
  return w;
}
template <class V, class I = uint32_t>
std::vector<float> grid_winding_numbers(const std::vector<V>& vertices, const Topology<I>& indices, const Grid<V>& grid,
                                        float beta = M2S_WINDING_BETA_DEFAULT) {
  return grid_winding_numbers(vertices.data(), vertices.size(), indices, grid, beta);
}
// Signed distances with the winding number's sign: -d where w >= threshold, else d.
template <class V, class I = uint32_t>
std::vector<float> generate_grid_sdf_winding(const std::vector<V>& vertices, const Topology<I>& indices, const Grid<V>& grid,
                                             float beta = M2S_WINDING_BETA_DEFAULT, float threshold = 0.5f) {
  detail::Packed<V> v(vertices.data(), vertices.size());
  detail::IndexArg<I> ia(indices);
  std::vector<float> d(grid.get_total_cell_count());
  detail::check(m2s_grid_winding_numbers(v.ptr, vertices.size(), ia.ptr, indices.count, ia.bytes, indices.kind, &grid.raw(), beta, threshold,
                                         nullptr, d.data(), nullptr));
  return d;
}

// ---- ray casting against the mesh (m2s_cast_rays) -------------------------------------------------------------------------------
// The watertight test of Woop, Benthin and Wald, defined to the bit (m2s.h): per ray o + t d, t_min <= t <= t_max, the first hit (t = +inf,
// triangle = UINT32_MAX, uv = NaN when none), the number of triangles hit, or whether anything is in the way.  Directions are used as
// given, so t is in units of |d|.
struct RayHits {
  std::vector<float> t;
  std::vector<uint32_t> triangle;
  std::vector<std::array<float, 2>> uv;   // hit = a + u (b - a) + v (c - a)
};
namespace detail {
template <class V, class I>
void cast_rays_call(const std::vector<V>& vertices, const Topology<I>& indices, const std::vector<V>& origins, const std::vector<V>& directions,
                    float t_min, float t_max, float* t, uint32_t* triangle, float* uv, uint32_t* count, uint8_t* occluded) {
  if (origins.size() != directions.size()) throw Panic(M2S_ERR_BAD_ARG, "origins and directions differ in length");
  Packed<V> v(vertices.data(), vertices.size()), o(origins.data(), origins.size()), d(directions.data(), directions.size());
  IndexArg<I> ia(indices);
  const m2s_ray_opts ro = {sizeof(m2s_ray_opts), t_min, t_max};
  check(m2s_cast_rays(v.ptr, vertices.size(), ia.ptr, indices.count, ia.bytes, indices.kind, o.ptr, d.ptr, origins.size(), &ro, t, triangle, uv,
                      count, occluded, nullptr));
}
}  // namespace detail
template <class V, class I = uint32_t>
RayHits cast_rays(const std::vector<V>& vertices, const Topology<I>& indices, const std::vector<V>& origins, const std::vector<V>& directions,
                  float t_min = 0.0f, float t_max = std::numeric_limits<float>::infinity()) {
  RayHits r;
  r.t.resize(origins.size());
  r.triangle.resize(origins.size());
  r.uv.resize(origins.size());
  detail::cast_rays_call(vertices, indices, origins, directions, t_min, t_max, r.t.data(), r.triangle.data(),
                         r.uv.empty() ? nullptr : r.uv.data()->data(), nullptr, nullptr);
  return r;
}
// A ray through a shared edge or vertex counts every triangle that includes it.
template <class V, class I = uint32_t>
std::vector<uint32_t> count_intersections(const std::vector<V>& vertices, const Topology<I>& indices, const std::vector<V>& origins,
                                          const std::vector<V>& directions, float t_min = 0.0f,
                                          float t_max = std::numeric_limits<float>::infinity()) {
  std::vector<uint32_t> n(origins.size());
  detail::cast_rays_call(vertices, indices, origins, directions, t_min, t_max, nullptr, nullptr, nullptr, n.data(), nullptr);
  return n;
}
template <class V, class I = uint32_t>
std::vector<uint8_t> test_occlusions(const std::vector<V>& vertices, const Topology<I>& indices, const std::vector<V>& origins,
                                     const std::vector<V>& directions, float t_min = 0.0f,
                                     float t_max = std::numeric_limits<float>::infinity()) {
  std::vector<uint8_t> occ(origins.size());
  detail::cast_rays_call(vertices, indices, origins, directions, t_min, t_max, nullptr, nullptr, nullptr, nullptr, occ.data());
  return occ;
}

// ---- area-weighted surface sampling (m2s_sample_surface) ---------------------------------------------------------------------------
// Points distributed uniformly over the surface, defined to the bit (m2s.h): sample i is global sample first_sample + i and depends only
// on the triangles in Topology order, the seed and that number.  A mesh without area throws (M2S_ERR_EMPTY_MESH) when n > 0.
struct SurfaceSamples {
  std::vector<std::array<float, 3>> points;
  std::vector<uint32_t> triangle;            // Topology order
  std::vector<std::array<float, 2>> uv;      // point = a + u (b - a) + v (c - a)
  std::vector<std::array<float, 3>> normal;  // unit right-hand normal of the triangle; empty unless asked for
  double area = 0.0;                         // total area of the triangles the sampler can reach
};
template <class V, class I = uint32_t>
SurfaceSamples sample_surface(const std::vector<V>& vertices, const Topology<I>& indices, size_t n, uint64_t seed = 0, uint64_t first_sample = 0,
                              bool normals = false) {
  detail::Packed<V> v(vertices.data(), vertices.size());
  detail::IndexArg<I> ia(indices);
  SurfaceSamples r;
  r.points.resize(n);
  r.triangle.resize(n);
  r.uv.resize(n);
  if (normals) r.normal.resize(n);
  const m2s_surface_sample_opts so = {sizeof(m2s_surface_sample_opts), 0, seed, first_sample};
  detail::check(m2s_sample_surface(v.ptr, vertices.size(), ia.ptr, indices.count, ia.bytes, indices.kind, n, &so,
                                   n ? r.points.data()->data() : nullptr, n ? r.triangle.data() : nullptr, n ? r.uv.data()->data() : nullptr,
                                   (n && normals) ? r.normal.data()->data() : nullptr, &r.area, nullptr));
  return r;
}
template <class V, class I = uint32_t>
double surface_area(const std::vector<V>& vertices, const Topology<I>& indices) {
  return sample_surface(vertices, indices, 0).area;
}

// ---- voxelization (m2s_voxelize) -----------------------------------------------------------------------------------------------------
// Which cells of the grid the mesh occupies, defined to the bit (m2s.h): a cell is set when its closed box touches a triangle, and with
// `solid` also when its centre is inside by the Raycast sign of generate_grid_sdf.
struct Voxels {
  std::vector<uint8_t> occupancy;   // 0 / 1 per cell, grid order (Grid::get_cell_idx)
  std::vector<uint32_t> bits;       // cell (i, j, k) is bit k & 31 of word (i * ny + j) * ceil(nz / 32) + (k >> 5); empty unless asked for
  uint64_t count = 0;               // set cells
};
template <class V, class I = uint32_t>
Voxels voxelize(const std::vector<V>& vertices, const Topology<I>& indices, const Grid<V>& grid, bool solid = false, bool bits = false) {
  detail::Packed<V> v(vertices.data(), vertices.size());
  detail::IndexArg<I> ia(indices);
  Voxels r;
  const auto n = grid.get_cell_count();
  r.occupancy.resize(grid.get_total_cell_count());
  if (bits) r.bits.resize(n[0] * n[1] * ((n[2] + 31) / 32));
  const m2s_voxelize_opts vo = {sizeof(m2s_voxelize_opts), (uint32_t)(solid ? M2S_VOXELIZE_SOLID : M2S_VOXELIZE_SURFACE)};
  detail::check(m2s_voxelize(v.ptr, vertices.size(), ia.ptr, indices.count, ia.bytes, indices.kind, &grid.raw(), &vo,
                             r.bits.empty() ? nullptr : r.bits.data(), r.occupancy.empty() ? nullptr : r.occupancy.data(), nullptr, 0, &r.count,
                             nullptr));
  return r;
}

// ---- narrow bands (m2s_narrow_band_sdf) ------------------------------------------------------------------------------------------------
// The cells whose generate_grid_sdf value D lies in -interior <= D <= exterior (world units, +inf allowed), ascending, and those values bit
// for bit.  Two calls: the count, then the fill.
struct NarrowBand {
  std::vector<uint64_t> cells;      // grid order (Grid::get_cell_idx), ascending
  std::vector<float> distances;     // distances[n] = the dense value at cells[n]
  std::vector<uint32_t> bits;       // the active set in the layout of Voxels::bits; empty unless asked for
  uint64_t count = 0;
};
template <class V, class I = uint32_t>
NarrowBand narrow_band_sdf(const std::vector<V>& vertices, const Topology<I>& indices, const Grid<V>& grid, float interior, float exterior,
                           SignMethod sign_method = SignMethod::Raycast, bool bits = false) {
  detail::Packed<V> v(vertices.data(), vertices.size());
  detail::IndexArg<I> ia(indices);
  NarrowBand r;
  const m2s_band_opts bo = {sizeof(m2s_band_opts), exterior, interior};
  detail::check(m2s_narrow_band_sdf(v.ptr, vertices.size(), ia.ptr, indices.count, ia.bytes, indices.kind, &grid.raw(), (int)sign_method, &bo, nullptr,
                                    nullptr, 0, nullptr, &r.count, nullptr));
  const auto n = grid.get_cell_count();
  r.cells.resize(r.count);
  r.distances.resize(r.count);
  if (bits) r.bits.resize(n[0] * n[1] * ((n[2] + 31) / 32));
  if (r.count == 0 && !bits) return r;
  detail::check(m2s_narrow_band_sdf(v.ptr, vertices.size(), ia.ptr, indices.count, ia.bytes, indices.kind, &grid.raw(), (int)sign_method, &bo,
                                    r.count ? r.cells.data() : nullptr, r.count ? r.distances.data() : nullptr, r.count,
                                    r.bits.empty() ? nullptr : r.bits.data(), &r.count, nullptr));
  return r;
}

// ---- queries on a finished grid (m2s_sample_grid, m2s_raymarch_grid) ------------------------------------------------------
// The reference client's shader (draw_raymarching.wgsl: sdf_grid, estimate_normal, sdf_3d) over `distances`, the grid's cells in grid
// order (what generate_grid_sdf returns).  Host memory: every call copies the grid to the device (m2s.h says when that matters).
enum class SampleMode : int32_t { Snap = M2S_SAMPLE_SNAP, Trilinear = M2S_SAMPLE_TRILINEAR, Tetrahedral = M2S_SAMPLE_TETRAHEDRAL };
struct SampleOptions {
  SampleMode mode = SampleMode::Trilinear;
  float iso = 0.0f;
  float outside = 100.0f;
  uint32_t max_steps = 100;   // raymarch_grid only
};
struct GridSamples {
  std::vector<float> value;
  std::vector<std::array<float, 3>> normal;   // empty unless asked for
};
struct RayMarch {
  std::vector<std::array<float, 4>> hit;      // position, distance
  std::vector<uint32_t> steps;
  std::vector<std::array<float, 3>> normal;   // empty unless asked for
};
namespace detail {
template <class V>
void check_cells(const Grid<V>& grid, size_t n) {
  if (n != grid.get_total_cell_count()) throw Panic(M2S_ERR_BAD_ARG, "distances do not match the grid's cell count");
}
inline m2s_sample_opts sample_opts(const SampleOptions& o) {
  m2s_sample_opts s{};
  s.struct_size = sizeof(s);
  s.mode = (int32_t)o.mode;
  s.iso = o.iso;
  s.outside = o.outside;
  s.max_steps = o.max_steps;
  return s;
}
}  // namespace detail
template <class V>
GridSamples sample_grid(const Grid<V>& grid, const std::vector<float>& distances, const std::vector<V>& points, const SampleOptions& options = {},
                        bool normals = false) {
  detail::check_cells(grid, distances.size());
  detail::Packed<V> p(points.data(), points.size());
  const m2s_sample_opts so = detail::sample_opts(options);
  GridSamples r;
  r.value.resize(points.size());
  if (normals) r.normal.resize(points.size());
  detail::check(m2s_sample_grid(&grid.raw(), distances.data(), p.ptr, points.size(), &so, r.value.data(),
                                normals ? reinterpret_cast<float*>(r.normal.data()) : nullptr, nullptr));
  return r;
}
template <class V>
RayMarch raymarch_grid(const Grid<V>& grid, const std::vector<float>& distances, const std::vector<V>& origins, const std::vector<V>& directions,
                       const SampleOptions& options = {}, bool normals = false) {
  detail::check_cells(grid, distances.size());
  if (origins.size() != directions.size()) throw Panic(M2S_ERR_BAD_ARG, "origins and directions differ in length");
  detail::Packed<V> o(origins.data(), origins.size()), d(directions.data(), directions.size());
  const m2s_sample_opts so = detail::sample_opts(options);
  RayMarch r;
  r.hit.resize(origins.size());
  r.steps.resize(origins.size());
  if (normals) r.normal.resize(origins.size());
  detail::check(m2s_raymarch_grid(&grid.raw(), distances.data(), o.ptr, d.ptr, origins.size(), &so, reinterpret_cast<float*>(r.hit.data()), r.steps.data(),
                                  normals ? reinterpret_cast<float*>(r.normal.data()) : nullptr, nullptr));
  return r;
}

// ---- isosurface of a finished grid (m2s_grid_isosurface) ------------------------------------------------------------------
// The level set d = iso of `distances` (the grid's cells in grid order) as a welded, indexed mesh: indices are 3 per triangle,
// wound outwards (towards increasing d).  m2s.h states the exact contract.
template <class V>
struct Isosurface {
  std::vector<V> vertices;
  std::vector<uint32_t> indices;
};
template <class V>
Isosurface<V> grid_isosurface(const Grid<V>& grid, const std::vector<float>& distances, float iso = 0.0f) {
  detail::check_cells(grid, distances.size());
  uint64_t counts[2] = {0, 0};
  detail::check(m2s_grid_isosurface(&grid.raw(), distances.data(), iso, nullptr, 0, nullptr, 0, counts, nullptr));
  std::vector<float> v(3 * counts[0] + 3);   // never empty: two NULL outputs would mean "count only"
  Isosurface<V> r;
  r.indices.resize(3 * counts[1] + 3);
  detail::check(m2s_grid_isosurface(&grid.raw(), distances.data(), iso, v.data(), counts[0], r.indices.data(), counts[1], counts, nullptr));
  r.indices.resize(3 * counts[1]);
  r.vertices.reserve(counts[0]);
  for (uint64_t i = 0; i < counts[0]; ++i) r.vertices.push_back(detail::make_point<V>(v[3 * i], v[3 * i + 1], v[3 * i + 2]));
  return r;
}

// ---- isosurface of a narrow band (m2s_band_isosurface) --------------------------------------------------------------------
// The same level set from the band's own cells (strictly ascending grid-order indices) and distances: grid_isosurface of any dense
// grid that agrees with the band, kept where the band alone decides it.  n_open != 0 proves the band was too narrow for this iso
// (m2s.h: n_open); with a band of one cell diagonal either side of iso and an exact distance field the mesh is the dense call's.
template <class V>
struct BandIsosurface : Isosurface<V> {
  uint64_t n_open = 0;
};
template <class V>
BandIsosurface<V> band_isosurface(const Grid<V>& grid, const std::vector<uint64_t>& cells, const std::vector<float>& distances, float iso = 0.0f) {
  if (cells.size() != distances.size()) throw Panic(M2S_ERR_BAD_ARG, "band_isosurface: cells and distances differ in length");
  uint64_t counts[3] = {0, 0, 0};
  detail::check(m2s_band_isosurface(&grid.raw(), cells.data(), distances.data(), cells.size(), iso, nullptr, 0, nullptr, 0, counts, nullptr));
  std::vector<float> v(3 * counts[0] + 3);   // never empty: two NULL outputs would mean "count only"
  BandIsosurface<V> r;
  r.indices.resize(3 * counts[1] + 3);
  detail::check(m2s_band_isosurface(&grid.raw(), cells.data(), distances.data(), cells.size(), iso, v.data(), counts[0], r.indices.data(), counts[1],
                                    counts, nullptr));
  r.indices.resize(3 * counts[1]);
  r.vertices.reserve(counts[0]);
  for (uint64_t i = 0; i < counts[0]; ++i) r.vertices.push_back(detail::make_point<V>(v[3 * i], v[3 * i + 1], v[3 * i + 2]));
  r.n_open = counts[2];
  return r;
}

// ---- queries on a narrow band (m2s_band_create, m2s_band_sample, m2s_band_raymarch) ---------------------------------------
// A band made queryable: the index of its cells, its distances and an optional sign mask stay on the device; sample and raymarch equal
// sample_grid / raymarch_grid on the dense grid the band stands for (its values on its cells, -background_inside where `inside_bits` has
// the cell's bit, +background_outside elsewhere) bit for bit, and that grid is never made.  m2s.h states the contract.  Move-only.
struct BandSamples : GridSamples {
  std::vector<uint8_t> support;   // per point: how many of the sample's 1 / 8 / 4 cell reads hit a band cell
};
struct BandRayMarch : RayMarch {
  std::vector<uint8_t> support;   // per ray: the support of the last sample the march evaluated
};
// How BandField::csg combines two fields (m2s_csg_op); Difference is this minus the other.
enum class CsgOp : int { Union = M2S_CSG_UNION, Intersection = M2S_CSG_INTERSECTION, Difference = M2S_CSG_DIFFERENCE };
// What BandField::redistance reports (m2s_band_redistance_info): the sweeps that changed a value, whether the last one run changed none,
// the frozen cells next to the zero set, the sign changes towards an inactive cell (> 0: the band does not bracket its zero set there),
// the candidate cells the sweeps ran over.
struct RedistanceInfo {
  uint32_t sweeps = 0;
  bool converged = false;
  uint64_t n_frozen = 0, n_open = 0, n_candidates = 0;
};
// What BandField::filter runs (m2s_filter_kind): the separable 3 x 3 x 3 box (four iterations approximate a Gaussian), one explicit step of
// the heat equation, one explicit step of the mean-curvature flow.
enum class FilterKind : int { Mean = M2S_FILTER_MEAN, Laplacian = M2S_FILTER_LAPLACIAN, MeanCurvature = M2S_FILTER_MEAN_CURVATURE };
// What BandField::filter reports (m2s_band_filter_info): the passes run, the largest |result - input| over the cells, the cells whose bits
// changed, the cells whose sign changed, the candidates that were not finite and were dropped (per cell and pass).
struct FilterInfo {
  uint32_t passes = 0;
  float max_change = 0.0f;
  uint64_t n_changed = 0, n_sign_flips = 0, n_nonfinite = 0;
};
// What BandField::advect steps (m2s_advect_kind): the field carried along a velocity per cell (phi_t + u . grad phi = 0), or the surface moved
// along its normal by a speed per cell (phi_t + F |grad phi| = 0).
enum class AdvectKind : int { Velocity = M2S_ADVECT_VELOCITY, Normal = M2S_ADVECT_NORMAL };
// What BandField::advect reports (m2s_band_advect_info): the steps run, the largest |result - input| over the cells, the largest CFL number
// of a cell (stable up to 1; reported, not enforced), the cells with a field entry other than zero, the cells whose bits changed, the cells
// whose sign changed, the candidates that were not finite and were dropped (per cell and step).
struct AdvectInfo {
  uint32_t steps = 0;
  float max_change = 0.0f, max_cfl = 0.0f;
  uint64_t n_moving = 0, n_changed = 0, n_sign_flips = 0, n_nonfinite = 0;
};
// What BandField::resample reports (m2s_band_resample_info): the result's cells, the points on the source box with some but not all of
// their reads in the band (the rim the interpolation loses), the points whose value came out non-finite and were dropped, the sign changes
// towards an inactive cell (> 0: the result does not bracket its zero set there).
struct ResampleInfo {
  uint64_t n_cells = 0, n_partial = 0, n_nonfinite = 0, n_open = 0;
};
// Which cells of a band count as joined (m2s_connectivity): faces, faces and edges, faces, edges and corners.
enum class Connectivity : int { Faces = M2S_CONNECT_6, Edges = M2S_CONNECT_18, Corners = M2S_CONNECT_26 };
// What BandField::components returns (m2s_band_components): the components numbered in ascending order of their smallest cell index (the
// raster numbering of scipy.ndimage.label); labels[r] is the component of the r-th cell of export_band().cells; components[c] holds its
// first cell, cell count, negative-cell count (a volume proxy) and inclusive (i, j, k) bounding box.
struct Components {
  std::vector<uint32_t> labels;
  std::vector<m2s_band_component> components;
  uint64_t count() const { return components.size(); }
  // The numbers of the k components with the most cells, largest first; a tie goes to the lower number.
  std::vector<uint32_t> largest(size_t k = 1) const {
    std::vector<uint32_t> order(components.size());
    for (size_t c = 0; c < order.size(); ++c) order[c] = (uint32_t)c;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return components[a].n_cells > components[b].n_cells; });
    order.resize(std::min(k, order.size()));
    return order;
  }
};
// What BandField::select reports (m2s_band_select_info): the result's cells, the cells erased, the inactive points whose inside bit was
// cleared because erased cells bracketed them.
struct SelectInfo {
  uint64_t n_cells = 0, n_dropped = 0, n_sign_cleared = 0;
};
// What BandField::measure returns (m2s_band_measure_record): the level set measured as band_isosurface would mesh it.  The counts, the
// raw integer sums the C header defines to the bit, and area, volume and centroid in world units.
struct Measure : m2s_band_measure_record {
  // Only a closed surface has a volume and a centre of mass; otherwise volume and centroid are the defined sums and depend on the origin.
  bool closed() const { return n_open == 0 && n_border == 0; }
  // The Euler characteristic of a closed surface: 2 for a sphere, 0 for a torus.
  int64_t euler() const { return (int64_t)n_vertices - (int64_t)(n_triangles / 2); }
};
// What BandField::from_capsules reports (m2s_band_shapes_info): the result's cells, the grid points inside the union, the shapes left out
// (a non-finite coordinate or radius, a negative radius) and the sound shapes that reach no grid point within the exterior width.
struct ShapesInfo : m2s_band_shapes_info {};
template <class V>
class BandField {
 public:
  // inside_bits: empty, or uint32[nx][ny][ceil(nz / 32)] (voxelize(solid) / narrow_band_sdf bits)
  BandField(const Grid<V>& grid, const std::vector<uint64_t>& cells, const std::vector<float>& distances, float background_outside,
            float background_inside, const std::vector<uint32_t>& inside_bits = {})
      : grid_(grid) {
    if (cells.size() != distances.size()) throw Panic(M2S_ERR_BAD_ARG, "BandField: cells and distances differ in length");
    const auto n = grid.get_cell_count();
    if (!inside_bits.empty() && inside_bits.size() != (size_t)(n[0] * n[1] * ((n[2] + 31) / 32)))
      throw Panic(M2S_ERR_BAD_ARG, "BandField: inside_bits do not match the grid");
    m2s_band_field_opts fo{};
    fo.struct_size = sizeof(fo);
    fo.background_outside = background_outside;
    fo.background_inside = background_inside;
    detail::check(m2s_band_create(&grid.raw(), cells.data(), distances.data(), cells.size(), inside_bits.empty() ? nullptr : inside_bits.data(), &fo,
                                  nullptr, &h_));
  }
  BandField(const BandField&) = delete;
  BandField& operator=(const BandField&) = delete;
  BandField(BandField&& o) noexcept : grid_(o.grid_), h_(o.h_) { o.h_ = nullptr; }
  BandField& operator=(BandField&& o) noexcept {
    if (this != &o) {
      m2s_band_destroy(h_);
      grid_ = o.grid_;
      h_ = o.h_;
      o.h_ = nullptr;
    }
    return *this;
  }
  ~BandField() { m2s_band_destroy(h_); }

  const Grid<V>& grid() const { return grid_; }
  uint64_t count() const { return info(0); }
  uint64_t device_bytes() const { return info(1); }
  m2s_band* raw() const { return h_; }

  BandSamples sample(const std::vector<V>& points, const SampleOptions& options = {}, bool normals = false) const {
    detail::Packed<V> p(points.data(), points.size());
    const m2s_sample_opts so = detail::sample_opts(options);
    BandSamples r;
    r.value.resize(points.size());
    r.support.resize(points.size());
    if (normals) r.normal.resize(points.size());
    detail::check(m2s_band_sample(h_, p.ptr, points.size(), &so, r.value.data(), normals ? reinterpret_cast<float*>(r.normal.data()) : nullptr,
                                  r.support.data(), nullptr));
    return r;
  }
  BandRayMarch raymarch(const std::vector<V>& origins, const std::vector<V>& directions, const SampleOptions& options = {}, bool normals = false) const {
    if (origins.size() != directions.size()) throw Panic(M2S_ERR_BAD_ARG, "origins and directions differ in length");
    detail::Packed<V> o(origins.data(), origins.size()), d(directions.data(), directions.size());
    const m2s_sample_opts so = detail::sample_opts(options);
    BandRayMarch r;
    r.hit.resize(origins.size());
    r.steps.resize(origins.size());
    r.support.resize(origins.size());
    if (normals) r.normal.resize(origins.size());
    detail::check(m2s_band_raymarch(h_, o.ptr, d.ptr, origins.size(), &so, reinterpret_cast<float*>(r.hit.data()), r.steps.data(),
                                    normals ? reinterpret_cast<float*>(r.normal.data()) : nullptr, r.support.data(), nullptr));
    return r;
  }

  // The union, intersection or difference of two fields on the same grid as a new resident field (m2s_band_csg: min / max of the grids
  // the bands stand for, per grid point and to the bit; no dense grid, nothing leaves the device).  Without backgrounds the result takes
  // the smaller of the operands' on each side.  The zero set is the combined solid's; the values are a lower bound of its distance.
  BandField csg(const BandField& other, CsgOp op) const { return csg_as(other, op, nullptr); }
  BandField csg(const BandField& other, CsgOp op, float background_outside, float background_inside) const {
    m2s_band_field_opts fo{};
    fo.struct_size = sizeof(fo);
    fo.background_outside = background_outside;
    fo.background_inside = background_inside;
    return csg_as(other, op, &fo);
  }
  // The field with the same zero set, values that are distances again and the half-widths asked for, as a new resident field
  // (m2s_band_redistance: Jacobi sweeps of the first-order update from the cells next to the zero set, per grid point and to the bit;
  // no dense grid).  The cells next to the zero set keep their values in every bit; the backgrounds become the two widths.
  BandField redistance(float exterior, float interior, uint32_t max_sweeps = 0, RedistanceInfo* info = nullptr) const {
    m2s_band_redistance_opts ro{};
    ro.struct_size = sizeof(ro);
    ro.exterior = exterior;
    ro.interior = interior;
    ro.max_sweeps = max_sweeps;
    m2s_band_redistance_info ri{};
    ri.struct_size = sizeof(ri);
    m2s_band* h = nullptr;
    detail::check(m2s_band_redistance(h_, &ro, nullptr, nullptr, &h, &ri));
    if (info) {
      info->sweeps = ri.sweeps;
      info->converged = ri.converged != 0;
      info->n_frozen = ri.n_frozen;
      info->n_open = ri.n_open;
      info->n_candidates = ri.n_candidates;
    }
    return BandField(grid_, h);
  }
  // The field on the same cells with its values smoothed by `iterations` iterations of `kind`, as a new resident field (m2s_band_filter:
  // Jacobi passes over the band's cells, per grid point and to the bit; no dense grid).  where: a field on the same grid whose inside is the
  // region to smooth; the cells outside it keep every bit.  The backgrounds are kept.  The result is not a distance field: follow it
  // with redistance.
  BandField filter(FilterKind kind, uint32_t iterations = 1, const BandField* where = nullptr, FilterInfo* info = nullptr) const {
    m2s_band_filter_opts fl{};
    fl.struct_size = sizeof(fl);
    fl.kind = (int32_t)kind;
    fl.iterations = iterations;
    fl.width = 1;
    m2s_band_filter_info fi{};
    fi.struct_size = sizeof(fi);
    m2s_band* h = nullptr;
    detail::check(m2s_band_filter(h_, where ? where->h_ : nullptr, &fl, nullptr, nullptr, &h, &fi));
    if (info) {
      info->passes = fi.passes;
      info->max_change = fi.max_change;
      info->n_changed = fi.n_changed;
      info->n_sign_flips = fi.n_sign_flips;
      info->n_nonfinite = fi.n_nonfinite;
    }
    return BandField(grid_, h);
  }
  // The field on the same cells after `steps` first-order upwind steps of dt, as a new resident field (m2s_band_advect: Jacobi steps over
  // the band's cells, per grid point and to the bit; no dense grid).  field: one entry per cell in the order of export_band().cells, three
  // floats (AdvectKind::Velocity) or one (AdvectKind::Normal); a cell whose entry is zero keeps every bit.  The backgrounds are kept.  The
  // result is not a distance field and the band does not follow the surface: move it by less than the half-width minus two cells, then
  // redistance.  info->max_cfl should stay at or below 1.
  BandField advect(AdvectKind kind, const std::vector<float>& field, float dt, uint32_t steps = 1, AdvectInfo* info = nullptr) const {
    if (field.size() != count() * (kind == AdvectKind::Velocity ? 3 : 1)) throw Panic(M2S_ERR_BAD_ARG, "advect: field does not hold one entry per cell");
    m2s_band_advect_opts ao{};
    ao.struct_size = sizeof(ao);
    ao.kind = (int32_t)kind;
    ao.steps = steps;
    ao.dt = dt;
    m2s_band_advect_info ai{};
    ai.struct_size = sizeof(ai);
    m2s_band* h = nullptr;
    detail::check(m2s_band_advect(h_, field.empty() ? nullptr : field.data(), &ao, nullptr, nullptr, &h, &ai));
    if (info) {
      info->steps = ai.steps;
      info->max_change = ai.max_change;
      info->max_cfl = ai.max_cfl;
      info->n_moving = ai.n_moving;
      info->n_changed = ai.n_changed;
      info->n_sign_flips = ai.n_sign_flips;
      info->n_nonfinite = ai.n_nonfinite;
    }
    return BandField(grid_, h);
  }
  // The field evaluated at the cell centres of another grid, as a new resident field on that grid (m2s_band_resample, per target grid
  // point and to the bit; no dense grid): crop, pad, move, turn, scale, refine.  to_source: 12 floats, the row-major 3 x 4 map from TARGET
  // space to SOURCE space (the inverse of the placement; nullptr is the identity); the library inverts nothing.  value_scale: the
  // placement's uniform scale, which the values are multiplied by; the backgrounds are this field's times it.  After an interpolating mode
  // the result is not a distance field: follow it with redistance.
  BandField resample(const Grid<V>& target, const float* to_source = nullptr, float value_scale = 1.0f, SampleMode mode = SampleMode::Trilinear, ResampleInfo* info = nullptr) const {
    m2s_band_resample_opts ro{};
    ro.struct_size = sizeof(ro);
    ro.mode = (int32_t)mode;
    for (int a = 0; a < 12; ++a) ro.to_source[a] = to_source ? to_source[a] : (a % 5 == 0 ? 1.0f : 0.0f);
    ro.value_scale = value_scale;
    m2s_band_resample_info ri{};
    ri.struct_size = sizeof(ri);
    m2s_band* h = nullptr;
    detail::check(m2s_band_resample(h_, &target.raw(), &ro, nullptr, nullptr, &h, &ri));
    if (info) {
      info->n_cells = ri.n_cells;
      info->n_partial = ri.n_partial;
      info->n_nonfinite = ri.n_nonfinite;
      info->n_open = ri.n_open;
    }
    return BandField(target, h);
  }
  // The connected components of the field's cells (m2s_band_components: a lock-free union-find on the device, to the bit).  One
  // labelling, with room for 256 components; a second only when there are more (the call then reports the count and fills nothing).
  Components components(Connectivity connectivity = Connectivity::Faces) const {
    m2s_band_components_opts co{};
    co.struct_size = sizeof(co);
    co.connectivity = (int32_t)connectivity;
    Components r;
    r.labels.resize(count());
    r.components.resize(256);
    uint64_t n = 0;
    const int rc = m2s_band_components(h_, &co, nullptr, r.labels.data(), r.components.data(), r.components.size(), &n);
    if (rc == M2S_ERR_BAD_ARG && n > r.components.size()) {
      r.components.resize(n);
      detail::check(m2s_band_components(h_, &co, nullptr, r.labels.data(), r.components.data(), n, &n));
    } else {
      detail::check(rc);
    }
    r.components.resize(n);
    return r;
  }
  // The field with some components erased, as a new resident field (m2s_band_select): a cell is kept iff keep[labels[r]] != 0 (a label
  // beyond keep, M2S_LABEL_NONE included, erases it).  The kept cells keep every bit; an erased cell becomes inactive and outside, and so
  // does the solid interior that only erased cells bracketed along k.  Erase islands, not voids: erasing the band around a cavity
  // leaves the solid around it without a band cell on that side.  The backgrounds are kept.
  BandField select(const std::vector<uint32_t>& labels, const std::vector<uint8_t>& keep, SelectInfo* info = nullptr) const {
    if (labels.size() != count()) throw Panic(M2S_ERR_BAD_ARG, "select: one label per cell");
    static const uint32_t none = M2S_LABEL_NONE;
    m2s_band_select_info si{};
    si.struct_size = sizeof(si);
    m2s_band* h = nullptr;
    detail::check(m2s_band_select(h_, labels.empty() ? &none : labels.data(), keep.empty() ? nullptr : keep.data(), keep.size(), nullptr, nullptr, &h, &si));
    if (info) {
      info->n_cells = si.n_cells;
      info->n_dropped = si.n_dropped;
      info->n_sign_cleared = si.n_sign_cleared;
    }
    return BandField(grid_, h);
  }
  // The field with all but its k largest components erased.
  BandField keep_largest(size_t k = 1, Connectivity connectivity = Connectivity::Faces, SelectInfo* info = nullptr) const {
    const Components c = components(connectivity);
    std::vector<uint8_t> keep(c.count(), 0);
    for (uint32_t id : c.largest(k)) keep[id] = 1;
    return select(c.labels, keep, info);
  }
  // The level set d = iso measured without a mesh (m2s_band_measure): triangle and vertex counts, area, enclosed volume, centroid.
  Measure measure(float iso = 0.0f) const {
    m2s_band_measure_opts mo{};
    mo.struct_size = sizeof(mo);
    mo.iso = iso;
    Measure r{};
    detail::check(m2s_band_measure(h_, &mo, nullptr, 0, nullptr, &r, nullptr, nullptr));
    return r;
  }
  // One Measure per group: a cell belongs to the group labels[r] of its base corner (Components::labels with count() groups; label with
  // Connectivity::Corners to measure per mesh component); a label of n_groups or more, M2S_LABEL_NONE included, leaves the cell out.
  std::vector<Measure> measure(const std::vector<uint32_t>& labels, uint64_t n_groups, float iso = 0.0f) const {
    if (labels.size() != count()) throw Panic(M2S_ERR_BAD_ARG, "measure: one label per cell");
    static const uint32_t none = M2S_LABEL_NONE;
    m2s_band_measure_opts mo{};
    mo.struct_size = sizeof(mo);
    mo.iso = iso;
    std::vector<Measure> r(n_groups);
    static_assert(sizeof(Measure) == sizeof(m2s_band_measure_record), "Measure adds no data to the record");
    detail::check(m2s_band_measure(h_, &mo, labels.empty() ? &none : labels.data(), n_groups, nullptr, r.data(), nullptr, nullptr));
    return r;
  }
  std::vector<Measure> measure(const Components& c, float iso = 0.0f) const { return measure(c.labels, c.count(), iso); }
  // The field's lists back out (m2s_band_export): cells ascending, distances bit for bit, and `bits` the sign mask in the layout of
  // Voxels::bits (all zero for a field made without one).  band_isosurface(grid, b.cells, b.distances) meshes it.
  NarrowBand export_band() const {
    NarrowBand r;
    r.count = count();
    const auto n = grid_.get_cell_count();
    r.cells.resize(r.count);
    r.distances.resize(r.count);
    r.bits.resize(n[0] * n[1] * ((n[2] + 31) / 32));
    detail::check(m2s_band_export(h_, r.count ? r.cells.data() : nullptr, r.count ? r.distances.data() : nullptr, r.count, r.bits.data(), nullptr));
    return r;
  }
  // The union of the capsules a[n]-b[n] with the radii radius[n] as a resident field, with no mesh (m2s_band_from_capsules: the smallest
  // distance to a capsule's surface per grid point and to the bit, active within the half-widths, a sign mask on every point).  b empty:
  // spheres.  radius: one per shape, or a single value for all.  The backgrounds are the two widths.  Inside the union the values are a
  // lower bound of the depth: redistance makes distances of them.
  static BandField from_capsules(const Grid<V>& grid, const std::vector<V>& a, const std::vector<V>& b, const std::vector<float>& radius, float exterior,
                                 float interior, ShapesInfo* info = nullptr) {
    if (!b.empty() && b.size() != a.size()) throw Panic(M2S_ERR_BAD_ARG, "from_capsules: a and b differ in length");
    if (radius.size() != a.size() && radius.size() != 1) throw Panic(M2S_ERR_BAD_ARG, "from_capsules: one radius per shape, or one for all");
    detail::Packed<V> pa(a.data(), a.size()), pb(b.data(), b.size());
    m2s_band_shapes_opts so{};
    so.struct_size = sizeof(so);
    so.exterior = exterior;
    so.interior = interior;
    const bool one = radius.size() == 1 && a.size() != 1;
    so.radius = one ? radius[0] : 0.0f;
    ShapesInfo si{};
    m2s_band* h = nullptr;
    detail::check(m2s_band_from_capsules(&grid.raw(), pa.ptr, b.empty() ? nullptr : pb.ptr, one ? nullptr : radius.data(), a.size(), &so, nullptr, nullptr, &h,
                                         &si, nullptr));
    if (info) *info = si;
    return BandField(grid, h);
  }
  static BandField from_spheres(const Grid<V>& grid, const std::vector<V>& centers, const std::vector<float>& radius, float exterior, float interior,
                                ShapesInfo* info = nullptr) {
    return from_capsules(grid, centers, {}, radius, exterior, interior, info);
  }
  float background_outside() const { return field_info().background_outside; }
  float background_inside() const { return field_info().background_inside; }

 private:
  BandField(const Grid<V>& grid, m2s_band* h) : grid_(grid), h_(h) {}
  BandField csg_as(const BandField& other, CsgOp op, const m2s_band_field_opts* fo) const {
    m2s_band* h = nullptr;
    detail::check(m2s_band_csg(h_, other.h_, (int)op, fo, nullptr, &h));
    return BandField(grid_, h);
  }
  m2s_band_field_opts field_info() const {
    m2s_band_field_opts fo{};
    detail::check(m2s_band_field_info(h_, &fo, nullptr));
    return fo;
  }
  uint64_t info(int which) const {
    uint64_t n = 0, bytes = 0;
    detail::check(m2s_band_info(h_, nullptr, &n, &bytes));
    return which ? bytes : n;
  }
  Grid<V> grid_;
  m2s_band* h_ = nullptr;
};

// ---- serde (serde.rs:75-221) ----------------------------------------------------------------------------------------------
namespace serde {
enum class SerdeErrorKind { SerializationFailed, DeserializationFailed, IoError };
struct SerdeError : Error {
  SerdeErrorKind kind;
  SerdeError(int c, const std::string& m)
      : Error(c, m), kind(c == M2S_ERR_IO ? SerdeErrorKind::IoError
                          : m.rfind("Serialization", 0) == 0 ? SerdeErrorKind::SerializationFailed : SerdeErrorKind::DeserializationFailed) {}
};
inline void check(int rc) { if (rc != M2S_OK) throw SerdeError(rc, m2s_last_error()); }

template <class V> struct SerializeGeneric { const V* query_points; size_t n_queries; const float* distances; size_t n_distances; };
template <class V> struct SerializeGrid { const Grid<V>* grid; const float* distances; size_t n_distances; };
template <class V> using SerializeSdf = std::variant<SerializeGeneric<V>, SerializeGrid<V>>;

template <class V> struct DeserializeGeneric { std::vector<V> query_points; std::vector<float> distances; };
template <class V> struct DeserializeGrid { Grid<V> grid; std::vector<float> distances; };
template <class V> using DeserializeSdf = std::variant<DeserializeGeneric<V>, DeserializeGrid<V>>;

template <class V>
std::vector<uint8_t> serialize(const SerializeSdf<V>& sdf) {   // serde.rs:161-166
  std::vector<uint8_t> out;
  size_t written = 0;
  if (const auto* g = std::get_if<SerializeGrid<V>>(&sdf)) {
    out.resize(m2s_sdf_grid_encoded_size(&g->grid->raw(), g->n_distances));
    if (out.empty()) throw SerdeError(M2S_ERR_BAD_ARG, "SerializationFailed");
    check(m2s_sdf_encode_grid(&g->grid->raw(), g->distances, g->n_distances, out.data(), out.size(), &written, nullptr));
  } else {
    const auto& q = std::get<SerializeGeneric<V>>(sdf);
    detail::Packed<V> pts(q.query_points, q.n_queries);
    out.resize(m2s_sdf_generic_encoded_size(q.n_queries, q.n_distances));
    if (out.empty()) throw SerdeError(M2S_ERR_BAD_ARG, "SerializationFailed");
    check(m2s_sdf_encode_generic(pts.ptr, q.n_queries, q.distances, q.n_distances, out.data(), out.size(), &written, nullptr));
  }
  out.resize(written);
  return out;
}

namespace detail_serde {
template <class V>
DeserializeSdf<V> finish(const m2s_sdf_info& info, std::vector<float>&& q, std::vector<float>&& d) {
  if (info.kind == M2S_SDF_GRID) return DeserializeGrid<V>{Grid<V>::from_raw(info.grid), std::move(d)};
  DeserializeGeneric<V> g;
  g.query_points.reserve(info.n_queries);
  for (uint64_t i = 0; i < info.n_queries; ++i) g.query_points.push_back(mesh_to_sdf::detail::make_point<V>(q[3 * i], q[3 * i + 1], q[3 * i + 2]));
  g.distances = std::move(d);
  return g;
}
}  // namespace detail_serde

template <class V>
DeserializeSdf<V> deserialize(const uint8_t* data, size_t n) {   // serde.rs:169-176
  m2s_sdf_info info;
  check(m2s_sdf_probe(data, n, &info, nullptr));
  std::vector<float> q(3 * info.n_queries), d(info.n_distances);
  check(m2s_sdf_decode(data, n, q.data(), d.data(), nullptr));
  return detail_serde::finish<V>(info, std::move(q), std::move(d));
}
template <class V> DeserializeSdf<V> deserialize(const std::vector<uint8_t>& data) { return deserialize<V>(data.data(), data.size()); }

template <class V>
void save_to_file(const SerializeSdf<V>& sdf, const std::string& path) {   // serde.rs:192-198
  if (const auto* g = std::get_if<SerializeGrid<V>>(&sdf)) {
    check(m2s_sdf_save_grid(path.c_str(), &g->grid->raw(), g->distances, g->n_distances, nullptr));
  } else {
    const auto& q = std::get<SerializeGeneric<V>>(sdf);
    mesh_to_sdf::detail::Packed<V> pts(q.query_points, q.n_queries);
    check(m2s_sdf_save_generic(path.c_str(), pts.ptr, q.n_queries, q.distances, q.n_distances, nullptr));
  }
}

template <class V>
DeserializeSdf<V> read_from_file(const std::string& path) {   // serde.rs:216-220
  m2s_sdf_info info;
  check(m2s_sdf_probe_file(path.c_str(), &info));
  std::vector<float> q(3 * info.n_queries), d(info.n_distances);
  check(m2s_sdf_read_file(path.c_str(), q.data(), d.data(), nullptr));
  return detail_serde::finish<V>(info, std::move(q), std::move(d));
}
}  // namespace serde

}  // namespace mesh_to_sdf
