// BandField::csg / export_band of include/mesh_to_sdf.hpp (C++17, -Wall -Werror).  With no arguments it only exercises what is decided
// without a handle (no GPU needed): the types, and the C calls' answers to NULL.  With an argument (anything) it makes the band fields of
// two overlapping cubes in a 24 x 24 x 24 grid on the GPU — narrow_band_sdf three cells wide, voxelize(solid) for the sign, both
// backgrounds that width —, combines them with all three ops and checks: the export against the rules on the dense grids the bands stand
// for, point by point and to the bit, and band_isosurface of the export against grid_isosurface of the dense op, with n_open == 0.
// Prints "all checks passed".
#include <array>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "mesh_to_sdf.hpp"

using V = std::array<float, 3>;
using Field = mesh_to_sdf::BandField<V>;

static std::vector<V> cube(float cx, float cy, float cz, float h) {
  std::vector<V> v;
  for (int i = 0; i < 8; ++i) v.push_back({cx + ((i & 4) ? h : -h), cy + ((i & 2) ? h : -h), cz + ((i & 1) ? h : -h)});
  return v;
}

int main(int argc, char**) {
  static_assert((int)mesh_to_sdf::CsgOp::Union == 0 && (int)mesh_to_sdf::CsgOp::Intersection == 1 && (int)mesh_to_sdf::CsgOp::Difference == 2, "CsgOp");
  static_assert(std::is_same<decltype(std::declval<const Field&>().csg(std::declval<const Field&>(), mesh_to_sdf::CsgOp::Union)), Field>::value, "csg");
  static_assert(std::is_same<decltype(std::declval<const Field&>().csg(std::declval<const Field&>(), mesh_to_sdf::CsgOp::Union, 1.0f, 1.0f)), Field>::value,
                "csg with backgrounds");
  static_assert(std::is_same<decltype(std::declval<const Field&>().export_band()), mesh_to_sdf::NarrowBand>::value, "export_band");
  static_assert(!std::is_copy_constructible<Field>::value && std::is_move_constructible<Field>::value, "BandField is move-only");
  const std::vector<uint32_t> indices = {0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3};
  const auto topo = mesh_to_sdf::Topology<uint32_t>::TriangleList(indices);
  const auto grid = mesh_to_sdf::Grid<V>::from_bounding_box({-1.5f, -1.5f, -1.5f}, {1.5f, 1.5f, 1.5f}, {24, 24, 24});
  int failures = 0;
  if (argc == 1) {
    m2s_band* out = reinterpret_cast<m2s_band*>(&failures);
    if (m2s_band_csg(nullptr, nullptr, M2S_CSG_DIFFERENCE, nullptr, nullptr, &out) != M2S_ERR_BAD_ARG || out != nullptr) ++failures;
    if (m2s_band_csg(nullptr, nullptr, 5, nullptr, nullptr, &out) != M2S_ERR_BAD_ARG) ++failures;
    if (m2s_band_export(nullptr, nullptr, nullptr, 0, nullptr, nullptr) != M2S_ERR_BAD_ARG) ++failures;
    if (m2s_band_field_info(nullptr, nullptr, nullptr) != M2S_ERR_BAD_ARG) ++failures;
  } else {
    const size_t N = 24 * 24 * 24;
    const float h = grid.get_cell_size()[0], w = 3.0f * h;
    const std::vector<V> va = cube(-0.2f, -0.1f, 0.0f, 0.7f), vb = cube(0.3f, 0.25f, 0.2f, 0.6f);
    const auto dense_of = [&](const std::vector<V>& verts, Field* field) {
      const mesh_to_sdf::NarrowBand b = mesh_to_sdf::narrow_band_sdf(verts, topo, grid, w, w);
      const auto vox = mesh_to_sdf::voxelize(verts, topo, grid, true, true);
      *field = Field(grid, b.cells, b.distances, w, w, vox.bits);
      std::vector<float> dense(N);
      for (size_t L = 0; L < N; ++L) dense[L] = ((vox.bits[L / 24] >> (L % 24)) & 1u) ? -w : w;
      for (size_t a = 0; a < b.cells.size(); ++a) dense[b.cells[a]] = b.distances[a];
      return dense;
    };
    Field fa(grid, {}, {}, w, w), fb(grid, {}, {}, w, w);
    const std::vector<float> da = dense_of(va, &fa), db = dense_of(vb, &fb);
    for (const auto op : {mesh_to_sdf::CsgOp::Union, mesh_to_sdf::CsgOp::Intersection, mesh_to_sdf::CsgOp::Difference}) {
      const Field r = fa.csg(fb, op);
      if (r.background_outside() != w || r.background_inside() != w) ++failures;
      const mesh_to_sdf::NarrowBand e = r.export_band();
      if (e.count != r.count() || e.cells.size() != e.count || r.device_bytes() != 24ull * (N / 64) + 4ull * e.count) ++failures;
      // the dense op; the backgrounds are equal, so the result stands for it on every point (m2s.h, consequence 1)
      std::vector<float> want(N), got(N);
      for (size_t L = 0; L < N; ++L) {
        const float a = da[L], b = op == mesh_to_sdf::CsgOp::Difference ? -db[L] : db[L];
        want[L] = op == mesh_to_sdf::CsgOp::Union ? (b < a ? b : a) : (b > a ? b : a);
        got[L] = ((e.bits[L / 24] >> (L % 24)) & 1u) ? -w : w;
      }
      for (size_t a = 0; a < e.cells.size(); ++a) got[e.cells[a]] = e.distances[a];
      size_t differ = 0;
      for (size_t L = 0; L < N; ++L) differ += got[L] != want[L];
      if (differ) ++failures;
      const auto mesh = mesh_to_sdf::band_isosurface(grid, e.cells, e.distances, 0.0f);
      const auto ref = mesh_to_sdf::grid_isosurface(grid, want, 0.0f);
      if (mesh.n_open != 0 || mesh.vertices.empty() || mesh.vertices.size() != ref.vertices.size() || mesh.indices != ref.indices) ++failures;
      else if (std::memcmp(mesh.vertices.data(), ref.vertices.data(), sizeof(V) * ref.vertices.size()) != 0) ++failures;
    }
  }
  std::printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
