// BandField::from_capsules / from_spheres of include/mesh_to_sdf.hpp (C++17, -Wall -Werror).  With no arguments it only exercises what is
// decided without a device: the types, and the C call's answers to bad arguments.  With an argument (anything) it runs on the GPU, on a
// 16 x 16 x 16 grid of unit cells with centres at the integers: two balls of radius 2 about (4, 4, 4) and (11, 11, 11) (two components,
// each a closed surface), and a strut between them that joins them into one.  Prints "all checks passed".
#include <array>
#include <cmath>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "mesh_to_sdf.hpp"

using V = std::array<float, 3>;
using Field = mesh_to_sdf::BandField<V>;
using mesh_to_sdf::Connectivity;
using mesh_to_sdf::ShapesInfo;

int main(int argc, char**) {
  static_assert(std::is_base_of<m2s_band_shapes_info, ShapesInfo>::value && sizeof(ShapesInfo) == 32 && sizeof(m2s_band_shapes_opts) == 16, "the structs' sizes");
  int failures = 0;
  const auto grid = mesh_to_sdf::Grid<V>::new_({0.0f, 0.0f, 0.0f}, {1.0f, 1.0f, 1.0f}, {16, 16, 16});
  if (argc == 1) {
    m2s_band_shapes_opts so{};
    so.struct_size = sizeof(so);
    so.exterior = so.interior = 1.0f;
    const float a[3] = {1, 2, 3};
    m2s_band* h = nullptr;
    if (m2s_band_from_capsules(&grid.raw(), a, nullptr, nullptr, 1, &so, nullptr, nullptr, nullptr, nullptr, nullptr) != M2S_ERR_BAD_ARG) ++failures;
    if (m2s_band_from_capsules(&grid.raw(), nullptr, nullptr, nullptr, 1, &so, nullptr, nullptr, &h, nullptr, nullptr) != M2S_ERR_BAD_ARG) ++failures;
    so.interior = -1.0f;
    if (m2s_band_from_capsules(&grid.raw(), a, nullptr, nullptr, 1, &so, nullptr, nullptr, &h, nullptr, nullptr) != M2S_ERR_BAD_ARG) ++failures;
    bool threw = false;
    try { (void)Field::from_capsules(grid, {V{1, 1, 1}, V{2, 2, 2}}, {V{1, 1, 1}}, {1.0f}, 1.0f, 1.0f); } catch (const mesh_to_sdf::Error&) { threw = true; }
    if (!threw) ++failures;
    threw = false;
    try { (void)Field::from_spheres(grid, {V{1, 1, 1}, V{2, 2, 2}, V{3, 3, 3}}, {1.0f, 2.0f}, 1.0f, 1.0f); } catch (const mesh_to_sdf::Error&) { threw = true; }
    if (!threw) ++failures;
  } else {
    ShapesInfo si;
    const std::vector<V> centres = {V{4, 4, 4}, V{11, 11, 11}, V{NAN, 0, 0}};
    const Field balls = Field::from_spheres(grid, centres, {2.0f}, 2.0f, 2.0f, &si);
    // a ball of radius 2 about an integer point holds the 27 points with i^2 + j^2 + k^2 <= 3; those with 4 lie on its surface (d = 0, not inside)
    if (si.n_skipped != 1 || si.n_off_grid != 0 || si.n_inside != 2 * 27 || si.n_cells != balls.count() || balls.count() == 0) ++failures;
    if (balls.background_outside() != 2.0f || balls.background_inside() != 2.0f) ++failures;
    if (balls.components(Connectivity::Corners).count() != 2) ++failures;
    const mesh_to_sdf::Measure m = balls.measure();
    if (!m.closed() || m.euler() != 4 || !(m.volume > 0.0)) ++failures;
    const auto band = balls.export_band();
    uint64_t wrong = 0;
    for (size_t c = 0; c < band.cells.size(); ++c) {
      const float i = (float)(band.cells[c] / 256), j = (float)(band.cells[c] / 16 % 16), k = (float)(band.cells[c] % 16);
      const float d0 = std::sqrt(((i - 4) * (i - 4) + (j - 4) * (j - 4)) + (k - 4) * (k - 4)) - 2.0f;
      const float d1 = std::sqrt(((i - 11) * (i - 11) + (j - 11) * (j - 11)) + (k - 11) * (k - 11)) - 2.0f;
      wrong += band.distances[c] != std::fmin(d0, d1);
    }
    if (wrong) ++failures;
    // the strut joins them; per-shape radii
    const Field strut = Field::from_capsules(grid, {V{4, 4, 4}, V{11, 11, 11}, V{4, 4, 4}}, {V{4, 4, 4}, V{11, 11, 11}, V{11, 11, 11}}, {2.0f, 2.0f, 1.0f}, 2.0f, 2.0f, &si);
    if (si.n_skipped != 0 || strut.components(Connectivity::Corners).count() != 1 || strut.count() <= balls.count()) ++failures;
    const mesh_to_sdf::Measure ms = strut.measure();
    if (!ms.closed() || ms.euler() != 2 || !(ms.volume > m.volume)) ++failures;
    // the balls cut out of the strut's union leave nothing inside where they were
    const Field cut = strut.csg(balls, mesh_to_sdf::CsgOp::Difference);
    if (cut.count() == 0) ++failures;
  }
  std::printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
