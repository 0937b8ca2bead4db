// BandField::measure of include/mesh_to_sdf.hpp (C++17, -Wall -Werror).  With no arguments it only exercises what is decided without a
// handle (no GPU needed): the types, and the C call's answers to NULL.  With an argument (anything) it measures on the GPU, on an 8 x 8 x 8
// grid of cells 0.5: two octahedra (one inside point among its 26 neighbours, at (2, 2, 2) and at (5, 5, 5)), whose blocks of 27 points
// touch no common cell: two components by corners, each with exact sums.  Prints "all checks passed".
#include <array>
#include <cmath>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "mesh_to_sdf.hpp"

using V = std::array<float, 3>;
using Field = mesh_to_sdf::BandField<V>;
using mesh_to_sdf::Connectivity;
using mesh_to_sdf::Measure;

int main(int argc, char**) {
  static_assert(std::is_same<decltype(std::declval<const Field&>().measure()), Measure>::value, "measure");
  static_assert(std::is_same<decltype(std::declval<const Field&>().measure(std::declval<const mesh_to_sdf::Components&>())), std::vector<Measure>>::value,
                "measure per component");
  static_assert(std::is_base_of<m2s_band_measure_record, Measure>::value && sizeof(Measure) == 112 && sizeof(m2s_band_measure_opts) == 8 &&
                    sizeof(m2s_band_measure_info) == 24,
                "the structs' sizes");
  int failures = 0;
  if (argc == 1) {
    m2s_band_measure_record m{};
    uint32_t label = 0;
    if (m2s_band_measure(nullptr, nullptr, nullptr, 0, nullptr, &m, nullptr, nullptr) != M2S_ERR_BAD_ARG) ++failures;
    if (m2s_band_measure(reinterpret_cast<const m2s_band*>(&m), nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) != M2S_ERR_BAD_ARG) ++failures;
    if (m2s_band_measure(reinterpret_cast<const m2s_band*>(&m), nullptr, &label, 0, nullptr, &m, nullptr, nullptr) != M2S_ERR_BAD_ARG) ++failures;
    Measure z{};
    if (!z.closed() || z.euler() != 0) ++failures;
  } else {
    const auto grid = mesh_to_sdf::Grid<V>::new_({0.25f, 0.25f, 0.25f}, {0.5f, 0.5f, 0.5f}, {8, 8, 8});
    std::vector<uint64_t> cells;
    std::vector<float> d;
    for (uint64_t L = 0; L < 512; ++L) {
      const uint64_t i = L / 64, j = (L / 8) % 8, k = L % 8;
      const bool a = i >= 1 && i <= 3 && j >= 1 && j <= 3 && k >= 1 && k <= 3, b = i >= 4 && i <= 6 && j >= 4 && j <= 6 && k >= 4 && k <= 6;
      if (a || b) {
        cells.push_back(L);
        d.push_back((i == 2 && j == 2 && k == 2) || (i == 5 && j == 5 && k == 5) ? -1.0f : 1.0f);
      }
    }
    const Field f(grid, cells, d, 1.0f, 1.0f);
    const uint64_t w = (uint64_t)std::floor((double)std::sqrt(0.01171875f) * 67108864.0);
    const Measure all = f.measure();
    if (all.n_triangles != 16 || all.n_vertices != 12 || all.n_open != 0 || all.n_border != 0 || !all.closed() || all.euler() != 4) ++failures;
    if (all.volume_q != 2 * 1048576 || all.area_q != 16 * w || all.volume != 0.125 / 3) ++failures;
    if (std::fabs(all.centroid[0] - 2.0) > 1e-12 || std::fabs(all.centroid[2] - 2.0) > 1e-12) ++failures;
    const mesh_to_sdf::Components c = f.components(Connectivity::Corners);
    // the two blocks touch at the corner (3, 3, 3) - (4, 4, 4): one component by corners, two by faces
    const mesh_to_sdf::Components faces = f.components(Connectivity::Faces);
    if (c.count() != 1 || faces.count() != 2) ++failures;
    const std::vector<Measure> parts = f.measure(faces);
    if (parts.size() != 2) ++failures;
    for (size_t g = 0; g < parts.size() && parts.size() == 2; ++g) {
      const Measure& p = parts[g];
      const double centre = 0.25 + (g == 0 ? 2.0 : 5.0) * 0.5;
      if (p.n_triangles != 8 || p.n_vertices != 6 || !p.closed() || p.euler() != 2 || p.volume_q != 1048576 || p.area_q != 8 * w) ++failures;
      if (p.volume != 0.125 / 6 || std::fabs(p.centroid[0] - centre) > 1e-12 || std::fabs(p.centroid[1] - centre) > 1e-12 || std::fabs(p.centroid[2] - centre) > 1e-12)
        ++failures;
    }
    if (f.measure(5.0f).n_triangles != 0 || !std::isnan(f.measure(5.0f).centroid[0])) ++failures;
    bool threw = false;
    try { (void)f.measure(std::vector<uint32_t>{0, 1}, 2); } catch (const mesh_to_sdf::Error&) { threw = true; }   // one label per cell
    if (!threw) ++failures;
  }
  std::printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
