// BandField::components / select / keep_largest of include/mesh_to_sdf.hpp (C++17, -Wall -Werror).  With no arguments it only exercises what
// is decided without a handle (no GPU needed): the types, and the C calls' answers to NULL.  With an argument (anything) it labels and selects
// on the GPU, on an 8 x 8 x 8 grid: two cubes of 2 x 2 x 2 cells that touch at one corner, (0..1)^3 and (2..3)^3, and a lone cell at (7, 7, 0).
// Three components by faces and by edges, two by corners.  Prints "all checks passed".
#include <array>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "mesh_to_sdf.hpp"

using V = std::array<float, 3>;
using Field = mesh_to_sdf::BandField<V>;
using mesh_to_sdf::Connectivity;

int main(int argc, char**) {
  static_assert(std::is_same<decltype(std::declval<const Field&>().components()), mesh_to_sdf::Components>::value, "components");
  static_assert(std::is_same<decltype(std::declval<const Field&>().select(std::declval<const std::vector<uint32_t>&>(),
                                                                          std::declval<const std::vector<uint8_t>&>(), (mesh_to_sdf::SelectInfo*)nullptr)),
                             Field>::value, "select");
  static_assert(std::is_same<decltype(std::declval<const Field&>().keep_largest(2, Connectivity::Corners)), Field>::value, "keep_largest");
  static_assert(sizeof(m2s_band_component) == 48 && sizeof(m2s_band_components_opts) == 8 && sizeof(m2s_band_select_info) == 32, "the structs' sizes");
  static_assert((int)Connectivity::Faces == 6 && (int)Connectivity::Edges == 18 && (int)Connectivity::Corners == 26, "the connectivities");
  int failures = 0;
  if (argc == 1) {
    m2s_band* out = reinterpret_cast<m2s_band*>(&failures);
    uint64_t n = 0;
    uint32_t label = 0;
    if (m2s_band_components(nullptr, nullptr, nullptr, nullptr, nullptr, 0, &n) != M2S_ERR_BAD_ARG) ++failures;
    if (m2s_band_select(nullptr, &label, nullptr, 0, nullptr, nullptr, &out, nullptr) != M2S_ERR_BAD_ARG || out != nullptr) ++failures;
    if (m2s_band_select(nullptr, &label, nullptr, 0, nullptr, nullptr, nullptr, nullptr) != M2S_ERR_BAD_ARG) ++failures;
  } else {
    const auto grid = mesh_to_sdf::Grid<V>::new_({0.25f, 0.25f, 0.25f}, {0.5f, 0.5f, 0.5f}, {8, 8, 8});
    std::vector<uint64_t> cells;
    std::vector<float> d;
    for (uint64_t L = 0; L < 512; ++L) {
      const uint64_t i = L / 64, j = (L / 8) % 8, k = L % 8;
      const bool a = i < 2 && j < 2 && k < 2, b = i >= 2 && i < 4 && j >= 2 && j < 4 && k >= 2 && k < 4, c = i == 7 && j == 7 && k == 0;
      if (a || b || c) {
        cells.push_back(L);
        d.push_back(a ? -0.25f : 0.25f);
      }
    }
    const Field f(grid, cells, d, 0.75f, 0.5f);
    const mesh_to_sdf::Components faces = f.components(), edges = f.components(Connectivity::Edges), corners = f.components(Connectivity::Corners);
    if (faces.count() != 3 || edges.count() != 3 || corners.count() != 2 || faces.labels.size() != 17) ++failures;
    if (faces.count() == 3) {
      const m2s_band_component& a = faces.components[0];
      const m2s_band_component& b = faces.components[1];
      const m2s_band_component& c = faces.components[2];
      if (a.first_cell != 0 || a.n_cells != 8 || a.n_negative != 8 || a.hi[0] != 1 || a.hi[1] != 1 || a.hi[2] != 1) ++failures;
      if (b.first_cell != 2 * 64 + 2 * 8 + 2 || b.n_cells != 8 || b.n_negative != 0 || b.lo[0] != 2 || b.hi[2] != 3) ++failures;
      if (c.first_cell != 7 * 64 + 7 * 8 || c.n_cells != 1 || c.lo[1] != 7 || c.hi[2] != 0) ++failures;
      for (size_t r = 0; r < 17; ++r)
        if (faces.labels[r] != (r < 8 ? 0u : (r < 16 ? 1u : 2u))) { ++failures; break; }
      if (faces.largest(2) != std::vector<uint32_t>{0, 1}) ++failures;   // a tie goes to the lower number
    }
    if (corners.count() == 2 && (corners.components[0].n_cells != 16 || corners.components[1].n_cells != 1 || corners.largest(1) != std::vector<uint32_t>{0}))
      ++failures;
    mesh_to_sdf::SelectInfo info;
    Field two = f.keep_largest(2, Connectivity::Faces, &info);
    if (info.n_cells != 16 || info.n_dropped != 1 || info.n_sign_cleared != 0 || two.count() != 16) ++failures;
    if (two.background_outside() != 0.75f || two.background_inside() != 0.5f || two.device_bytes() != 24ull * 8 + 4ull * 16) ++failures;
    const mesh_to_sdf::NarrowBand e = two.export_band();
    for (size_t r = 0; r < 16 && e.count == 16; ++r)
      if (e.cells[r] != cells[r] || e.distances[r] != d[r]) { ++failures; break; }
    if (e.count == 16 && (e.bits[0] != 3u || e.bits[1] != 3u || e.bits[8] != 3u || e.bits[9] != 3u || e.bits[63] != 0u)) ++failures;
    Field one = f.select(faces.labels, {0, 1});                          // keep shorter than the count: the lone cell goes too
    if (one.count() != 8 || one.export_band().cells.front() != 2 * 64 + 2 * 8 + 2) ++failures;
    Field none = f.select(std::vector<uint32_t>(17, M2S_LABEL_NONE), {1, 1, 1}, &info);
    if (none.count() != 0 || info.n_dropped != 17) ++failures;
    bool threw = false;
    try { (void)f.select({0, 1}, {1}); } catch (const mesh_to_sdf::Error&) { threw = true; }   // one label per cell
    if (!threw) ++failures;
  }
  std::printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
