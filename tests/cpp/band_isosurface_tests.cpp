// band_isosurface of include/mesh_to_sdf.hpp (C++17, -Wall -Werror).  With no arguments it only exercises what is decided before any device
// work (no GPU needed).  With an argument (anything) it remeshes a cube of half side 1 in a 24 x 24 x 24 grid over [-1.5, 1.5]^3 on the GPU:
// the band of one cell diagonal (x 1.001) around iso from narrow_band_sdf, then band_isosurface, which must equal grid_isosurface of the
// dense generate_grid_sdf bit for bit with n_open == 0; a band of half that width must differ and report n_open > 0.
// Prints "all checks passed".
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mesh_to_sdf.hpp"

int main(int argc, char**) {
  using V = std::array<float, 3>;
  const std::vector<V> vertices = {{-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}, {1, -1, -1}, {1, -1, 1}, {1, 1, -1}, {1, 1, 1}};
  const std::vector<uint32_t> indices = {0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3};
  const auto topo = mesh_to_sdf::Topology<uint32_t>::TriangleList(indices);
  const auto grid = mesh_to_sdf::Grid<V>::from_bounding_box({-1.5f, -1.5f, -1.5f}, {1.5f, 1.5f, 1.5f}, {24, 24, 24});
  int failures = 0;
  if (argc == 1) {
    const auto throws = [&](const std::vector<uint64_t>& cells, const std::vector<float>& d, float iso) {
      try {
        (void)mesh_to_sdf::band_isosurface(grid, cells, d, iso);
      } catch (const mesh_to_sdf::Panic&) {
        return true;
      }
      return false;
    };
    if (!throws({1, 2, 3}, {0.0f, 0.0f}, 0.0f)) ++failures;                    // lengths differ
    if (!throws({3, 2}, {0.0f, 0.0f}, 0.0f)) ++failures;                       // descending
    if (!throws({2, 2}, {0.0f, 0.0f}, 0.0f)) ++failures;                       // a duplicate
    if (!throws({2, 24 * 24 * 24}, {0.0f, 0.0f}, 0.0f)) ++failures;            // at the cell count
    if (!throws({2, 3}, {0.0f, 0.0f}, std::nanf(""))) ++failures;              // a NaN iso
    const auto none = mesh_to_sdf::band_isosurface(grid, {}, {});
    if (!none.vertices.empty() || !none.indices.empty() || none.n_open != 0) ++failures;
  } else {
    // Normal: the sign rule under which this cube's distance field is exact on this grid (the corollary's condition holds)
    const auto sign = mesh_to_sdf::SignMethod::Normal;
    const float h = grid.get_cell_size()[0];
    const float w = 1.001f * std::sqrt(3.0f) * h * 1.0001f;
    const std::vector<float> dense = mesh_to_sdf::generate_grid_sdf(vertices, topo, grid, sign);
    for (const float iso : {0.0f, 0.07f, -0.05f}) {
      const auto want = mesh_to_sdf::grid_isosurface(grid, dense, iso);
      const mesh_to_sdf::NarrowBand b = mesh_to_sdf::narrow_band_sdf(vertices, topo, grid, w - iso, w + iso, sign);
      const auto got = mesh_to_sdf::band_isosurface(grid, b.cells, b.distances, iso);
      if (got.n_open != 0 || got.vertices.size() != want.vertices.size() || got.indices != want.indices || want.indices.empty()) ++failures;
      else if (std::memcmp(got.vertices.data(), want.vertices.data(), sizeof(V) * want.vertices.size()) != 0) ++failures;
    }
    // half that width around iso = 0.07: the band holds one layer of points either side of the level, never a whole cell
    const float iso = 0.07f;
    const mesh_to_sdf::NarrowBand nb = mesh_to_sdf::narrow_band_sdf(vertices, topo, grid, std::max(0.0f, 0.5f * w - iso), 0.5f * w + iso, sign);
    const auto part = mesh_to_sdf::band_isosurface(grid, nb.cells, nb.distances, iso);
    if (part.n_open == 0 || part.indices.size() >= mesh_to_sdf::grid_isosurface(grid, dense, iso).indices.size()) ++failures;
  }
  std::printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
