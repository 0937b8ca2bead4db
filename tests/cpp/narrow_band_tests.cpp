// narrow_band_sdf of include/mesh_to_sdf.hpp (C++17, -Wall -Werror).  With no arguments it only exercises what is decided before any device
// work (no GPU needed).  With an argument (anything) it takes the band (interior 1, exterior 0.25) of a cube of half side 1 in an 8 x 8 x 8
// grid over [-1.5, 1.5]^3 on the GPU, under both sign methods, and compares cells, distances and bits with the dense generate_grid_sdf.
// Prints "all checks passed".
#include <array>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "mesh_to_sdf.hpp"

int main(int argc, char**) {
  using V = std::array<float, 3>;
  const std::vector<V> vertices = {{-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}, {1, -1, -1}, {1, -1, 1}, {1, 1, -1}, {1, 1, 1}};
  const std::vector<uint32_t> indices = {0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3};
  const auto topo = mesh_to_sdf::Topology<uint32_t>::TriangleList(indices);
  const auto grid = mesh_to_sdf::Grid<V>::from_bounding_box({-1.5f, -1.5f, -1.5f}, {1.5f, 1.5f, 1.5f}, {8, 8, 8});
  int failures = 0;
  if (argc == 1) {
    try {
      (void)mesh_to_sdf::narrow_band_sdf(vertices, topo, grid, -1.0f, 0.25f);
      ++failures;   // a negative width must throw
    } catch (const mesh_to_sdf::Panic&) {
    }
    try {
      (void)mesh_to_sdf::narrow_band_sdf(vertices, topo, grid, 1.0f, std::numeric_limits<float>::quiet_NaN());
      ++failures;   // a NaN width must throw
    } catch (const mesh_to_sdf::Panic&) {
    }
    try {
      (void)mesh_to_sdf::narrow_band_sdf(vertices, topo, mesh_to_sdf::Grid<V>::new_({0, 0, 0}, {0.5f, 0.0f, 0.5f}, {4, 4, 4}), 1.0f, 1.0f);
      ++failures;   // a cell size of 0 must throw
    } catch (const mesh_to_sdf::Panic&) {
    }
  } else {
    const float interior = 1.0f, exterior = 0.25f;
    for (const auto sign : {mesh_to_sdf::SignMethod::Raycast, mesh_to_sdf::SignMethod::Normal}) {
      const std::vector<float> dense = mesh_to_sdf::generate_grid_sdf(vertices, topo, grid, sign);
      const mesh_to_sdf::NarrowBand b = mesh_to_sdf::narrow_band_sdf(vertices, topo, grid, interior, exterior, sign, true);
      if (dense.size() != 512 || b.bits.size() != 64 || b.cells.size() != b.count || b.distances.size() != b.count) ++failures;
      uint64_t seen = 0;
      for (size_t L = 0; L < 512 && !failures; ++L) {
        const bool want = -interior <= dense[L] && dense[L] <= exterior;
        if ((((b.bits[L / 8] >> (L % 8)) & 1u) != 0) != want) ++failures;
        if (!want) continue;
        if (seen >= b.count || b.cells[seen] != L || std::memcmp(&b.distances[seen], &dense[L], 4) != 0) ++failures;
        ++seen;
      }
      if (seen != b.count || seen == 0 || seen == 512) ++failures;
    }
  }
  std::printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
