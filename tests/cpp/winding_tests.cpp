// winding_numbers / grid_winding_numbers / generate_grid_sdf_winding of include/mesh_to_sdf.hpp (C++17, -Wall -Werror).  Prints
// "all checks passed"; needs a GPU to run.
#include <array>
#include <cmath>
#include <cstdio>
#include <vector>

#include "mesh_to_sdf.hpp"

int main() {
  using V = std::array<float, 3>;
  const std::vector<V> vertices = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  const std::vector<uint32_t> indices = {0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3};   // outward
  const std::vector<V> queries = {{0.25f, 0.25f, -2.0f}, {0.1f, 0.1f, 0.1f}};
  const auto topo = mesh_to_sdf::Topology<uint32_t>::TriangleList(indices);
  int failures = 0;
  const std::vector<float> w = mesh_to_sdf::winding_numbers(vertices, topo, queries);
  if (w.size() != 2 || std::fabs(w[0]) > 1e-5f || std::fabs(w[1] - 1.0f) > 1e-5f) ++failures;
  const auto grid = mesh_to_sdf::Grid<V>::from_bounding_box({-1, -1, -1}, {2, 2, 2}, {3, 3, 3});
  const std::vector<float> gw = mesh_to_sdf::grid_winding_numbers(vertices, topo, grid, 2.0f);
  if (gw.size() != 27 || std::fabs(gw[0]) > 1e-2f) ++failures;
  const std::vector<float> sdf = mesh_to_sdf::generate_grid_sdf_winding(vertices, topo, grid);
  if (sdf.size() != 27 || !(sdf[0] > 0.0f)) ++failures;
  try {
    (void)mesh_to_sdf::winding_numbers(vertices, topo, queries, 0.5f);
    ++failures;   // beta < 1 must throw
  } catch (const mesh_to_sdf::Panic&) {
  }
  std::printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
