// closest_points / grid_closest_points of include/mesh_to_sdf.hpp (C++17, -Wall -Werror).  Prints "all checks passed"; needs a GPU to run.
#include <array>
#include <cstdio>
#include <vector>

#include "mesh_to_sdf.hpp"

int main() {
  using V = std::array<float, 3>;
  const std::vector<V> vertices = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  const std::vector<uint32_t> indices = {0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3};
  const std::vector<V> queries = {{0.25f, 0.25f, -2.0f}, {2.0f, 0.0f, 0.0f}};
  const auto topo = mesh_to_sdf::Topology<uint32_t>::TriangleList(indices);
  int failures = 0;
  const mesh_to_sdf::ClosestPoints r = mesh_to_sdf::closest_points(vertices, topo, queries);
  if (r.triangle.size() != 2 || r.triangle[0] != 0 || r.point[0][2] != 0.0f || r.distance[0] != 2.0f) ++failures;
  if (r.point[1][0] != 1.0f || r.distance[1] != 1.0f) ++failures;
  const auto grid = mesh_to_sdf::Grid<V>::from_bounding_box({-1, -1, -1}, {2, 2, 2}, {3, 3, 3});
  const mesh_to_sdf::ClosestPoints g = mesh_to_sdf::grid_closest_points(vertices, topo, grid);
  if (g.triangle.size() != 27 || g.triangle[0] != 0) ++failures;
  try {
    const std::vector<V> none;
    (void)mesh_to_sdf::closest_points(none, mesh_to_sdf::Topology<uint32_t>::TriangleList(), queries);
    ++failures;   // a mesh without triangles must throw
  } catch (const mesh_to_sdf::Panic&) {
  }
  std::printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
