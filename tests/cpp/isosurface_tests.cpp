// grid_isosurface of include/mesh_to_sdf.hpp (C++17, -Wall -Werror).  Prints "all checks passed"; needs a GPU to run.
#include <array>
#include <cstdio>
#include <vector>

#include "mesh_to_sdf.hpp"

int main() {
  using V = std::array<float, 3>;
  // cells of 0.5 over [0, 4]^3; d = z - 2 (a plane facing +z at z = 2)
  const auto grid = mesh_to_sdf::Grid<V>::from_bounding_box({0, 0, 0}, {4, 4, 4}, {8, 8, 8});
  std::vector<float> d(512);
  for (size_t i = 0; i < d.size(); ++i) d[i] = 0.25f + 0.5f * (float)(i % 8) - 2.0f;
  int failures = 0;
  const auto m = mesh_to_sdf::grid_isosurface(grid, d);
  if (m.vertices.size() != 64 || m.indices.size() != 3 * 98) ++failures;
  for (const V& v : m.vertices)
    if (v[2] != 2.0f) ++failures;
  for (size_t i = 0; i + 2 < m.indices.size(); i += 3) {
    const V &a = m.vertices[m.indices[i]], &b = m.vertices[m.indices[i + 1]], &c = m.vertices[m.indices[i + 2]];
    if ((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]) <= 0.0f) ++failures;   // faces +z
  }
  const auto off = mesh_to_sdf::grid_isosurface(grid, d, 0.5f);   // the plane z = 2.5
  if (off.vertices.empty() || off.vertices[0][2] != 2.5f) ++failures;
  try {
    (void)mesh_to_sdf::grid_isosurface(grid, std::vector<float>(511));
    ++failures;   // distances that do not match the grid must throw
  } catch (const mesh_to_sdf::Panic&) {
  }
  std::printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
