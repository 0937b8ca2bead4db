// cast_rays / count_intersections / test_occlusions of include/mesh_to_sdf.hpp (C++17, -Wall -Werror).  Prints "all checks passed";
// needs a GPU to run.
#include <array>
#include <cmath>
#include <cstdio>
#include <vector>

#include "mesh_to_sdf.hpp"

int main() {
  using V = std::array<float, 3>;
  const std::vector<V> vertices = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  const std::vector<uint32_t> indices = {0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3};   // outward
  const std::vector<V> origins = {{0.25f, 0.25f, -2.0f}, {0.25f, 0.25f, -2.0f}, {0.1f, 0.1f, 0.1f}};
  const std::vector<V> directions = {{0, 0, 1}, {0, 0, -1}, {-1, 0, 0}};
  const auto topo = mesh_to_sdf::Topology<uint32_t>::TriangleList(indices);
  int failures = 0;
  const mesh_to_sdf::RayHits h = mesh_to_sdf::cast_rays(vertices, topo, origins, directions);
  if (h.t.size() != 3 || h.t[0] != 2.0f || h.triangle[0] != 0 || !std::isinf(h.t[1]) || h.triangle[1] != UINT32_MAX || !std::isnan(h.uv[1][0])) ++failures;
  if (std::fabs(h.t[2] - 0.1f) > 1e-6f || h.triangle[2] != 2) ++failures;   // from inside onto the face x = 0
  const std::vector<uint32_t> n = mesh_to_sdf::count_intersections(vertices, topo, origins, directions);
  if (n.size() != 3 || n[0] != 2 || n[1] != 0 || n[2] != 1) ++failures;
  const std::vector<uint8_t> occ = mesh_to_sdf::test_occlusions(vertices, topo, origins, directions, 0.0f, 1.5f);
  if (occ.size() != 3 || occ[0] != 0 || occ[1] != 0 || occ[2] != 1) ++failures;   // the first ray's hits lie beyond t_max
  try {
    (void)mesh_to_sdf::cast_rays(vertices, topo, origins, directions, 2.0f, 1.0f);
    ++failures;   // t_min > t_max must throw
  } catch (const mesh_to_sdf::Panic&) {
  }
  std::printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
