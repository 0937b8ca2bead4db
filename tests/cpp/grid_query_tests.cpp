// sample_grid / raymarch_grid of include/mesh_to_sdf.hpp (C++17, -Wall -Werror).  Prints "all checks passed"; needs a GPU to run.
#include <array>
#include <cmath>
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
  const std::vector<V> pts = {{1, 1, 1}, {1, 1, 3}, {1, 1, 9}};
  const auto s = mesh_to_sdf::sample_grid(grid, d, pts, {}, true);
  if (s.value.size() != 3 || s.value[0] != -1.0f || s.value[1] != 1.0f || s.value[2] != 100.0f) ++failures;
  if (s.normal.size() != 3 || s.normal[0][2] != 1.0f || s.normal[0][0] != 0.0f) ++failures;
  mesh_to_sdf::SampleOptions snap;
  snap.mode = mesh_to_sdf::SampleMode::Snap;
  snap.outside = -5.0f;
  const auto sn = mesh_to_sdf::sample_grid(grid, d, pts, snap);
  if (sn.value[0] != -0.75f || sn.value[2] != -5.0f || !sn.normal.empty()) ++failures;   // snap: the centre at z = 1.25
  const std::vector<V> org = {{1, 1, 5}}, dir = {{0, 0, -1}};   // from the +z side, where d > 0, towards the plane
  const auto r = mesh_to_sdf::raymarch_grid(grid, d, org, dir, {}, true);
  if (r.hit.size() != 1 || std::fabs(r.hit[0][2] - 2.0f) > 0.01f || r.steps[0] == 0 || r.normal[0][2] != 1.0f) ++failures;
  try {
    (void)mesh_to_sdf::sample_grid(grid, std::vector<float>(511), pts);
    ++failures;   // distances that do not match the grid must throw
  } catch (const mesh_to_sdf::Panic&) {
  }
  std::printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
