// sample_surface / surface_area of include/mesh_to_sdf.hpp (C++17, -Wall -Werror).  With no arguments it only exercises what is decided
// before any device work (no GPU needed).  With arguments — seed, n, area as a hex double, then per sample "triangle u v x y z" with the
// floats as hex bit patterns — it samples a unit cube on the GPU and compares every bit.  Prints "all checks passed".
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mesh_to_sdf.hpp"

static uint32_t bits(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}

int main(int argc, char** argv) {
  using V = std::array<float, 3>;
  const std::vector<V> vertices = {{-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}, {1, -1, -1}, {1, -1, 1}, {1, 1, -1}, {1, 1, 1}};
  const std::vector<uint32_t> indices = {0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3};
  const auto topo = mesh_to_sdf::Topology<uint32_t>::TriangleList(indices);
  int failures = 0;
  if (argc == 1) {
    const std::vector<V> nothing;
    if (mesh_to_sdf::surface_area(nothing, mesh_to_sdf::Topology<uint32_t>::TriangleList()) != 0.0) ++failures;
    try {
      (void)mesh_to_sdf::sample_surface(nothing, mesh_to_sdf::Topology<uint32_t>::TriangleList(), 3);
      ++failures;   // nothing to sample must throw
    } catch (const mesh_to_sdf::Panic&) {
    }
    try {
      (void)mesh_to_sdf::sample_surface(vertices, topo, 3, 0, UINT64_MAX - 1);
      ++failures;   // first_sample + n overflows
    } catch (const mesh_to_sdf::Panic&) {
    }
  } else {
    const uint64_t seed = std::strtoull(argv[1], nullptr, 0);
    const size_t n = (size_t)std::strtoull(argv[2], nullptr, 0);
    const double area = std::strtod(argv[3], nullptr);
    if (argc != 4 + 6 * (int)n) return 2;
    const mesh_to_sdf::SurfaceSamples s = mesh_to_sdf::sample_surface(vertices, topo, n, seed, 0, true);
    if (s.area != area || mesh_to_sdf::surface_area(vertices, topo) != area || s.area != 24.0) ++failures;
    if (s.points.size() != n || s.triangle.size() != n || s.uv.size() != n || s.normal.size() != n) ++failures;
    for (size_t i = 0; i < n && !failures; ++i) {
      char** a = argv + 4 + 6 * i;
      if (s.triangle[i] != (uint32_t)std::strtoul(a[0], nullptr, 0)) ++failures;
      if (bits(s.uv[i][0]) != (uint32_t)std::strtoul(a[1], nullptr, 16) || bits(s.uv[i][1]) != (uint32_t)std::strtoul(a[2], nullptr, 16)) ++failures;
      for (int k = 0; k < 3; ++k)
        if (bits(s.points[i][k]) != (uint32_t)std::strtoul(a[3 + k], nullptr, 16)) ++failures;
      // a cube's normals are axis vectors
      const float len = s.normal[i][0] * s.normal[i][0] + s.normal[i][1] * s.normal[i][1] + s.normal[i][2] * s.normal[i][2];
      if (len != 1.0f) ++failures;
    }
    const mesh_to_sdf::SurfaceSamples tail = mesh_to_sdf::sample_surface(vertices, topo, n - n / 2, seed, n / 2);
    for (size_t i = n / 2; i < n; ++i)
      if (std::memcmp(&tail.points[i - n / 2], &s.points[i], 12) != 0) ++failures;
  }
  std::printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
