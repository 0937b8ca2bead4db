// voxelize of include/mesh_to_sdf.hpp (C++17, -Wall -Werror).  With no arguments it only exercises what is decided before any device work
// (no GPU needed).  With arguments — the expected SURFACE count, the expected SOLID count — it voxelizes a cube of half side 1 into an
// 8 x 8 x 8 grid over [-1.5, 1.5]^3 on the GPU and compares counts, bits and bytes.  Prints "all checks passed".
#include <array>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mesh_to_sdf.hpp"

int main(int argc, char** argv) {
  using V = std::array<float, 3>;
  const std::vector<V> vertices = {{-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}, {1, -1, -1}, {1, -1, 1}, {1, 1, -1}, {1, 1, 1}};
  const std::vector<uint32_t> indices = {0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3};
  const auto topo = mesh_to_sdf::Topology<uint32_t>::TriangleList(indices);
  const auto grid = mesh_to_sdf::Grid<V>::from_bounding_box({-1.5f, -1.5f, -1.5f}, {1.5f, 1.5f, 1.5f}, {8, 8, 8});
  int failures = 0;
  if (argc == 1) {
    try {
      (void)mesh_to_sdf::voxelize(vertices, topo, mesh_to_sdf::Grid<V>::new_({0, 0, 0}, {0.5f, 0.0f, 0.5f}, {4, 4, 4}));
      ++failures;   // a cell size of 0 must throw
    } catch (const mesh_to_sdf::Panic&) {
    }
    try {
      const std::vector<uint32_t> bad = {0, 1, 8};
      (void)mesh_to_sdf::voxelize(vertices, mesh_to_sdf::Topology<uint32_t>::TriangleList(bad), grid);
      ++failures;   // a vertex index out of range must throw
    } catch (const mesh_to_sdf::Panic&) {
    }
  } else {
    if (argc != 3) return 2;
    const uint64_t want_surface = std::strtoull(argv[1], nullptr, 0), want_solid = std::strtoull(argv[2], nullptr, 0);
    const mesh_to_sdf::Voxels s = mesh_to_sdf::voxelize(vertices, topo, grid, false, true);
    const mesh_to_sdf::Voxels f = mesh_to_sdf::voxelize(vertices, topo, grid, true);
    if (s.count != want_surface || f.count != want_solid) ++failures;
    if (s.occupancy.size() != 512 || s.bits.size() != 64 || !f.bits.empty()) ++failures;
    uint64_t ns = 0, nf = 0;
    for (size_t L = 0; L < 512 && !failures; ++L) {
      if (((s.bits[L / 8] >> (L % 8)) & 1u) != s.occupancy[L]) ++failures;
      if (s.occupancy[L] && !f.occupancy[L]) ++failures;   // solid contains the surface
      ns += s.occupancy[L];
      nf += f.occupancy[L];
    }
    if (ns != s.count || nf != f.count) ++failures;
  }
  std::printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
