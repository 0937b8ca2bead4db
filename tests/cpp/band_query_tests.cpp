// BandField of include/mesh_to_sdf.hpp (C++17, -Wall -Werror).  With no arguments it only exercises what is decided before any device work
// (no GPU needed).  With an argument (anything) it makes the band field of a cube of half side 1 in a 24 x 24 x 24 grid over [-1.5, 1.5]^3
// on the GPU — narrow_band_sdf three cells wide, voxelize(solid) for the sign — and checks sample and raymarch against sample_grid and
// raymarch_grid on the dense grid the band stands for, bit for bit.
// Prints "all checks passed".
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "mesh_to_sdf.hpp"

int main(int argc, char**) {
  using V = std::array<float, 3>;
  using Field = mesh_to_sdf::BandField<V>;
  static_assert(!std::is_copy_constructible<Field>::value && std::is_move_constructible<Field>::value, "BandField is move-only");
  const std::vector<V> vertices = {{-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}, {1, -1, -1}, {1, -1, 1}, {1, 1, -1}, {1, 1, 1}};
  const std::vector<uint32_t> indices = {0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3};
  const auto topo = mesh_to_sdf::Topology<uint32_t>::TriangleList(indices);
  const auto grid = mesh_to_sdf::Grid<V>::from_bounding_box({-1.5f, -1.5f, -1.5f}, {1.5f, 1.5f, 1.5f}, {24, 24, 24});
  int failures = 0;
  if (argc == 1) {
    const auto throws = [&](const std::vector<uint64_t>& cells, const std::vector<float>& d, float bo, float bi, const std::vector<uint32_t>& bits) {
      try {
        Field f(grid, cells, d, bo, bi, bits);
      } catch (const mesh_to_sdf::Panic&) {
        return true;
      }
      return false;
    };
    if (!throws({1, 2, 3}, {0.0f, 0.0f}, 0.1f, 0.1f, {})) ++failures;                        // lengths differ
    if (!throws({3, 2}, {0.0f, 0.0f}, 0.1f, 0.1f, {})) ++failures;                           // descending
    if (!throws({2, 2}, {0.0f, 0.0f}, 0.1f, 0.1f, {})) ++failures;                           // a duplicate
    if (!throws({2, 24 * 24 * 24}, {0.0f, 0.0f}, 0.1f, 0.1f, {})) ++failures;                // at the cell count
    if (!throws({2, 3}, {0.0f, std::nanf("")}, 0.1f, 0.1f, {})) ++failures;                  // a NaN distance
    if (!throws({2, 3}, {0.0f, 0.0f}, -0.1f, 0.1f, {})) ++failures;                          // a negative background
    if (!throws({2, 3}, {0.0f, 0.0f}, 0.1f, std::nanf(""), {})) ++failures;                  // a NaN background
    if (!throws({2, 3}, {0.0f, 0.0f}, 0.1f, 0.1f, std::vector<uint32_t>(5))) ++failures;     // a sign mask of the wrong size
  } else {
    const float h = grid.get_cell_size()[0], w = 3.0f * h;
    const mesh_to_sdf::NarrowBand b = mesh_to_sdf::narrow_band_sdf(vertices, topo, grid, w, w);
    const auto vox = mesh_to_sdf::voxelize(vertices, topo, grid, true, true);
    Field made(grid, b.cells, b.distances, w, w, vox.bits);
    Field field(std::move(made));
    if (field.count() != b.cells.size() || field.device_bytes() != 24ull * (24 * 24 * 24 / 64) + 4ull * b.cells.size()) ++failures;
    // the dense grid the band stands for
    std::vector<float> dense(24 * 24 * 24);
    for (size_t L = 0; L < dense.size(); ++L) {
      const size_t row = L / 24, k = L % 24;
      dense[L] = ((vox.bits[row] >> k) & 1u) ? -w : w;
    }
    for (size_t a = 0; a < b.cells.size(); ++a) dense[b.cells[a]] = b.distances[a];
    std::vector<V> pts, org, dir;
    for (int i = 0; i < 500; ++i) pts.push_back({-1.6f + 0.0064f * (float)i, -1.2f + 0.0047f * (float)i, 1.3f - 0.0052f * (float)i});
    for (int i = 0; i < 64; ++i) {
      org.push_back({-3.0f, -1.4f + 0.35f * (float)(i / 8), -1.4f + 0.35f * (float)(i % 8)});
      dir.push_back({1.0f, 0.0f, 0.0f});
    }
    for (const auto mode : {mesh_to_sdf::SampleMode::Snap, mesh_to_sdf::SampleMode::Trilinear, mesh_to_sdf::SampleMode::Tetrahedral}) {
      mesh_to_sdf::SampleOptions so;
      so.mode = mode;
      const auto want = mesh_to_sdf::sample_grid(grid, dense, pts, so, true);
      const auto got = field.sample(pts, so, true);
      if (std::memcmp(got.value.data(), want.value.data(), 4 * pts.size()) != 0) ++failures;
      if (std::memcmp(got.normal.data(), want.normal.data(), 12 * pts.size()) != 0) ++failures;
      size_t full = 0;
      const uint8_t k = mode == mesh_to_sdf::SampleMode::Snap ? 1 : (mode == mesh_to_sdf::SampleMode::Trilinear ? 8 : 4);
      for (const uint8_t s : got.support) full += s == k;
      if (full == 0 || full == pts.size()) ++failures;
      const auto wr = mesh_to_sdf::raymarch_grid(grid, dense, org, dir, so, true);
      const auto gr = field.raymarch(org, dir, so, true);
      if (std::memcmp(gr.hit.data(), wr.hit.data(), 16 * org.size()) != 0 || gr.steps != wr.steps) ++failures;
      if (std::memcmp(gr.normal.data(), wr.normal.data(), 12 * org.size()) != 0) ++failures;
    }
  }
  std::printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
