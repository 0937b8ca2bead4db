// BandField::redistance of include/mesh_to_sdf.hpp (C++17, -Wall -Werror).  With no arguments it only exercises what is decided without a
// handle (no GPU needed): the types, and the C call's answers to NULL.  With an argument (anything) it redistances on the GPU the slab
// |y - 2| <= 1 of an 8 x 8 x 8 grid with cells of 0.5, given on the layers j = 1 .. 6: to a width of 1 (all 512 points, |y - 2| - 1 on
// each, exactly) and to a width of 0.25 (the four frozen layers alone), and checks the move of a result.  Prints "all checks passed".
#include <array>
#include <cmath>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "mesh_to_sdf.hpp"

using V = std::array<float, 3>;
using Field = mesh_to_sdf::BandField<V>;

int main(int argc, char**) {
  static_assert(std::is_same<decltype(std::declval<const Field&>().redistance(1.0f, 1.0f)), Field>::value, "redistance");
  static_assert(std::is_same<decltype(std::declval<const Field&>().redistance(1.0f, 1.0f, 3u, (mesh_to_sdf::RedistanceInfo*)nullptr)), Field>::value,
                "redistance with a cap and an info");
  int failures = 0;
  if (argc == 1) {
    m2s_band* out = reinterpret_cast<m2s_band*>(&failures);
    m2s_band_redistance_opts ro{};
    ro.struct_size = sizeof(ro);
    if (m2s_band_redistance(nullptr, &ro, nullptr, nullptr, &out, nullptr) != M2S_ERR_BAD_ARG || out != nullptr) ++failures;
    if (m2s_band_redistance(nullptr, &ro, nullptr, nullptr, nullptr, nullptr) != M2S_ERR_BAD_ARG) ++failures;
  } else {
    const auto grid = mesh_to_sdf::Grid<V>::new_({0.25f, 0.25f, 0.25f}, {0.5f, 0.5f, 0.5f}, {8, 8, 8});
    const auto value = [](size_t L) { return std::fabs(0.25f + 0.5f * (float)((L / 8) % 8) - 2.0f) - 1.0f; };
    std::vector<uint64_t> cells;
    std::vector<float> d;
    for (size_t L = 0; L < 512; ++L) {
      const size_t j = (L / 8) % 8;
      if (j >= 1 && j <= 6) { cells.push_back(L); d.push_back(value(L)); }
    }
    const Field f(grid, cells, d, 0.75f, 0.75f);
    mesh_to_sdf::RedistanceInfo info;
    Field r = f.redistance(1.0f, 1.0f, 0, &info);
    if (info.sweeps != 1 || !info.converged || info.n_frozen != 256 || info.n_open != 0 || info.n_candidates != 512) ++failures;
    if (r.count() != 512 || r.background_outside() != 1.0f || r.background_inside() != 1.0f || r.device_bytes() != 24ull * 8 + 4ull * 512) ++failures;
    const mesh_to_sdf::NarrowBand e = r.export_band();
    for (size_t L = 0; L < 512 && e.count == 512; ++L)
      if (e.cells[L] != L || e.distances[L] != value(L) || (((e.bits[L / 8] >> (L % 8)) & 1u) != 0) != (value(L) < 0.0f)) { ++failures; break; }
    Field narrow = f.redistance(0.25f, 0.25f, 0, &info);
    if (narrow.count() != 256 || !info.converged || info.sweeps != 1) ++failures;   // the one sweep's values, 0.75, lie beyond the widths
    narrow = std::move(r);
    if (narrow.count() != 512) ++failures;
    bool threw = false;
    try { (void)f.redistance(-1.0f, 1.0f); } catch (const mesh_to_sdf::Error&) { threw = true; }
    if (!threw) ++failures;
  }
  std::printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
