// BandField::advect of include/mesh_to_sdf.hpp (C++17, -Wall -Werror).  With no arguments it only exercises what is decided without a
// handle (no GPU needed): the types, and the C call's answers to NULL.  With an argument (anything) it moves on the GPU the field y - 2
// on every point of an 8 x 8 x 8 grid with cells of 0.5 along its normal.  Its gradient is 1 along j, so a speed of 1 lowers every layer
// by dt but j = 0, whose backward read is clamped, and a speed of -1 raises every layer by dt but j = 7 (the values are computed here
// with the header's expressions).  A velocity of zero keeps every bit.  Prints "all checks passed".
#include <array>
#include <cmath>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "mesh_to_sdf.hpp"

using V = std::array<float, 3>;
using Field = mesh_to_sdf::BandField<V>;
using mesh_to_sdf::AdvectKind;

int main(int argc, char**) {
  static_assert(std::is_same<decltype(std::declval<const Field&>().advect(AdvectKind::Normal, std::vector<float>(), 0.5f)), Field>::value, "advect");
  static_assert(std::is_same<decltype(std::declval<const Field&>().advect(AdvectKind::Velocity, std::vector<float>(), 0.5f, 8u,
                                                                          (mesh_to_sdf::AdvectInfo*)nullptr)), Field>::value,
                "advect with steps and an info");
  static_assert((int)AdvectKind::Velocity == 0 && (int)AdvectKind::Normal == 1, "the kinds");
  int failures = 0;
  if (argc == 1) {
    m2s_band* out = reinterpret_cast<m2s_band*>(&failures);
    m2s_band_advect_opts ao{};
    ao.struct_size = sizeof(ao);
    ao.steps = 1;
    ao.dt = 0.5f;
    if (m2s_band_advect(nullptr, nullptr, &ao, nullptr, nullptr, &out, nullptr) != M2S_ERR_BAD_ARG || out != nullptr) ++failures;
    if (m2s_band_advect(nullptr, nullptr, &ao, nullptr, nullptr, nullptr, nullptr) != M2S_ERR_BAD_ARG) ++failures;
  } else {
    const auto grid = mesh_to_sdf::Grid<V>::new_({0.25f, 0.25f, 0.25f}, {0.5f, 0.5f, 0.5f}, {8, 8, 8});
    const auto value = [](size_t L) { return 0.25f + 0.5f * (float)((L / 8) % 8) - 2.0f; };
    std::vector<uint64_t> cells;
    std::vector<float> d;
    for (size_t L = 0; L < 512; ++L) { cells.push_back(L); d.push_back(value(L)); }
    const Field f(grid, cells, d, 0.75f, 0.5f);
    // the host constant and one Godunov step where the one-sided difference the speed's sign picks is 1 along j and 0 along i and k
    const float r = 1.0f / 0.5f, dt = 0.125f;
    const auto step = [&](float c, float lower, float speed) {
      const float D = (c - lower) * r, q = D * D;
      return c - dt * (speed * std::sqrt((0.0f + q) + 0.0f));
    };
    mesh_to_sdf::AdvectInfo info;
    for (const float speed : {1.0f, -1.0f}) {
      Field moved = f.advect(AdvectKind::Normal, std::vector<float>(512, speed), dt, 1, &info);
      if (info.steps != 1 || info.n_moving != 512 || info.n_changed != 448 || info.n_sign_flips != 0 || info.n_nonfinite != 0 ||
          info.max_change != dt || info.max_cfl != dt * (1.0f * ((r + r) + r)))
        ++failures;
      if (moved.count() != 512 || moved.background_outside() != 0.75f || moved.background_inside() != 0.5f || moved.device_bytes() != 24ull * 8 + 4ull * 512)
        ++failures;
      const mesh_to_sdf::NarrowBand e = moved.export_band();
      for (size_t L = 0; L < 512 && e.count == 512; ++L) {
        const size_t j = (L / 8) % 8;
        const float want = j == (speed > 0.0f ? 0u : 7u) ? value(L) : step(value(L), value(L) - 0.5f, speed);
        if (e.cells[L] != L || e.distances[L] != want || (((e.bits[L / 8] >> (L % 8)) & 1u) != 0) != (want < 0.0f)) { ++failures; break; }
      }
    }
    Field still = f.advect(AdvectKind::Velocity, std::vector<float>(3 * 512, 0.0f), dt, 3, &info);
    if (info.steps != 3 || info.n_moving != 0 || info.n_changed != 0 || info.max_cfl != 0.0f || still.count() != 512) ++failures;
    Field carried = f.advect(AdvectKind::Velocity, std::vector<float>(3 * 512, 0.5f), dt, 2, &info);
    if (info.steps != 2 || info.n_moving != 512 || info.n_changed == 0 || carried.count() != 512) ++failures;
    carried = std::move(still);
    if (carried.count() != 512) ++failures;
    bool threw = false;
    try { (void)f.advect(AdvectKind::Normal, std::vector<float>(512, 1.0f), dt, 0); } catch (const mesh_to_sdf::Error&) { threw = true; }
    if (!threw) ++failures;
    threw = false;
    try { (void)f.advect(AdvectKind::Normal, std::vector<float>(511, 1.0f), dt); } catch (const mesh_to_sdf::Error&) { threw = true; }
    if (!threw) ++failures;
  }
  std::printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
