// BandField::resample of include/mesh_to_sdf.hpp (C++17, -Wall -Werror).  With no arguments it only exercises what is decided without a
// handle (no GPU needed): the types, and the C call's answers to NULL.  With an argument (anything) it resamples on the GPU the field y - 2
// on every point of an 8 x 8 x 8 grid with cells of 0.5, all of it exact in binary32: padded by SNAP onto a grid grown by one cell on every
// side (the centre on the box's `end` face repeats the last cell), moved by two cells along +y, united with the original, and read back by
// TRILINEAR on its own grid, which on a full band of a linear field returns every value.  Prints "all checks passed".
#include <array>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "mesh_to_sdf.hpp"

using V = std::array<float, 3>;
using Field = mesh_to_sdf::BandField<V>;
using mesh_to_sdf::SampleMode;

int main(int argc, char**) {
  static_assert(std::is_same<decltype(std::declval<const Field&>().resample(std::declval<const mesh_to_sdf::Grid<V>&>())), Field>::value, "resample");
  static_assert(std::is_same<decltype(std::declval<const Field&>().resample(std::declval<const mesh_to_sdf::Grid<V>&>(), (const float*)nullptr, 2.0f,
                                                                            SampleMode::Snap, (mesh_to_sdf::ResampleInfo*)nullptr)), Field>::value,
                "resample with a map, a scale, a mode and an info");
  static_assert(sizeof(m2s_band_resample_opts) == 60 && sizeof(m2s_band_resample_info) == 40, "the structs' sizes");
  int failures = 0;
  if (argc == 1) {
    m2s_band* out = reinterpret_cast<m2s_band*>(&failures);
    m2s_grid g{};
    if (m2s_band_resample(nullptr, &g, nullptr, nullptr, nullptr, &out, nullptr) != M2S_ERR_BAD_ARG || out != nullptr) ++failures;
    if (m2s_band_resample(nullptr, &g, nullptr, nullptr, nullptr, nullptr, nullptr) != M2S_ERR_BAD_ARG) ++failures;
  } else {
    const auto grid = mesh_to_sdf::Grid<V>::new_({0.25f, 0.25f, 0.25f}, {0.5f, 0.5f, 0.5f}, {8, 8, 8});
    const auto big = mesh_to_sdf::Grid<V>::new_({-0.25f, -0.25f, -0.25f}, {0.5f, 0.5f, 0.5f}, {10, 10, 10});
    const auto line = [](size_t j) { return 0.25f + 0.5f * (float)j - 2.0f; };
    std::vector<uint64_t> cells;
    std::vector<float> d;
    for (size_t L = 0; L < 512; ++L) { cells.push_back(L); d.push_back(line((L / 8) % 8)); }
    const Field f(grid, cells, d, 0.75f, 0.5f);
    mesh_to_sdf::ResampleInfo info;
    // pad: target index t reads u = t - 1; u in 0 .. 7 is that cell, u == 8 repeats cell 7, u == -1 is off the box
    Field padded = f.resample(big, nullptr, 1.0f, SampleMode::Snap, &info);
    if (info.n_cells != 729 || info.n_partial != 0 || info.n_nonfinite != 0 || padded.count() != 729) ++failures;
    if (padded.background_outside() != 0.75f || padded.background_inside() != 0.5f || padded.device_bytes() != 24ull * 16 + 4ull * 729) ++failures;
    if (padded.grid().get_cell_count()[0] != 10) ++failures;
    {
      const mesh_to_sdf::NarrowBand e = padded.export_band();
      size_t k = 0;
      for (size_t L = 0; L < 1000 && e.count == 729; ++L) {
        const size_t ti = L / 100, tj = (L / 10) % 10, tk = L % 10;
        const bool on = ti >= 1 && tj >= 1 && tk >= 1;
        const float want = line(tj < 1 ? 0 : (tj - 1 > 7 ? 7 : tj - 1));
        if (on && (e.cells[k] != L || e.distances[k] != want)) { ++failures; break; }
        if ((((e.bits[ti * 10 + tj] >> tk) & 1u) != 0) != (on && want < 0.0f)) { ++failures; break; }
        k += on ? 1 : 0;
      }
    }
    bool threw = false;
    try { (void)f.csg(padded, mesh_to_sdf::CsgOp::Union); } catch (const mesh_to_sdf::Error&) { threw = true; }   // the grids differ
    if (!threw) ++failures;
    // crop back: every bit of f
    Field back = padded.resample(grid, nullptr, 1.0f, SampleMode::Snap, &info);
    const mesh_to_sdf::NarrowBand e0 = f.export_band(), e1 = back.export_band();
    if (info.n_cells != 512 || e1.cells != e0.cells || e1.distances != e0.distances) ++failures;
    // move by two cells along +y, twice as large values, then unite with the original
    const float to_source[12] = {1, 0, 0, 0, 0, 1, 0, -1.0f, 0, 0, 1, 0};
    Field moved = f.resample(grid, to_source, 2.0f, SampleMode::Snap, &info);
    if (info.n_cells != 384 || moved.background_outside() != 1.5f || moved.background_inside() != 1.0f) ++failures;
    Field both = f.csg(moved, mesh_to_sdf::CsgOp::Union);
    const mesh_to_sdf::NarrowBand eu = both.export_band();
    for (size_t L = 0; L < 512 && eu.count == 512; ++L) {
      const size_t j = (L / 8) % 8;
      const float a = line(j), b = j >= 2 ? 2.0f * line(j - 2) : 1.5f;
      if (eu.cells[L] != L || eu.distances[L] != (b < a ? b : a)) { ++failures; break; }
    }
    if (eu.count != 512) ++failures;
    // TRILINEAR with the identity on a full band of a linear field: the weights are 0 and 1
    Field same = f.resample(grid, nullptr, 1.0f, SampleMode::Trilinear, &info);
    if (info.n_cells != 512 || info.n_partial != 0 || same.export_band().distances != e0.distances) ++failures;
    threw = false;
    try { (void)f.resample(grid, nullptr, 0.0f); } catch (const mesh_to_sdf::Error&) { threw = true; }
    if (!threw) ++failures;
  }
  std::printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
