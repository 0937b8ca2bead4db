// BandField::filter of include/mesh_to_sdf.hpp (C++17, -Wall -Werror).  With no arguments it only exercises what is decided without a
// handle (no GPU needed): the types, and the C call's answers to NULL.  With an argument (anything) it filters on the GPU the field y - 2
// on every point of an 8 x 8 x 8 grid with cells of 0.5.  It is linear, so the Laplacian changes only the two layers at the j faces, whose
// reads are clamped (their values are computed here with the header's expressions), and the mean-curvature flow changes nothing.  With the
// field as its own region (its inside, y < 2) only the layer j = 0 changes.  Prints "all checks passed".
#include <array>
#include <cmath>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "mesh_to_sdf.hpp"

using V = std::array<float, 3>;
using Field = mesh_to_sdf::BandField<V>;
using mesh_to_sdf::FilterKind;

int main(int argc, char**) {
  static_assert(std::is_same<decltype(std::declval<const Field&>().filter(FilterKind::Mean)), Field>::value, "filter");
  static_assert(std::is_same<decltype(std::declval<const Field&>().filter(FilterKind::MeanCurvature, 8u, (const Field*)nullptr,
                                                                          (mesh_to_sdf::FilterInfo*)nullptr)), Field>::value,
                "filter with a region and an info");
  static_assert((int)FilterKind::Mean == 0 && (int)FilterKind::Laplacian == 1 && (int)FilterKind::MeanCurvature == 2, "the kinds");
  int failures = 0;
  if (argc == 1) {
    m2s_band* out = reinterpret_cast<m2s_band*>(&failures);
    m2s_band_filter_opts fl{};
    fl.struct_size = sizeof(fl);
    fl.iterations = 1;
    fl.width = 1;
    if (m2s_band_filter(nullptr, nullptr, &fl, nullptr, nullptr, &out, nullptr) != M2S_ERR_BAD_ARG || out != nullptr) ++failures;
    if (m2s_band_filter(nullptr, nullptr, &fl, nullptr, nullptr, nullptr, nullptr) != M2S_ERR_BAD_ARG) ++failures;
  } else {
    const auto grid = mesh_to_sdf::Grid<V>::new_({0.25f, 0.25f, 0.25f}, {0.5f, 0.5f, 0.5f}, {8, 8, 8});
    const auto value = [](size_t L) { return 0.25f + 0.5f * (float)((L / 8) % 8) - 2.0f; };
    std::vector<uint64_t> cells;
    std::vector<float> d;
    for (size_t L = 0; L < 512; ++L) { cells.push_back(L); d.push_back(value(L)); }
    const Field f(grid, cells, d, 0.75f, 0.5f);
    // the host constants and one Laplacian pass at a j face: the clamped read is the cell itself
    const float r = 1.0f / 0.5f, w = r * r, dt = 1.0f / (2.0f * ((w + w) + w));
    const auto face = [&](float c, float other) { const float t = ((other - c) + (c - c)) * w; return c + dt * ((0.0f + t) + 0.0f); };
    const float lo = face(value(0), value(8)), hi = face(value(56), value(48));
    mesh_to_sdf::FilterInfo info;
    Field lap = f.filter(FilterKind::Laplacian, 1, nullptr, &info);
    if (info.passes != 1 || info.n_changed != 128 || info.n_sign_flips != 0 || info.n_nonfinite != 0 || info.max_change != std::fabs(lo - value(0))) ++failures;
    if (lap.count() != 512 || lap.background_outside() != 0.75f || lap.background_inside() != 0.5f || lap.device_bytes() != 24ull * 8 + 4ull * 512) ++failures;
    const mesh_to_sdf::NarrowBand e = lap.export_band();
    for (size_t L = 0; L < 512 && e.count == 512; ++L) {
      const size_t j = (L / 8) % 8;
      const float want = j == 0 ? lo : j == 7 ? hi : value(L);
      if (e.cells[L] != L || e.distances[L] != want || (((e.bits[L / 8] >> (L % 8)) & 1u) != 0) != (want < 0.0f)) { ++failures; break; }
    }
    Field inside = f.filter(FilterKind::Laplacian, 1, &f, &info);
    if (info.n_changed != 64 || inside.count() != 512) ++failures;               // y < 2: the layer j = 0 alone
    Field flow = f.filter(FilterKind::MeanCurvature, 2, nullptr, &info);
    if (info.passes != 2 || info.n_changed != 0 || info.n_nonfinite != 0 || flow.count() != 512) ++failures;   // a plane has no curvature, at a clamped face either
    Field mean = f.filter(FilterKind::Mean, 2, nullptr, &info);
    if (info.passes != 6 || mean.count() != 512) ++failures;
    mean = std::move(lap);
    if (mean.count() != 512) ++failures;
    bool threw = false;
    try { (void)f.filter(FilterKind::Mean, 0); } catch (const mesh_to_sdf::Error&) { threw = true; }
    if (!threw) ++failures;
  }
  std::printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
