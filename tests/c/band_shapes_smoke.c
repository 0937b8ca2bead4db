/* m2s_band_from_capsules from plain C (C99, -Wall -Werror): the declarations compile and link, and every answer that is decided before any
 * device work comes out as include/m2s.h states it.  With an argument (anything) it also runs on the GPU, on a 16 x 16 x 16 grid of unit
 * cells with centres at the integers: a ball of radius 3 about (8, 8, 8), a bare segment, a shape that is not sound and one off the grid.
 * Every distance of the ball at an integer point is sqrt(integer) - 3, so the counts are known: the points with i^2 + j^2 + k^2 < 9 are
 * inside (93 of them), those with 4 <= i^2 + j^2 + k^2 <= 16 are active for the widths (1, 1).  Prints "all checks passed". */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "m2s.h"

static int failures = 0;
static void check(int ok, const char* what) {
  if (!ok) {
    printf("FAIL %s (%s)\n", what, m2s_last_error());
    ++failures;
  }
}

int main(int argc, char** argv) {
  m2s_grid g;
  m2s_band_shapes_opts so;
  m2s_band_shapes_info info;
  m2s_band_field_opts fo;
  m2s_timings tm;
  m2s_band* h = (m2s_band*)&g;
  static const float a[12] = {8, 8, 8, 1, 1, 1, NAN, 0, 0, 100, 100, 100};
  static const float b[12] = {8, 8, 8, 1, 1, 5, 0, 0, 0, 100, 100, 101};
  static const float r[4] = {3, 0, 1, 1};
  int x;
  (void)argv;
  for (x = 0; x < 3; ++x) { g.first_cell[x] = 0.0f; g.cell_size[x] = 1.0f; g.cell_count[x] = 16; }
  so.struct_size = sizeof(so);
  so.exterior = 1.0f;
  so.interior = 1.0f;
  so.radius = 0.5f;
  check(sizeof(so) == 16 && sizeof(info) == 32, "the structs' sizes");
  check(m2s_band_from_capsules(&g, a, b, r, 4, &so, NULL, NULL, NULL, &info, NULL) == M2S_ERR_BAD_ARG, "NULL out");
  check(m2s_band_from_capsules(NULL, a, b, r, 4, &so, NULL, NULL, &h, &info, NULL) == M2S_ERR_BAD_ARG && h == NULL, "NULL grid");
  check(m2s_band_from_capsules(&g, a, b, r, 4, NULL, NULL, NULL, &h, &info, NULL) == M2S_ERR_BAD_ARG, "NULL options");
  so.struct_size = 12;
  check(m2s_band_from_capsules(&g, a, b, r, 4, &so, NULL, NULL, &h, &info, NULL) == M2S_ERR_BAD_ARG, "the options' struct_size");
  so.struct_size = sizeof(so);
  so.exterior = -1.0f;
  check(m2s_band_from_capsules(&g, a, b, r, 4, &so, NULL, NULL, &h, &info, NULL) == M2S_ERR_BAD_ARG, "a negative width");
  so.exterior = 1.0f;
  so.radius = (float)NAN;
  check(m2s_band_from_capsules(&g, a, b, r, 4, &so, NULL, NULL, &h, &info, NULL) == M2S_ERR_BAD_ARG, "a NaN radius");
  so.radius = 0.5f;
  check(m2s_band_from_capsules(&g, NULL, b, r, 4, &so, NULL, NULL, &h, &info, NULL) == M2S_ERR_BAD_ARG, "NULL a");
  check(m2s_band_from_capsules(&g, a, b, r, (uint64_t)1 << 32, &so, NULL, NULL, &h, &info, NULL) == M2S_ERR_BAD_ARG, "2^32 shapes");
  fo.struct_size = 4;
  fo.background_outside = fo.background_inside = 1.0f;
  check(m2s_band_from_capsules(&g, a, b, r, 4, &so, &fo, NULL, &h, &info, NULL) == M2S_ERR_BAD_ARG, "the backgrounds' struct_size");
  g.cell_count[0] = (uint64_t)1 << 36;
  g.cell_count[1] = g.cell_count[2] = 1;
  check(m2s_band_from_capsules(&g, a, b, r, 4, &so, NULL, NULL, &h, &info, NULL) == M2S_ERR_BAD_ARG, "a grid of 2^36 points");
  g.cell_count[0] = g.cell_count[1] = g.cell_count[2] = 16;
  if (argc > 1) {
    uint64_t n_cells = 0, bytes = 0, want_active = 0, want_inside = 0;
    int i, j, k, has_inside = 0;
    for (i = -8; i < 8; ++i)
      for (j = -8; j < 8; ++j)
        for (k = -8; k < 8; ++k) {
          const int q = i * i + j * j + k * k;
          want_inside += q < 9;
          want_active += q >= 4 && q <= 16;
        }
    /* the ball alone, spheres by b == NULL and one radius for all */
    so.radius = 3.0f;
    memset(&info, 0xee, sizeof(info));
    memset(&tm, 0xee, sizeof(tm));
    h = NULL;
    check(m2s_band_from_capsules(&g, a, NULL, NULL, 1, &so, NULL, NULL, &h, &info, &tm) == M2S_OK && h != NULL, "one ball");
    check(info.n_cells == want_active && info.n_inside == want_inside && info.n_inside == 93 && info.n_skipped == 0 && info.n_off_grid == 0, "the ball's counts");
    check(m2s_band_info(h, NULL, &n_cells, &bytes) == M2S_OK && n_cells == want_active && bytes == 64 * 24 + 4 * want_active, "the handle's info");
    check(m2s_band_field_info(h, &fo, &has_inside) == M2S_OK && fo.struct_size == sizeof(fo) && fo.background_outside == 1.0f && fo.background_inside == 1.0f &&
              has_inside == 1, "the backgrounds are the widths");
    check(tm.total_ms > 0.0f && tm.n_units == want_active && tm.n_triangles == 1, "the timings");
    {
      static uint64_t cells[4096];
      static float d[4096];
      static uint32_t bits[256];
      uint64_t c, bad = 0, set = 0;
      check(m2s_band_export(h, cells, d, 4096, bits, NULL) == M2S_OK, "export");
      for (c = 0; c < n_cells && c < 4096; ++c) {
        const int ci = (int)(cells[c] / 256) - 8, cj = (int)(cells[c] / 16 % 16) - 8, ck = (int)(cells[c] % 16) - 8;
        const float want = sqrtf((float)(ci * ci + cj * cj + ck * ck)) - 3.0f;
        bad += d[c] != want;
      }
      for (c = 0; c < 256; ++c)
        for (x = 0; x < 32; ++x) set += (bits[c] >> x) & 1u;
      check(bad == 0, "every value is sqrt(i^2 + j^2 + k^2) - 3");
      check(set == 93, "the sign mask's bits");
    }
    m2s_band_destroy(h);
    /* all four shapes: the segment adds its cells, the others are counted */
    so.exterior = 0.5f;
    so.interior = 0.0f;
    h = NULL;
    check(m2s_band_from_capsules(&g, a, b, r, 4, &so, NULL, NULL, &h, &info, NULL) == M2S_OK && h != NULL, "four shapes");
    check(info.n_skipped == 1 && info.n_off_grid == 1 && info.n_inside == 93, "one shape skipped, one off the grid");
    /* the ball: 9 <= q <= 12 (sqrt(12) - 3 = 0.46); the segment: its five points */
    want_active = 5;
    for (i = -8; i < 8; ++i)
      for (j = -8; j < 8; ++j)
        for (k = -8; k < 8; ++k) want_active += (i * i + j * j + k * k >= 9 && i * i + j * j + k * k <= 12);
    check(info.n_cells == want_active, "the cells of the ball's shell and of the segment");
    m2s_band_destroy(h);
    /* no shape at all: an empty field */
    h = NULL;
    check(m2s_band_from_capsules(&g, NULL, NULL, NULL, 0, &so, NULL, NULL, &h, &info, NULL) == M2S_OK && h != NULL && info.n_cells == 0 && info.n_inside == 0,
          "no shapes: an empty field");
    m2s_band_destroy(h);
  }
  if (failures == 0) printf("all checks passed\n");
  return failures ? 1 : 0;
}
