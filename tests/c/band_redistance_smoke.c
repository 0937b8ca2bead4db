/* m2s_band_redistance from plain C (C99, -Wall -Werror): the declarations compile and link, and every answer that is decided without a
 * handle comes out as include/m2s.h states it.  With an argument (anything) it also redistances a band on the GPU: the slab
 * |x - 2| <= 1 of an 8 x 8 x 8 grid with cells of 0.5, given on the layers i = 1 .. 6, to a width of 1.  The layers next to the two
 * faces are frozen; one sweep reaches the other four, and since 0.25 + 0.5 is exact the result is |x - 2| - 1 on all 512 points.
 * Prints "all checks passed". */
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
  static uint64_t cells[512];
  static float d[512];
  static uint32_t bits[64];
  m2s_band_field_opts fo, got;
  m2s_band_redistance_opts ro;
  m2s_band_redistance_info info;
  m2s_band *a = NULL, *r = (m2s_band*)&g; /* any non-NULL value: a failed call must reset it */
  int x, has = 7;
  (void)argv;
  ro.struct_size = sizeof(ro);
  ro.exterior = 1.0f;
  ro.interior = 1.0f;
  ro.max_sweeps = 0;
  check(sizeof(ro) == 16 && sizeof(info) == 40, "the structs' sizes");
  check(m2s_band_redistance(NULL, &ro, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "NULL handle");
  check(m2s_band_redistance(NULL, &ro, NULL, NULL, NULL, NULL) == M2S_ERR_BAD_ARG, "NULL out");
  check(m2s_version() == 5, "version");
  if (argc > 1) {
    int n = 0;
    uint64_t k = 0, bytes = 0;
    for (x = 0; x < 3; ++x) { g.first_cell[x] = 0.25f; g.cell_size[x] = 0.5f; g.cell_count[x] = 8; }
    for (x = 0; x < 512; ++x) {
      const int i = x / 64;
      if (i >= 1 && i <= 6) { cells[n] = (uint64_t)x; d[n++] = fabsf(0.25f + 0.5f * (float)i - 2.0f) - 1.0f; }
    }
    fo.struct_size = sizeof(fo);
    fo.background_outside = 0.75f;
    fo.background_inside = 0.75f;
    check(m2s_band_create(&g, cells, d, (uint64_t)n, NULL, &fo, NULL, &a) == M2S_OK && a != NULL, "create");
    r = (m2s_band*)&g;
    check(m2s_band_redistance(a, NULL, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "NULL opts");
    ro.struct_size = 12;
    r = (m2s_band*)&g;
    check(m2s_band_redistance(a, &ro, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "struct_size");
    ro.struct_size = sizeof(ro);
    ro.interior = -1.0f;
    r = (m2s_band*)&g;
    check(m2s_band_redistance(a, &ro, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "a negative width");
    ro.interior = 1.0f;
    fo.background_inside = -1.0f;
    r = (m2s_band*)&g;
    check(m2s_band_redistance(a, &ro, &fo, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "a negative background");
    memset(&info, 0, sizeof(info));
    info.struct_size = sizeof(info);
    check(m2s_band_redistance(a, &ro, NULL, NULL, &r, &info) == M2S_OK && r != NULL, "redistance");
    if (r) {
      int bad = 0;
      check(info.sweeps == 1 && info.converged == 1 && info.n_frozen == 256 && info.n_open == 0 && info.n_candidates == 512, "info");
      check(m2s_band_info(r, NULL, &k, &bytes) == M2S_OK && k == 512 && bytes == 24 * 8 + 4 * k, "band_info");
      check(m2s_band_field_info(r, &got, &has) == M2S_OK && has == 1 && got.background_outside == 1.0f && got.background_inside == 1.0f,
            "field_info: the widths");
      check(m2s_band_export(r, cells, d, 512, bits, NULL) == M2S_OK, "export");
      for (x = 0; x < 512; ++x) {
        const float want = fabsf(0.25f + 0.5f * (float)(x / 64) - 2.0f) - 1.0f;
        if (cells[x] != (uint64_t)x || d[x] != want || (int)((bits[x / 8] >> (x % 8)) & 1u) != (want < 0.0f)) ++bad;
      }
      check(bad == 0, "every grid point holds |x - 2| - 1");
      m2s_band_destroy(r);
    }
    m2s_band_destroy(a);
  }
  if (failures == 0) printf("all checks passed\n");
  return failures ? 1 : 0;
}
