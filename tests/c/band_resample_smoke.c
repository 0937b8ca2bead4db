/* m2s_band_resample from plain C (C99, -Wall -Werror): the declarations compile and link, and every answer that is decided without a
 * handle comes out as include/m2s.h states it.  With an argument (anything) it also resamples a band on the GPU: the field x - 2 on every
 * point of an 8 x 8 x 8 grid with cells of 0.5, all of it exact in binary32.
 *   pad    SNAP onto the grid grown by 2 cells on every side: target index t reads source index u = t - 2; u in 0 .. 7 is that cell, u == 8
 *          is the centre on the box's `end` face, which repeats cell 7 (the clamped reads), the rest is off the box.
 *   move   SNAP onto the same grid with to_source = x - 1: the solid moves by two cells along +x.
 *   union  m2s_band_csg refuses the padded band (another grid) and takes the moved one.
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
  m2s_grid g, big;
  static uint64_t cells[1728];
  static float d[1728];
  static uint32_t bits[144];
  float line[8];
  m2s_band_field_opts fo, got;
  m2s_band_resample_opts ro;
  m2s_band_resample_info info;
  m2s_band *a = NULL, *r = (m2s_band*)&g; /* any non-NULL value: a failed call must reset it */
  int x, has = 7;
  (void)argv;
  memset(&ro, 0, sizeof(ro));
  ro.struct_size = sizeof(ro);
  ro.mode = M2S_SAMPLE_SNAP;
  ro.to_source[0] = ro.to_source[5] = ro.to_source[10] = 1.0f;
  ro.value_scale = 1.0f;
  for (x = 0; x < 3; ++x) { g.first_cell[x] = 0.25f; g.cell_size[x] = 0.5f; g.cell_count[x] = 8; }
  big = g;
  for (x = 0; x < 3; ++x) { big.first_cell[x] = -0.75f; big.cell_count[x] = 12; }
  check(sizeof(ro) == 60 && sizeof(info) == 40, "the structs' sizes");
  check(m2s_band_resample(NULL, &g, &ro, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "NULL handle");
  check(m2s_band_resample(NULL, &g, &ro, NULL, NULL, NULL, NULL) == M2S_ERR_BAD_ARG, "NULL out");
  check(m2s_version() == 5, "version");
  if (argc > 1) {
    uint64_t k = 0, bytes = 0;
    int bad, L;
    for (x = 0; x < 8; ++x) line[x] = 0.25f + 0.5f * (float)x - 2.0f;
    for (x = 0; x < 512; ++x) { cells[x] = (uint64_t)x; d[x] = line[x / 64]; }
    fo.struct_size = sizeof(fo);
    fo.background_outside = 0.75f;
    fo.background_inside = 0.5f;
    check(m2s_band_create(&g, cells, d, 512, NULL, &fo, NULL, &a) == M2S_OK && a != NULL, "create");
    r = (m2s_band*)&g;
    check(m2s_band_resample(a, NULL, &ro, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "NULL target");
    ro.struct_size = 56;
    r = (m2s_band*)&g;
    check(m2s_band_resample(a, &g, &ro, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "struct_size");
    ro.struct_size = sizeof(ro);
    ro.mode = 3;
    r = (m2s_band*)&g;
    check(m2s_band_resample(a, &g, &ro, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "a bad mode");
    ro.mode = M2S_SAMPLE_SNAP;
    ro.value_scale = 0.0f;
    r = (m2s_band*)&g;
    check(m2s_band_resample(a, &g, &ro, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "a scale of 0");
    ro.value_scale = 1.0f;
    ro.to_source[7] = INFINITY;
    r = (m2s_band*)&g;
    check(m2s_band_resample(a, &g, &ro, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "an infinite entry");
    ro.to_source[7] = 0.0f;
    /* pad */
    memset(&info, 0, sizeof(info));
    info.struct_size = sizeof(info);
    check(m2s_band_resample(a, &big, &ro, NULL, NULL, &r, &info) == M2S_OK && r != NULL, "pad");
    if (r) {
      m2s_band* u = (m2s_band*)&g;
      check(info.n_cells == 729 && info.n_partial == 0 && info.n_nonfinite == 0, "pad: info");
      check(m2s_band_info(r, NULL, &k, &bytes) == M2S_OK && k == 729 && bytes == 24 * 27 + 4 * k, "pad: band_info");
      check(m2s_band_field_info(r, &got, &has) == M2S_OK && has == 1 && got.background_outside == 0.75f && got.background_inside == 0.5f,
            "pad: the input's backgrounds");
      check(m2s_band_export(r, cells, d, 1728, bits, NULL) == M2S_OK, "pad: export");
      bad = 0;
      k = 0;
      for (L = 0; L < 1728; ++L) {
        const int ti = L / 144, tj = (L / 12) % 12, tk = L % 12;
        const int on = ti >= 2 && ti <= 10 && tj >= 2 && tj <= 10 && tk >= 2 && tk <= 10;
        const float want = line[ti - 2 > 7 ? 7 : (ti < 2 ? 0 : ti - 2)];
        const int word = (ti * 12 + tj), sign = (int)((bits[word] >> tk) & 1u);
        if (on) {
          if (cells[k] != (uint64_t)L || d[k] != want) ++bad;
          ++k;
        }
        if (sign != (on && want < 0.0f)) ++bad;
      }
      check(bad == 0 && k == 729, "pad: every cell, value and sign bit");
      check(m2s_band_csg(a, r, M2S_CSG_UNION, NULL, NULL, &u) == M2S_ERR_BAD_ARG && u == NULL, "union across grids is refused");
      m2s_band_destroy(r);
    }
    /* move, then union */
    ro.to_source[3] = -1.0f;
    check(m2s_band_resample(a, &g, &ro, NULL, NULL, &r, &info) == M2S_OK && r != NULL, "move");
    if (r) {
      m2s_band* u = NULL;
      check(info.n_cells == 384 && info.n_partial == 0 && info.n_nonfinite == 0, "move: info");
      check(m2s_band_csg(a, r, M2S_CSG_UNION, NULL, NULL, &u) == M2S_OK && u != NULL, "union");
      if (u) {
        check(m2s_band_export(u, cells, d, 1728, bits, NULL) == M2S_OK, "union: export");
        bad = 0;
        for (L = 0; L < 512; ++L) {
          const int i = L / 64;
          const float want = i >= 2 ? line[i - 2] : line[i]; /* the moved solid's value is the smaller one where it exists */
          if (cells[L] != (uint64_t)L || d[L] != want || (int)((bits[L / 8] >> (L % 8)) & 1u) != (want < 0.0f)) ++bad;
        }
        check(bad == 0, "union: every cell, value and sign bit");
        m2s_band_destroy(u);
      }
      m2s_band_destroy(r);
    }
    m2s_band_destroy(a);
  }
  if (failures == 0) printf("all checks passed\n");
  return failures ? 1 : 0;
}
