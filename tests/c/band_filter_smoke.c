/* m2s_band_filter from plain C (C99, -Wall -Werror): the declarations compile and link, and every answer that is decided without a
 * handle comes out as include/m2s.h states it.  With an argument (anything) it also filters a band on the GPU: the field x - 2 on every
 * point of an 8 x 8 x 8 grid with cells of 0.5.  It is linear, so one iteration of M2S_FILTER_MEAN changes only the two layers at the i
 * faces, whose reads are clamped; what they become is computed here with the header's expressions.  With the band as its own region
 * (its inside, x < 2) only the layer i = 0 changes.  Prints "all checks passed". */
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

/* One iteration of M2S_FILTER_MEAN on a field that depends on i alone: the i pass, then the j and k passes, whose three reads agree. */
static void mean_iteration(const float* in, float* out, int first, int last) {
  int i, pass;
  for (i = 0; i < 8; ++i) {
    const float lo = in[i > 0 ? i - 1 : 0], hi = in[i < 7 ? i + 1 : 7];
    out[i] = (i >= first && i <= last) ? ((lo + in[i]) + hi) / 3.0f : in[i];
  }
  for (pass = 0; pass < 2; ++pass)
    for (i = first; i <= last; ++i) out[i] = ((out[i] + out[i]) + out[i]) / 3.0f;
}

int main(int argc, char** argv) {
  m2s_grid g;
  static uint64_t cells[512];
  static float d[512];
  static uint32_t bits[64];
  float line[8], want[8];
  m2s_band_field_opts fo, got;
  m2s_band_filter_opts fl;
  m2s_band_filter_info info;
  m2s_band *a = NULL, *r = (m2s_band*)&g; /* any non-NULL value: a failed call must reset it */
  int x, has = 7;
  (void)argv;
  fl.struct_size = sizeof(fl);
  fl.kind = M2S_FILTER_MEAN;
  fl.iterations = 1;
  fl.width = 1;
  check(sizeof(fl) == 16 && sizeof(info) == 40, "the structs' sizes");
  check(m2s_band_filter(NULL, NULL, &fl, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "NULL handle");
  check(m2s_band_filter(NULL, NULL, &fl, NULL, NULL, NULL, NULL) == M2S_ERR_BAD_ARG, "NULL out");
  check(m2s_version() == 5, "version");
  if (argc > 1) {
    uint64_t k = 0, bytes = 0;
    for (x = 0; x < 3; ++x) { g.first_cell[x] = 0.25f; g.cell_size[x] = 0.5f; g.cell_count[x] = 8; }
    for (x = 0; x < 8; ++x) line[x] = 0.25f + 0.5f * (float)x - 2.0f;
    for (x = 0; x < 512; ++x) { cells[x] = (uint64_t)x; d[x] = line[x / 64]; }
    fo.struct_size = sizeof(fo);
    fo.background_outside = 0.75f;
    fo.background_inside = 0.5f;
    check(m2s_band_create(&g, cells, d, 512, NULL, &fo, NULL, &a) == M2S_OK && a != NULL, "create");
    r = (m2s_band*)&g;
    check(m2s_band_filter(a, NULL, NULL, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "NULL opts");
    fl.struct_size = 12;
    r = (m2s_band*)&g;
    check(m2s_band_filter(a, NULL, &fl, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "struct_size");
    fl.struct_size = sizeof(fl);
    fl.kind = 3;
    r = (m2s_band*)&g;
    check(m2s_band_filter(a, NULL, &fl, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "a bad kind");
    fl.kind = M2S_FILTER_MEAN;
    fl.iterations = 0;
    r = (m2s_band*)&g;
    check(m2s_band_filter(a, NULL, &fl, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "no iterations");
    fl.iterations = 1;
    fl.width = 2;
    r = (m2s_band*)&g;
    check(m2s_band_filter(a, NULL, &fl, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "a width of 2");
    fl.width = 1;
    fo.background_inside = -1.0f;
    r = (m2s_band*)&g;
    check(m2s_band_filter(a, NULL, &fl, &fo, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "a negative background");
    for (x = 0; x < 2; ++x) { /* everywhere, then inside the band itself */
      const int last = x ? 3 : 7;
      mean_iteration(line, want, 0, last);
      memset(&info, 0, sizeof(info));
      info.struct_size = sizeof(info);
      check(m2s_band_filter(a, x ? a : NULL, &fl, NULL, NULL, &r, &info) == M2S_OK && r != NULL, "filter");
      if (r) {
        int bad = 0, L;
        check(info.passes == 3 && info.n_changed == (x ? 64u : 128u) && info.n_sign_flips == 0 && info.n_nonfinite == 0 &&
                  info.max_change == fabsf(want[0] - line[0]), "info");
        check(m2s_band_info(r, NULL, &k, &bytes) == M2S_OK && k == 512 && bytes == 24 * 8 + 4 * k, "band_info");
        check(m2s_band_field_info(r, &got, &has) == M2S_OK && has == 1 && got.background_outside == 0.75f && got.background_inside == 0.5f,
              "field_info: the input's backgrounds");
        check(m2s_band_export(r, cells, d, 512, bits, NULL) == M2S_OK, "export");
        for (L = 0; L < 512; ++L)
          if (cells[L] != (uint64_t)L || d[L] != want[L / 64] || (int)((bits[L / 8] >> (L % 8)) & 1u) != (want[L / 64] < 0.0f)) ++bad;
        check(bad == 0 && want[0] != line[0] && want[1] == line[1], "the faces moved, the rest kept every bit");
        m2s_band_destroy(r);
      }
    }
    m2s_band_destroy(a);
  }
  if (failures == 0) printf("all checks passed\n");
  return failures ? 1 : 0;
}
