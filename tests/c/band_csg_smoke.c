/* m2s_band_csg / m2s_band_export / m2s_band_field_info from plain C (C99, -Wall -Werror): the declarations compile and link, and every
 * answer that is decided without a handle comes out as include/m2s.h states it.  With an argument (anything) it also combines two band
 * fields on the GPU — the slabs |x - 2| <= 1 and |y - 2| <= 1 of an 8 x 8 x 8 grid, each a band four layers wide — with all three ops,
 * exports the results and compares every grid point with the rules.  Prints "all checks passed". */
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
  static uint64_t cells_a[256], cells_b[256], cells_r[512];
  static float da[256], db[256], dr[512];
  static uint32_t bits_r[64];
  m2s_band_field_opts fo, got;
  m2s_band *a = NULL, *b = NULL, *r = (m2s_band*)&g; /* any non-NULL value: a failed call must reset it */
  int x, has = 7;
  (void)argv;
  check(m2s_band_csg(NULL, NULL, M2S_CSG_UNION, NULL, NULL, &r) == M2S_ERR_BAD_ARG && r == NULL, "NULL handles");
  check(m2s_band_csg(NULL, NULL, M2S_CSG_UNION, NULL, NULL, NULL) == M2S_ERR_BAD_ARG, "NULL out");
  r = (m2s_band*)&g;
  check(m2s_band_csg(NULL, NULL, 3, NULL, NULL, &r) == M2S_ERR_BAD_ARG && r == NULL, "a bad op");
  check(m2s_band_export(NULL, cells_r, dr, 512, bits_r, NULL) == M2S_ERR_BAD_ARG, "export: NULL handle");
  check(m2s_band_export(NULL, NULL, NULL, 512, NULL, NULL) == M2S_ERR_BAD_ARG, "export: no output");
  check(m2s_band_field_info(NULL, &got, &has) == M2S_ERR_BAD_ARG && has == 7, "field_info: NULL handle");
  check(M2S_CSG_UNION == 0 && M2S_CSG_INTERSECTION == 1 && M2S_CSG_DIFFERENCE == 2, "the op values");
  check(m2s_version() == 5, "version");
  if (argc > 1) {
    /* cells of 0.5 starting at 0.25: centres 0.25 ... 3.75.  A: layers i = 2 .. 5 hold |x - 2| - 1; B: layers j = 2 .. 5 hold |y - 2| - 1.
     * Both backgrounds 0.75: beyond the layers both fields are outside and at least that far. */
    int n = 0, m = 0, op;
    for (x = 0; x < 3; ++x) { g.first_cell[x] = 0.25f; g.cell_size[x] = 0.5f; g.cell_count[x] = 8; }
    for (x = 0; x < 512; ++x) {
      const int i = x / 64, j = (x / 8) % 8;
      if (i >= 2 && i <= 5) { cells_a[n] = (uint64_t)x; da[n++] = fabsf(0.25f + 0.5f * (float)i - 2.0f) - 1.0f; }
      if (j >= 2 && j <= 5) { cells_b[m] = (uint64_t)x; db[m++] = fabsf(0.25f + 0.5f * (float)j - 2.0f) - 1.0f; }
    }
    fo.struct_size = sizeof(fo);
    fo.background_outside = 0.75f;
    fo.background_inside = 0.75f;
    check(m2s_band_create(&g, cells_a, da, 256, NULL, &fo, NULL, &a) == M2S_OK && a != NULL, "create A");
    check(m2s_band_create(&g, cells_b, db, 256, NULL, &fo, NULL, &b) == M2S_OK && b != NULL, "create B");
    fo.struct_size = 8;
    check(m2s_band_csg(a, b, M2S_CSG_UNION, &fo, NULL, &r) == M2S_ERR_BAD_ARG && r == NULL, "struct_size");
    fo.struct_size = sizeof(fo);
    fo.background_inside = -1.0f;
    check(m2s_band_csg(a, b, M2S_CSG_UNION, &fo, NULL, &r) == M2S_ERR_BAD_ARG && r == NULL, "a negative background");
    for (op = 0; op < 3 && a && b; ++op) {
      uint64_t k = 0, bytes = 0, at = 0;
      int bad = 0;
      check(m2s_band_csg(a, b, op, NULL, NULL, &r) == M2S_OK && r != NULL, "csg");
      if (!r) break;
      check(m2s_band_info(r, NULL, &k, &bytes) == M2S_OK && k <= 512 && bytes == 24 * 8 + 4 * k, "info");
      check(m2s_band_field_info(r, &got, &has) == M2S_OK && has == 1 && got.struct_size == sizeof(got) && got.background_outside == 0.75f &&
                got.background_inside == 0.75f, "field_info");
      check(m2s_band_export(r, cells_r, dr, k ? k - 1 : 0, bits_r, NULL) == (k ? M2S_ERR_BAD_ARG : M2S_OK), "a short capacity");
      check(m2s_band_export(r, cells_r, dr, 512, bits_r, NULL) == M2S_OK, "export");
      for (x = 0; x < 512; ++x) {
        const int i = x / 64, j = (x / 8) % 8;
        const int act_a = i >= 2 && i <= 5, act_b = j >= 2 && j <= 5;
        const float va = act_a ? fabsf(0.25f + 0.5f * (float)i - 2.0f) - 1.0f : 0.75f;
        float vb = act_b ? fabsf(0.25f + 0.5f * (float)j - 2.0f) - 1.0f : 0.75f;
        float want;
        int active, inside;
        if (op == M2S_CSG_DIFFERENCE) vb = -vb;
        if (op == M2S_CSG_UNION) { want = vb < va ? vb : va; active = (act_a && !(vb < va)) || (act_b && !(va < vb)); }
        else { want = vb > va ? vb : va; active = (act_a && !(vb > va)) || (act_b && !(va > vb)); }
        inside = (int)((bits_r[x / 8] >> (x % 8)) & 1u);
        if (inside != (want < 0.0f)) ++bad; /* the values are never zero here, so s is the sign of the dense op everywhere */
        if (active) {
          if (at >= k || cells_r[at] != (uint64_t)x || dr[at] != want) ++bad;
          ++at;
        }
      }
      check(bad == 0 && at == k, "every grid point follows the rules");
      m2s_band_destroy(r);
      r = NULL;
    }
    m2s_band_destroy(a);
    m2s_band_destroy(b);
  }
  if (failures == 0) printf("all checks passed\n");
  return failures ? 1 : 0;
}
