/* m2s_band_advect from plain C (C99, -Wall -Werror): the declarations compile and link, and every answer that is decided without a
 * handle comes out as include/m2s.h states it.  With an argument (anything) it also moves a band on the GPU: the field x - 2 on every
 * point of an 8 x 8 x 8 grid with cells of 0.5, carried by the velocity (1, 0, 0) for one step of 0.125.  The backward difference along
 * i is 1 everywhere but in the layer i = 0, whose read is clamped, so every other layer becomes its value minus 0.125: the plane
 * moved by 0.125.  With the cells of i >= 4 at rest only the layers 1 .. 3 change.  Prints "all checks passed". */
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
  static float d[512], u[3 * 512];
  static uint32_t bits[64];
  float line[8], want[8];
  m2s_band_field_opts fo, got;
  m2s_band_advect_opts ao;
  m2s_band_advect_info info;
  m2s_band *a = NULL, *r = (m2s_band*)&g; /* any non-NULL value: a failed call must reset it */
  int x, has = 7;
  (void)argv;
  ao.struct_size = sizeof(ao);
  ao.kind = M2S_ADVECT_VELOCITY;
  ao.steps = 1;
  ao.scheme = 0;
  ao.dt = 0.125f;
  check(sizeof(ao) == 20 && sizeof(info) == 48, "the structs' sizes");
  check(m2s_band_advect(NULL, u, &ao, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "NULL handle");
  check(m2s_band_advect(NULL, u, &ao, NULL, NULL, NULL, NULL) == M2S_ERR_BAD_ARG, "NULL out");
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
    check(m2s_band_advect(a, u, NULL, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "NULL opts");
    r = (m2s_band*)&g;
    check(m2s_band_advect(a, NULL, &ao, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "NULL field");
    ao.struct_size = 16;
    r = (m2s_band*)&g;
    check(m2s_band_advect(a, u, &ao, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "struct_size");
    ao.struct_size = sizeof(ao);
    ao.kind = 2;
    r = (m2s_band*)&g;
    check(m2s_band_advect(a, u, &ao, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "a bad kind");
    ao.kind = M2S_ADVECT_VELOCITY;
    ao.steps = 0;
    r = (m2s_band*)&g;
    check(m2s_band_advect(a, u, &ao, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "no steps");
    ao.steps = 1;
    ao.scheme = 1;
    r = (m2s_band*)&g;
    check(m2s_band_advect(a, u, &ao, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "a scheme of 1");
    ao.scheme = 0;
    ao.dt = 0.0f;
    r = (m2s_band*)&g;
    check(m2s_band_advect(a, u, &ao, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "a dt of 0");
    ao.dt = 0.125f;
    fo.background_inside = -1.0f;
    r = (m2s_band*)&g;
    check(m2s_band_advect(a, u, &ao, &fo, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "a negative background");
    for (x = 0; x < 2; ++x) { /* every cell moving, then the cells of i >= 4 at rest */
      const int last = x ? 3 : 7;
      int i, L;
      for (L = 0; L < 512; ++L) {
        u[3 * L] = (L / 64 <= last) ? 1.0f : (L % 2 ? 0.0f : -0.0f);
        u[3 * L + 1] = 0.0f;
        u[3 * L + 2] = -0.0f;
      }
      for (i = 0; i < 8; ++i) want[i] = (i >= 1 && i <= last) ? line[i] - 0.125f * ((1.0f * ((line[i] - line[i - 1]) * 2.0f) + 0.0f) + 0.0f) : line[i];
      memset(&info, 0, sizeof(info));
      info.struct_size = sizeof(info);
      check(m2s_band_advect(a, u, &ao, NULL, NULL, &r, &info) == M2S_OK && r != NULL, "advect");
      if (r) {
        int bad = 0;
        check(info.steps == 1 && info.n_moving == (x ? 256u : 512u) && info.n_changed == (x ? 192u : 448u) && info.n_sign_flips == 0 &&
                  info.n_nonfinite == 0 && info.max_change == 0.125f && info.max_cfl == 0.25f, "info");
        check(m2s_band_info(r, NULL, &k, &bytes) == M2S_OK && k == 512 && bytes == 24 * 8 + 4 * k, "band_info");
        check(m2s_band_field_info(r, &got, &has) == M2S_OK && has == 1 && got.background_outside == 0.75f && got.background_inside == 0.5f,
              "field_info: the input's backgrounds");
        check(m2s_band_export(r, cells, d, 512, bits, NULL) == M2S_OK, "export");
        for (L = 0; L < 512; ++L)
          if (cells[L] != (uint64_t)L || d[L] != want[L / 64] || (int)((bits[L / 8] >> (L % 8)) & 1u) != (want[L / 64] < 0.0f)) ++bad;
        check(bad == 0 && want[0] == line[0] && want[1] == line[1] - 0.125f, "the plane moved by 0.125, the clamped layer and the cells at rest kept every bit");
        for (L = 0; L < 512; ++L) d[L] = line[L / 64];
        m2s_band_destroy(r);
      }
    }
    m2s_band_destroy(a);
  }
  if (failures == 0) printf("all checks passed\n");
  return failures ? 1 : 0;
}
