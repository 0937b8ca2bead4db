/* m2s_band_create / m2s_band_sample / m2s_band_raymarch from plain C (C99, -Wall -Werror): the declarations compile and link, and every
 * answer that is decided before any device work comes out as include/m2s.h states it.  With an argument (anything) it also builds the band
 * field of the plane d = x - 2 on the GPU from the four layers beside the plane of an 8 x 8 x 8 grid, samples it on the plane and marches a
 * ray onto it.  Prints "all checks passed". */
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
  m2s_grid g, gb;
  static uint64_t cells[256];
  static float d[256];
  uint64_t bad[3] = {5, 4, 9}, dup[3] = {4, 5, 5}, far_[3] = {4, 5, 512};
  float pts[6] = {2.0f, 1.0f, 1.0f, 2.125f, 3.0f, 0.5f}, val[2], nrm[6], hit[4], org[3] = {4.0f, 2.0f, 2.0f}, dir[3] = {-1.0f, 0.0f, 0.0f};
  uint8_t sup[2];
  uint32_t steps[1];
  m2s_band_field_opts fo;
  m2s_sample_opts so;
  m2s_opts o;
  m2s_band* h = (m2s_band*)&g; /* any non-NULL value: a failed create must reset it */
  int x;
  (void)argv;
  /* cells of 0.5 starting at 0.25: centres 0.25 ... 3.75; layers i = 2 .. 5 (x = 1.25 .. 2.75) hold d = x - 2, the background is 0.75 */
  for (x = 0; x < 3; ++x) { g.first_cell[x] = 0.25f; g.cell_size[x] = 0.5f; g.cell_count[x] = 8; }
  for (x = 0; x < 256; ++x) { cells[x] = (uint64_t)(128 + x); d[x] = 0.25f + 0.5f * (float)(2 + x / 64) - 2.0f; }
  fo.struct_size = sizeof(fo);
  fo.background_outside = 0.75f;
  fo.background_inside = 0.75f;
  check(m2s_band_create(NULL, cells, d, 256, NULL, &fo, NULL, &h) == M2S_ERR_BAD_ARG && h == NULL, "NULL grid");
  check(m2s_band_create(&g, cells, d, 256, NULL, &fo, NULL, NULL) == M2S_ERR_BAD_ARG, "NULL out");
  check(m2s_band_create(&g, cells, d, 256, NULL, NULL, NULL, &h) == M2S_ERR_BAD_ARG, "NULL field opts");
  check(m2s_band_create(&g, NULL, d, 256, NULL, &fo, NULL, &h) == M2S_ERR_BAD_ARG, "NULL cells");
  check(m2s_band_create(&g, cells, NULL, 256, NULL, &fo, NULL, &h) == M2S_ERR_BAD_ARG, "NULL distances");
  check(m2s_band_create(&g, cells, d, 513, NULL, &fo, NULL, &h) == M2S_ERR_BAD_ARG, "n_cells above the cell count");
  fo.struct_size = 8;
  check(m2s_band_create(&g, cells, d, 256, NULL, &fo, NULL, &h) == M2S_ERR_BAD_ARG, "struct_size");
  fo.struct_size = sizeof(fo);
  fo.background_inside = -0.5f;
  check(m2s_band_create(&g, cells, d, 256, NULL, &fo, NULL, &h) == M2S_ERR_BAD_ARG, "a negative background");
  fo.background_inside = 0.75f;
  fo.background_outside = INFINITY;
  check(m2s_band_create(&g, cells, d, 256, NULL, &fo, NULL, &h) == M2S_ERR_BAD_ARG, "an infinite background");
  fo.background_outside = 0.75f;
  gb = g;
  gb.cell_count[1] = 0;
  check(m2s_band_create(&gb, cells, d, 1, NULL, &fo, NULL, &h) == M2S_ERR_BAD_ARG, "a zero cell count");
  gb = g;
  gb.cell_count[0] = gb.cell_count[1] = gb.cell_count[2] = 4096; /* 2^36 cells */
  check(m2s_band_create(&gb, cells, d, 1, NULL, &fo, NULL, &h) == M2S_ERR_BAD_ARG, "2^36 cells");
  memset(&o, 0, sizeof(o));
  o.struct_size = sizeof(o);
  o.device = -1;
  o.x_end = 2;
  check(m2s_band_create(&g, cells, d, 256, NULL, &fo, &o, &h) == M2S_ERR_BAD_ARG, "x_end");
  check(m2s_band_create(&g, bad, d, 3, NULL, &fo, NULL, &h) == M2S_ERR_BAD_ARG, "descending cells");
  check(m2s_band_create(&g, dup, d, 3, NULL, &fo, NULL, &h) == M2S_ERR_BAD_ARG, "a duplicate cell");
  check(m2s_band_create(&g, far_, d, 3, NULL, &fo, NULL, &h) == M2S_ERR_BAD_ARG, "a cell at the cell count");
  d[5] = NAN;
  check(m2s_band_create(&g, cells, d, 256, NULL, &fo, NULL, &h) == M2S_ERR_NAN && h == NULL, "a NaN distance");
  d[5] = 0.25f + 0.5f * 2.0f - 2.0f;
  check(m2s_band_sample(NULL, pts, 2, NULL, val, NULL, sup, NULL) == M2S_ERR_BAD_ARG, "sample: NULL handle");
  check(m2s_band_raymarch(NULL, org, dir, 1, NULL, hit, steps, NULL, sup, NULL) == M2S_ERR_BAD_ARG, "raymarch: NULL handle");
  check(m2s_band_info(NULL, NULL, NULL, NULL) == M2S_ERR_BAD_ARG, "info: NULL handle");
  m2s_band_destroy(NULL);
  check(m2s_version() == 5, "version");
  if (argc > 1) {
    uint64_t n = 0, bytes = 0;
    check(m2s_band_create(&g, cells, d, 256, NULL, &fo, NULL, &h) == M2S_OK && h != NULL, "create");
    check(m2s_band_info(h, &gb, &n, &bytes) == M2S_OK && n == 256 && bytes == 16 * 8 + 4 * 256 && gb.cell_count[2] == 8, "info");
    check(m2s_band_sample(h, pts, 2, NULL, NULL, NULL, sup, NULL) == M2S_ERR_BAD_ARG, "support_out alone is no output");
    memset(&so, 0, sizeof(so));
    so.struct_size = sizeof(so);
    so.mode = 7;
    so.max_steps = 100;
    check(m2s_band_sample(h, pts, 2, &so, val, NULL, sup, NULL) == M2S_ERR_BAD_ARG, "a bad mode");
    check(m2s_band_sample(h, pts, 2, NULL, val, nrm, sup, NULL) == M2S_OK, "sample");
    /* trilinear inside the four layers: exactly x - 2, all 8 reads in the band, normal +x */
    check(val[0] == 0.0f && val[1] == 0.125f && sup[0] == 8 && sup[1] == 8, "values and support on the band");
    check(nrm[0] == 1.0f && nrm[1] == 0.0f && nrm[2] == 0.0f, "normal");
    check(m2s_band_raymarch(h, org, dir, 1, NULL, hit, steps, nrm, sup, NULL) == M2S_OK, "raymarch");
    /* from x = 4 against x: 0.75, 0.75 (the background), 0.5 (the band) and the plane: three advances */
    check(hit[0] == 2.0f && hit[1] == 2.0f && hit[2] == 2.0f && hit[3] == 0.0f && steps[0] == 3 && sup[0] == 8, "the march ends on the plane");
    check(nrm[0] == 1.0f, "the hit's normal");
    m2s_band_destroy(h);
  }
  if (failures == 0) printf("all checks passed\n");
  return failures ? 1 : 0;
}
