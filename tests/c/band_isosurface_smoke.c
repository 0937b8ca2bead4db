/* m2s_band_isosurface from plain C (C99, -Wall -Werror): the declaration compiles and links, and every answer that is decided before any
 * device work comes out as include/m2s.h states it — host-memory lists that do not ascend or run past the grid included.  With an argument
 * (anything) it also extracts the plane d = x - 2 on the GPU from an 8 x 8 x 8 grid three times: with every point active (the dense mesh),
 * with the two layers beside the plane only (the same mesh), and with half of the upper layer missing (fewer triangles, n_open > 0).
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
  /* cells of 0.5 starting at 0.25: centres 0.25, 0.75, ... 3.75; d = x - 2 crosses between x = 1.75 (i = 3) and 2.25 (i = 4) */
  m2s_grid g, gb;
  static uint64_t cells[512];
  static float d[512], v[3 * 64];
  static uint32_t t[3 * 98];
  uint64_t counts[3] = {7, 7, 7}, bad[3] = {5, 4, 9}, dup[3] = {4, 5, 5}, far_[3] = {4, 5, 512};
  m2s_opts o;
  int x;
  (void)argv;
  for (x = 0; x < 3; ++x) { g.first_cell[x] = 0.25f; g.cell_size[x] = 0.5f; g.cell_count[x] = 8; }
  for (x = 0; x < 512; ++x) { cells[x] = (uint64_t)x; d[x] = 0.25f + 0.5f * (float)(x / 64) - 2.0f; }
  check(m2s_band_isosurface(NULL, cells, d, 512, 0.0f, NULL, 0, NULL, 0, counts, NULL) == M2S_ERR_BAD_ARG, "NULL grid");
  check(m2s_band_isosurface(&g, cells, d, 512, 0.0f, NULL, 0, NULL, 0, NULL, NULL) == M2S_ERR_BAD_ARG, "NULL counts");
  check(m2s_band_isosurface(&g, NULL, d, 512, 0.0f, NULL, 0, NULL, 0, counts, NULL) == M2S_ERR_BAD_ARG, "NULL cells");
  check(m2s_band_isosurface(&g, cells, NULL, 512, 0.0f, NULL, 0, NULL, 0, counts, NULL) == M2S_ERR_BAD_ARG, "NULL distances");
  check(m2s_band_isosurface(&g, cells, d, 513, 0.0f, NULL, 0, NULL, 0, counts, NULL) == M2S_ERR_BAD_ARG, "n_cells above the cell count");
  check(m2s_band_isosurface(&g, cells, d, 512, 0.0f, v, 64, NULL, 98, counts, NULL) == M2S_ERR_BAD_ARG, "one output NULL");
  check(m2s_band_isosurface(&g, cells, d, 512, NAN, NULL, 0, NULL, 0, counts, NULL) == M2S_ERR_BAD_ARG, "NaN iso");
  gb = g;
  gb.cell_count[1] = 0;
  check(m2s_band_isosurface(&gb, cells, d, 1, 0.0f, NULL, 0, NULL, 0, counts, NULL) == M2S_ERR_BAD_ARG, "a zero cell count");
  gb = g;
  gb.cell_size[2] = 0.0f;
  check(m2s_band_isosurface(&gb, cells, d, 1, 0.0f, NULL, 0, NULL, 0, counts, NULL) == M2S_ERR_BAD_ARG, "a cell size of 0");
  gb = g;
  gb.cell_count[0] = gb.cell_count[1] = gb.cell_count[2] = 4096; /* 2^36 cells */
  check(m2s_band_isosurface(&gb, cells, d, 1, 0.0f, NULL, 0, NULL, 0, counts, NULL) == M2S_ERR_BAD_ARG, "2^36 cells");
  memset(&o, 0, sizeof(o));
  o.struct_size = sizeof(o);
  o.device = -1;
  o.x_end = 2;
  check(m2s_band_isosurface(&g, cells, d, 512, 0.0f, NULL, 0, NULL, 0, counts, &o) == M2S_ERR_BAD_ARG, "x_end");
  check(m2s_band_isosurface(&g, bad, d, 3, 0.0f, NULL, 0, NULL, 0, counts, NULL) == M2S_ERR_BAD_ARG, "descending cells");
  check(m2s_band_isosurface(&g, dup, d, 3, 0.0f, NULL, 0, NULL, 0, counts, NULL) == M2S_ERR_BAD_ARG, "a duplicate cell");
  check(m2s_band_isosurface(&g, far_, d, 3, 0.0f, NULL, 0, NULL, 0, counts, NULL) == M2S_ERR_BAD_ARG, "a cell at the cell count");
  check(counts[0] == 7 && counts[1] == 7 && counts[2] == 7, "no failed argument check writes counts");
  check(m2s_band_isosurface(&g, NULL, NULL, 0, 0.0f, NULL, 0, NULL, 0, counts, NULL) == M2S_OK && counts[0] == 0 && counts[1] == 0 && counts[2] == 0,
        "an empty band");
  check(m2s_version() == 5, "version");
  if (argc > 1) {
    m2s_timings tm;
    int i, ok = 1;
    uint64_t n;
    memset(&o, 0, sizeof(o));
    o.struct_size = sizeof(o);
    o.device = -1;
    o.mem_kind = M2S_MEM_HOST;
    o.synchronous = 1;
    o.timings = &tm;
    check(m2s_band_isosurface(&g, cells, d, 512, 0.0f, NULL, 0, NULL, 0, counts, &o) == M2S_OK, "count");
    check(counts[0] == 64 && counts[1] == 98 && counts[2] == 0 && tm.n_units == 512, "every point active: the dense counts");
    check(m2s_band_isosurface(&g, cells, d, 512, 0.0f, v, 64, t, 97, counts, NULL) == M2S_ERR_BAD_ARG && counts[1] == 98, "capacity");
    /* layers i = 3 and 4 only */
    for (x = 0; x < 128; ++x) { cells[x] = (uint64_t)(192 + x); d[x] = 0.25f + 0.5f * (float)(3 + x / 64) - 2.0f; }
    check(m2s_band_isosurface(&g, cells, d, 128, 0.0f, v, 64, t, 98, counts, NULL) == M2S_OK, "fill");
    check(counts[0] == 64 && counts[1] == 98 && counts[2] == 0, "two layers: the same counts");
    for (i = 0; i < 64; ++i) ok &= v[3 * i] == 2.0f && v[3 * i + 1] == 0.25f + 0.5f * (float)(i / 8) && v[3 * i + 2] == 0.25f + 0.5f * (float)(i % 8);
    check(ok, "vertex positions");
    ok = 1;
    for (i = 0; i < 98; ++i) {
      const float* a = v + 3 * t[3 * i];
      const float* b = v + 3 * t[3 * i + 1];
      const float* c = v + 3 * t[3 * i + 2];
      const float nx = (b[1] - a[1]) * (c[2] - a[2]) - (b[2] - a[2]) * (c[1] - a[1]);
      ok &= t[3 * i] < 64 && t[3 * i + 1] < 64 && t[3 * i + 2] < 64 && nx > 0.0f;
    }
    check(ok, "triangles face +x, towards increasing d");
    /* layer 3 and the rows j < 4 of layer 4: 32 vertices, the cells with j < 3 complete, the row j = 3 cut but incomplete */
    n = 64 + 32;
    check(m2s_band_isosurface(&g, cells, d, n, 0.0f, v, 64, t, 98, counts, NULL) == M2S_OK, "a band too narrow");
    check(counts[0] == 32 && counts[1] == 2 * 3 * 7 && counts[2] == 7, "a band too narrow: counts and n_open");
    d[5] = NAN;
    check(m2s_band_isosurface(&g, cells, d, 128, 0.0f, v, 64, t, 98, counts, NULL) == M2S_ERR_NAN && counts[0] == 0 && counts[2] == 0, "NaN");
    d[5] = INFINITY;
    check(m2s_band_isosurface(&g, cells, d, 128, 0.0f, v, 64, t, 98, counts, NULL) == M2S_ERR_NAN, "inf");
  }
  if (failures == 0) printf("all checks passed\n");
  return failures ? 1 : 0;
}
