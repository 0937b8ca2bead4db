/* m2s_band_measure from plain C (C99, -Wall -Werror): the declarations compile and link, and every answer that is decided without a handle
 * comes out as include/m2s.h states it.  With an argument (anything) it also measures on the GPU, on an 8 x 8 x 8 grid of cells 0.5: the 27
 * points (3..5)^3 with the value +1 and -1 at the centre, whose zero set is the octahedron with vertices half a cell along the axes.  Every
 * term of its sums is exact: 8 triangles, 6 vertices, six times the volume 1 at a scale of 2^20, 24 times the moment 2 / 3 at 2^8.
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
  static uint64_t cells[27];
  static float d[27];
  static uint32_t labels[27];
  m2s_band_measure_opts mo;
  m2s_band_measure_record m[2];
  m2s_band_measure_info info;
  m2s_timings tm;
  m2s_band_field_opts fo;
  m2s_band* a = NULL;
  int x;
  (void)argv;
  for (x = 0; x < 3; ++x) { g.first_cell[x] = 0.25f; g.cell_size[x] = 0.5f; g.cell_count[x] = 8; }
  mo.struct_size = sizeof(mo);
  mo.iso = 0.0f;
  info.struct_size = sizeof(info);
  check(sizeof(m2s_band_measure_record) == 112 && sizeof(mo) == 8 && sizeof(info) == 24, "the structs' sizes");
  check(m2s_band_measure(NULL, &mo, NULL, 0, NULL, m, &info, NULL) == M2S_ERR_BAD_ARG, "NULL handle");
  check(m2s_band_measure((const m2s_band*)&g, &mo, NULL, 0, NULL, NULL, &info, NULL) == M2S_ERR_BAD_ARG, "NULL measures_out");
  mo.struct_size = 4;
  check(m2s_band_measure((const m2s_band*)&g, &mo, NULL, 0, NULL, m, &info, NULL) == M2S_ERR_BAD_ARG, "the options' struct_size");
  mo.struct_size = sizeof(mo);
  mo.iso = (float)NAN;
  check(m2s_band_measure((const m2s_band*)&g, &mo, NULL, 0, NULL, m, &info, NULL) == M2S_ERR_BAD_ARG, "a NaN iso");
  mo.iso = 0.0f;
  info.struct_size = 16;
  check(m2s_band_measure((const m2s_band*)&g, &mo, NULL, 0, NULL, m, &info, NULL) == M2S_ERR_BAD_ARG, "the info's struct_size");
  info.struct_size = sizeof(info);
  check(m2s_band_measure((const m2s_band*)&g, &mo, labels, 0, NULL, m, &info, NULL) == M2S_ERR_BAD_ARG, "labels with no groups");
  if (argc > 1) {
    const uint64_t w = (uint64_t)floor((double)sqrtf(0.01171875f) * 67108864.0);   /* |(1/16, 1/16, 1/16)| at 2^(24 - E), E = -2 */
    int n = 0, i, j, k;
    for (i = 3; i <= 5; ++i)
      for (j = 3; j <= 5; ++j)
        for (k = 3; k <= 5; ++k) {
          cells[n] = (uint64_t)(k + 8 * j + 64 * i);
          d[n] = (i == 4 && j == 4 && k == 4) ? -1.0f : 1.0f;
          labels[n] = n < 13 ? 1u : (n == 26 ? M2S_LABEL_NONE : 0u);   /* the cells based at the first 13 points, the rest, and one left out */
          ++n;
        }
    fo.struct_size = sizeof(fo);
    fo.background_outside = 1.0f;
    fo.background_inside = 1.0f;
    check(m2s_band_create(&g, cells, d, 27, NULL, &fo, NULL, &a) == M2S_OK && a != NULL, "create");
    memset(m, 0xee, sizeof(m));
    memset(&tm, 0xee, sizeof(tm));
    check(m2s_band_measure(a, &mo, NULL, 0, NULL, m, &info, &tm) == M2S_OK, "measure");
    check(m[0].n_triangles == 8 && m[0].n_vertices == 6 && m[0].n_open == 0 && m[0].n_border == 0, "the counts");
    check(m[0].volume_q == 1048576 && m[0].moment_q[0] == 4096 && m[0].moment_q[1] == 4096 && m[0].moment_q[2] == 4096 && m[0].area_q == 8 * w, "the raw sums");
    check(m[0].volume == 0.125 / 6 && m[0].centroid[0] == 2.25 && m[0].centroid[1] == 2.25 && m[0].centroid[2] == 2.25, "volume and centroid");
    check(fabs(m[0].area - 4.0 * sqrt(0.01171875)) < 1e-7 && m[0].area == ldexp((double)m[0].area_q, -27), "the area");
    check(info.area_exponent == -2 && info.n_groups == 1 && info.n_skipped == 0, "the info");
    check(tm.total_ms > 0.0f && tm.total_ms == tm.distance_ms && tm.n_units == 27, "the timings");
    check(m2s_band_measure(a, NULL, labels, 2, NULL, m, &info, NULL) == M2S_OK && info.n_groups == 2 && info.n_skipped == 1, "two groups");
    check(m[0].n_triangles + m[1].n_triangles == 8 && m[0].n_vertices + m[1].n_vertices == 6 && m[0].volume_q + m[1].volume_q == 1048576 &&
              m[0].area_q + m[1].area_q == 8 * w && m[0].moment_q[2] + m[1].moment_q[2] == 4096 && m[1].n_triangles > 0 && m[0].n_triangles > 0,
          "the groups sum to the whole");
    mo.iso = 5.0f;   /* no crossing */
    check(m2s_band_measure(a, &mo, NULL, 0, NULL, m, NULL, NULL) == M2S_OK && m[0].n_triangles == 0 && m[0].area == 0.0 && m[0].volume == 0.0 &&
              m[0].centroid[0] != m[0].centroid[0], "nothing to measure: zeros and a NaN centroid");
    m2s_band_destroy(a);
  }
  if (failures == 0) printf("all checks passed\n");
  return failures ? 1 : 0;
}
