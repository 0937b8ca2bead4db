/* m2s_grid_isosurface of include/m2s.h from plain C (C99, -Wall -Werror): the plane d = x - 2 on a small grid, host memory.
 * Prints "all checks passed" when the mesh is what the field says.  Needs a GPU to run. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "m2s.h"

static int failures = 0;
static void check(int ok, const char* what) {
  if (!ok) {
    printf("FAIL %s (%s)\n", what, m2s_last_error());
    ++failures;
  }
}

int main(void) {
  /* cells of 0.5 starting at 0.25: centres 0.25, 0.75, ... 3.75; d = x - 2 crosses between x = 1.75 (i = 3) and 2.25 (i = 4) */
  m2s_grid g;
  float d[8 * 8 * 8];
  int x, y, z;
  for (x = 0; x < 3; ++x) { g.first_cell[x] = 0.25f; g.cell_size[x] = 0.5f; g.cell_count[x] = 8; }
  for (x = 0; x < 8; ++x)
    for (y = 0; y < 8; ++y)
      for (z = 0; z < 8; ++z) d[z + y * 8 + x * 64] = 0.25f + 0.5f * (float)x - 2.0f;
  static float v[3 * 64];
  static uint32_t t[3 * 98];
  uint64_t counts[2] = {7, 7};
  m2s_timings tm;
  m2s_opts o = {0};
  o.struct_size = sizeof(m2s_opts);
  o.device = -1;
  o.mem_kind = M2S_MEM_HOST;
  o.synchronous = 1;
  o.timings = &tm;
  check(m2s_grid_isosurface(&g, d, 0.0f, NULL, 0, NULL, 0, counts, &o) == M2S_OK, "count");
  check(counts[0] == 64 && counts[1] == 98 && tm.n_units == 512, "one vertex per x-edge of layer 3, two triangles per cell");
  check(m2s_grid_isosurface(&g, d, 0.0f, v, 64, t, 97, counts, NULL) == M2S_ERR_BAD_ARG && counts[1] == 98, "capacity");
  check(m2s_grid_isosurface(&g, d, 0.0f, v, 64, t, 98, counts, NULL) == M2S_OK, "fill");
  {
    int ok = 1, i;
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
  }
  d[100] = NAN;
  check(m2s_grid_isosurface(&g, d, 0.0f, v, 64, t, 98, counts, NULL) == M2S_ERR_NAN, "NaN");
  check(m2s_grid_isosurface(&g, d, 0.0f, v, 64, NULL, 98, counts, NULL) == M2S_ERR_BAD_ARG, "one output NULL");
  if (failures == 0) printf("all checks passed\n");
  return failures ? 1 : 0;
}
