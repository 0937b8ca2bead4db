/* The grid-query entry points of include/m2s.h from plain C (C99, -Wall -Werror): a small grid of an affine field, host memory.
 * Prints "all checks passed" when every result is what the field says.  Needs a GPU to run. */
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
  /* cells of 0.5 starting at 0.25: centres 0.25, 0.75, ... 3.75; d = x - 2 (a plane facing +x at x = 2) */
  m2s_grid g;
  float d[8 * 8 * 8];
  int x, y, z;
  for (x = 0; x < 3; ++x) { g.first_cell[x] = 0.25f; g.cell_size[x] = 0.5f; g.cell_count[x] = 8; }
  for (x = 0; x < 8; ++x)
    for (y = 0; y < 8; ++y)
      for (z = 0; z < 8; ++z) d[z + y * 8 + x * 64] = 0.25f + 0.5f * (float)x - 2.0f;
  const float pts[] = {1.0f, 1.0f, 1.0f, 3.0f, 2.0f, 1.0f, 9.0f, 1.0f, 1.0f};
  float val[3], nrm[9];
  m2s_sample_opts so = {0};
  m2s_timings t;
  m2s_opts o = {0};
  o.struct_size = sizeof(m2s_opts);
  o.device = -1;
  o.mem_kind = M2S_MEM_HOST;
  o.synchronous = 1;
  o.timings = &t;
  so.struct_size = sizeof(so);
  so.mode = M2S_SAMPLE_TRILINEAR;
  so.iso = 0.0f;
  so.outside = 100.0f;
  so.max_steps = 100;
  check(m2s_sample_grid(&g, d, pts, 3, &so, val, nrm, &o) == M2S_OK, "m2s_sample_grid");
  check(val[0] == -1.0f && val[1] == 1.0f && val[2] == 100.0f, "trilinear values");
  check(nrm[0] == 1.0f && nrm[1] == 0.0f && nrm[2] == 0.0f, "normal along +x");
  check(t.n_units == 3, "timings");
  so.mode = M2S_SAMPLE_TETRAHEDRAL;
  so.iso = 0.5f;
  check(m2s_sample_grid(&g, d, pts, 2, &so, val, NULL, NULL) == M2S_OK && val[0] == -1.5f && val[1] == 0.5f, "tetrahedral at iso 0.5");

  const float org[] = {5.0f, 1.0f, 1.0f, 5.0f, 5.0f, 5.0f};   /* from the +x side (d > 0 there) towards the plane; beside the box */
  const float dir[] = {-1.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f};
  float hit[8];
  uint32_t steps[2];
  so.mode = M2S_SAMPLE_TRILINEAR;
  so.iso = 0.0f;
  check(m2s_raymarch_grid(&g, d, org, dir, 2, &so, hit, steps, nrm, NULL) == M2S_OK, "m2s_raymarch_grid");
  check(fabsf(hit[0] - 2.0f) < 0.01f && hit[3] < 0.005f && steps[0] >= 1 && nrm[0] == 1.0f, "the ray stops on the plane");
  check(hit[4] == 0.0f && hit[7] == 1.0f && steps[1] == 0, "a ray that misses the box");
  so.max_steps = 0;
  check(m2s_raymarch_grid(&g, d, org, dir, 2, &so, hit, steps, NULL, NULL) == M2S_ERR_BAD_ARG, "max_steps 0 is refused");
  if (failures == 0) printf("all checks passed\n");
  return failures ? 1 : 0;
}
