/* The winding-number entry points of include/m2s.h from plain C (C99, -Wall -Werror): one outward-wound tetrahedron, a few queries and a
 * small grid, host memory.  Prints "all checks passed" when every result is what the geometry says.  Needs a GPU to run. */
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
  const float v[] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
  const uint32_t idx[] = {0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3};
  const float q[] = {0.25f, 0.25f, -2.0f, 2.0f, 0.0f, 0.0f, 0.1f, 0.1f, 0.1f};
  float w[3], sdf[3], dist[3];
  m2s_opts o = {0};
  m2s_timings t;
  o.struct_size = sizeof(m2s_opts);
  o.device = -1;
  o.mem_kind = M2S_MEM_HOST;
  o.synchronous = 1;
  o.timings = &t;
  check(m2s_winding_numbers(v, 4, idx, 12, 4, M2S_TRIANGLE_LIST, q, 3, M2S_WINDING_BETA_DEFAULT, 0.5f, w, sdf, &o) == M2S_OK,
        "m2s_winding_numbers");
  check(fabsf(w[0]) < 1e-5f && fabsf(w[1]) < 1e-5f, "outside: w = 0");
  check(fabsf(w[2] - 1.0f) < 1e-5f, "inside: w = 1");
  check(sdf[0] == 2.0f && sdf[1] == 1.0f && sdf[2] < 0.0f, "signed distances");
  check(t.n_units == 3 && t.n_triangles == 4 && t.distance_launches == 2, "timings");
  check(m2s_closest_points(v, 4, idx, 12, 4, M2S_TRIANGLE_LIST, q, 3, NULL, NULL, dist, NULL) == M2S_OK && dist[2] == -sdf[2],
        "|sdf| is the closest-point distance");
  check(m2s_winding_numbers(v, 4, idx, 12, 4, M2S_TRIANGLE_LIST, q, 3, 0.5f, 0.5f, w, NULL, NULL) == M2S_ERR_BAD_ARG, "beta < 1");
  check(m2s_winding_numbers(v, 4, idx, 12, 4, M2S_TRIANGLE_LIST, q, 3, 2.0f, 0.5f, NULL, NULL, NULL) == M2S_ERR_BAD_ARG, "no output");

  m2s_grid g;
  const float lo[3] = {-1, -1, -1}, hi[3] = {2, 2, 2};
  const uint64_t n[3] = {3, 3, 3};
  float gw[27], gs[27];
  m2s_grid_from_bounding_box(lo, hi, n, &g);
  check(m2s_grid_winding_numbers(v, 4, idx, 12, 4, M2S_TRIANGLE_LIST, &g, INFINITY, 0.5f, gw, gs, NULL) == M2S_OK, "m2s_grid_winding_numbers");
  check(fabsf(gw[0]) < 1e-5f && fabsf(gs[0] - sqrtf(0.75f)) < 1e-6f, "grid cell (0, 0, 0): outside, nearest is vertex 0");

  m2s_mesh* mesh = NULL;
  check(m2s_mesh_create(v, 4, idx, 12, 4, M2S_TRIANGLE_LIST, NULL, &mesh) == M2S_OK, "m2s_mesh_create");
  if (mesh) {
    float mw[3], mg[27];
    check(m2s_mesh_winding_numbers(mesh, q, 3, M2S_WINDING_BETA_DEFAULT, 0.5f, mw, NULL, NULL) == M2S_OK && fabsf(mw[2] - 1.0f) < 1e-5f,
          "m2s_mesh_winding_numbers");
    check(m2s_mesh_grid_winding_numbers(mesh, &g, M2S_WINDING_BETA_DEFAULT, 0.5f, NULL, mg, NULL) == M2S_OK && mg[0] == gs[0],
          "m2s_mesh_grid_winding_numbers");
    m2s_mesh_destroy(mesh);
  }
  if (failures == 0) printf("all checks passed\n");
  return failures ? 1 : 0;
}
