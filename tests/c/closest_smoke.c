/* The closest-point entry points of include/m2s.h from plain C (C99, -Wall -Werror): one tetrahedron, a few queries and a small
 * grid, host memory.  Prints "all checks passed" when every result is what the geometry says.  Needs a GPU to run. */
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
  uint32_t tri[3];
  float pts[9], dist[3];
  m2s_opts o = {0};
  m2s_timings t;
  o.struct_size = sizeof(m2s_opts);
  o.device = -1;
  o.mem_kind = M2S_MEM_HOST;
  o.synchronous = 1;
  o.timings = &t;
  check(m2s_closest_points(v, 4, idx, 12, 4, M2S_TRIANGLE_LIST, q, 3, tri, pts, dist, &o) == M2S_OK, "m2s_closest_points");
  check(tri[0] == 0 && pts[0] == 0.25f && pts[1] == 0.25f && pts[2] == 0.0f && dist[0] == 2.0f, "below the base");
  check(pts[3] == 1.0f && pts[4] == 0.0f && pts[5] == 0.0f && dist[1] == 1.0f, "beyond a vertex");
  check(tri[1] == 0, "vertex tie: the lowest triangle index");
  check(dist[2] > 0.0f && dist[2] < 0.2f, "inside");
  check(t.n_units == 3 && t.n_triangles == 4, "timings");

  m2s_grid g;
  const float lo[3] = {-1, -1, -1}, hi[3] = {2, 2, 2};
  const uint64_t n[3] = {3, 3, 3};
  uint32_t gt[27];
  float gd[27];
  m2s_grid_from_bounding_box(lo, hi, n, &g);
  check(m2s_grid_closest_points(v, 4, idx, 12, 4, M2S_TRIANGLE_LIST, &g, gt, NULL, gd, NULL) == M2S_OK, "m2s_grid_closest_points");
  check(gt[0] == 0 && fabsf(gd[0] - sqrtf(0.75f)) < 1e-6f, "grid cell (0, 0, 0) -> vertex 0");

  m2s_mesh* mesh = NULL;
  check(m2s_mesh_create(v, 4, idx, 12, 4, M2S_TRIANGLE_LIST, NULL, &mesh) == M2S_OK, "m2s_mesh_create");
  if (mesh) {
    uint32_t mt[3];
    float md[3], mg[27];
    check(m2s_mesh_closest_points(mesh, q, 3, mt, NULL, md, NULL) == M2S_OK && mt[0] == tri[0] && md[2] == dist[2], "m2s_mesh_closest_points");
    check(m2s_mesh_grid_closest_points(mesh, &g, NULL, NULL, mg, NULL) == M2S_OK && mg[13] == gd[13], "m2s_mesh_grid_closest_points");
    m2s_mesh_destroy(mesh);
  }
  if (failures == 0) printf("all checks passed\n");
  return failures ? 1 : 0;
}
