/* The ray entry points of include/m2s.h from plain C (C99, -Wall -Werror): the unit cube's twelve triangles, a handful of rays, host
 * memory.  Prints "all checks passed" when every result is what the geometry says.  Needs a GPU to run. */
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
  /* vertex index = 4x + 2y + z over {-1, 1}^3; faces -x +x -y +y -z +z, outward */
  const float v[] = {-1, -1, -1, -1, -1, 1, -1, 1, -1, -1, 1, 1, 1, -1, -1, 1, -1, 1, 1, 1, -1, 1, 1, 1};
  const uint32_t idx[] = {0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3};
  /* down onto the +z face; along its diagonal (the shared edge); past the cube; from inside; a zero direction */
  const float org[] = {0.25f, 0.5f, 3, 0.5f, 0.5f, 3, 2, 2, 3, 0, 0.25f, 0.5f, 0, 0, 3};
  const float dir[] = {0, 0, -1, 0, 0, -2, 0, 0, -1, 1, 0, 0, 0, 0, 0};
  float t[5], uv[10];
  uint32_t tri[5], count[5];
  uint8_t occ[5];
  m2s_opts o = {0};
  m2s_timings tm;
  o.struct_size = sizeof(m2s_opts);
  o.device = -1;
  o.mem_kind = M2S_MEM_HOST;
  o.synchronous = 1;
  o.timings = &tm;
  check(m2s_cast_rays(v, 8, idx, 36, 4, M2S_TRIANGLE_LIST, org, dir, 5, NULL, t, tri, uv, count, occ, &o) == M2S_OK, "m2s_cast_rays");
  check(t[0] == 2.0f && count[0] == 2 && occ[0] == 1 && (tri[0] == 10 || tri[0] == 11), "ray 0: the +z face at t = 2, out again at 4");
  check(t[1] == 1.0f && count[1] == 4 && tri[1] == 10, "ray 1: the shared edge counts both triangles of each face; |d| = 2 halves t");
  check(isinf(t[2]) && count[2] == 0 && occ[2] == 0 && tri[2] == UINT32_MAX && isnan(uv[4]) && isnan(uv[5]), "ray 2: a miss");
  check(t[3] == 1.0f && count[3] == 1 && (tri[3] == 2 || tri[3] == 3), "ray 3: from inside, the +x face");
  check(isinf(t[4]) && count[4] == 0 && occ[4] == 0, "ray 4: a zero direction hits nothing");
  check(tm.n_units == 5 && tm.n_triangles == 12 && tm.distance_launches == 1, "timings");
  {
    const float a[3] = {v[3 * idx[3 * tri[0]]], v[3 * idx[3 * tri[0]] + 1], v[3 * idx[3 * tri[0]] + 2]};
    const float* b = v + 3 * idx[3 * tri[0] + 1];
    const float* c = v + 3 * idx[3 * tri[0] + 2];
    const float x = a[0] + uv[0] * (b[0] - a[0]) + uv[1] * (c[0] - a[0]), y = a[1] + uv[0] * (b[1] - a[1]) + uv[1] * (c[1] - a[1]);
    check(fabsf(x - 0.25f) < 1e-6f && fabsf(y - 0.5f) < 1e-6f, "uv rebuilds the hit point");
  }
  {
    const m2s_ray_opts ro = {sizeof(m2s_ray_opts), 2.5f, 4.0f};
    const m2s_ray_opts bad = {sizeof(m2s_ray_opts), 2.0f, 1.0f};
    check(m2s_cast_rays(v, 8, idx, 36, 4, M2S_TRIANGLE_LIST, org, dir, 5, &ro, t, NULL, NULL, count, NULL, NULL) == M2S_OK, "a range");
    check(t[0] == 4.0f && count[0] == 1 && isinf(t[3]), "[2.5, 4]: the far face only, its end included");
    check(m2s_cast_rays(v, 8, idx, 36, 4, M2S_TRIANGLE_LIST, org, dir, 5, &bad, t, NULL, NULL, NULL, NULL, NULL) == M2S_ERR_BAD_ARG, "t_min > t_max");
    check(m2s_cast_rays(v, 8, idx, 36, 4, M2S_TRIANGLE_LIST, org, dir, 5, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == M2S_ERR_BAD_ARG, "no output");
  }
  {
    m2s_mesh* mesh = NULL;
    uint8_t mocc[5];
    float mt[5];
    check(m2s_mesh_create(v, 8, idx, 36, 4, M2S_TRIANGLE_LIST, NULL, &mesh) == M2S_OK, "m2s_mesh_create");
    if (mesh) {
      check(m2s_mesh_cast_rays(mesh, org, dir, 5, NULL, NULL, NULL, NULL, NULL, mocc, NULL) == M2S_OK, "m2s_mesh_cast_rays (occluded only)");
      check(mocc[0] == 1 && mocc[1] == 1 && mocc[2] == 0 && mocc[3] == 1 && mocc[4] == 0, "occlusion flags");
      check(m2s_mesh_cast_rays(mesh, org, dir, 5, NULL, mt, NULL, NULL, NULL, NULL, NULL) == M2S_OK && mt[0] == 2.0f && mt[3] == 1.0f,
            "m2s_mesh_cast_rays (t only)");
      m2s_mesh_destroy(mesh);
    }
  }
  if (failures == 0) printf("all checks passed\n");
  return failures ? 1 : 0;
}
