/* m2s_sample_surface / m2s_mesh_sample_surface from plain C (C99, -Wall -Werror): the declarations compile and link, and every answer
 * that is decided before any device work comes out as include/m2s.h states it.  Needs no GPU.  Prints "all checks passed". */
#include <stdint.h>
#include <stdio.h>

#include "m2s.h"

int main(void) {
  const float v[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
  const uint32_t idx[6] = {0, 1, 2, 0, 2, 3};
  float point[12], uv[8], normal[12];
  uint32_t tri[4];
  double area = -1.0;
  int failures = 0;
  m2s_surface_sample_opts so = {sizeof(m2s_surface_sample_opts), 0, 7, 0};
  /* every output NULL */
  if (m2s_sample_surface(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, 4, &so, NULL, NULL, NULL, NULL, NULL, NULL) != M2S_ERR_BAD_ARG) ++failures;
  so.reserved = 1;
  if (m2s_sample_surface(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, 4, &so, point, tri, uv, normal, &area, NULL) != M2S_ERR_BAD_ARG) ++failures;
  so.reserved = 0;
  so.struct_size = 8;
  if (m2s_sample_surface(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, 4, &so, point, tri, uv, normal, &area, NULL) != M2S_ERR_BAD_ARG) ++failures;
  so.struct_size = sizeof(m2s_surface_sample_opts);
  so.first_sample = UINT64_MAX - 2;
  if (m2s_sample_surface(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, 4, &so, point, tri, uv, normal, &area, NULL) != M2S_ERR_BAD_ARG) ++failures;
  so.first_sample = 0;
  /* a mesh without triangles: area 0; M2S_OK without samples, M2S_ERR_EMPTY_MESH with */
  if (m2s_sample_surface(v, 2, NULL, 0, 4, M2S_TRIANGLE_LIST, 0, &so, NULL, NULL, NULL, NULL, &area, NULL) != M2S_OK || area != 0.0) ++failures;
  area = -1.0;
  if (m2s_sample_surface(v, 2, NULL, 0, 4, M2S_TRIANGLE_LIST, 4, &so, point, tri, uv, normal, &area, NULL) != M2S_ERR_EMPTY_MESH || area != 0.0) ++failures;
  if (m2s_mesh_sample_surface(NULL, 4, &so, point, tri, uv, normal, &area, NULL) != M2S_ERR_BAD_ARG) ++failures;
  if (m2s_version() != 5) ++failures;
  printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
