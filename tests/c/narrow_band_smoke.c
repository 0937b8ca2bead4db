/* m2s_narrow_band_sdf / m2s_mesh_narrow_band_sdf from plain C (C99, -Wall -Werror): the declarations compile and link, and every answer
 * that is decided before any device work comes out as include/m2s.h states it.  With an argument (anything) it also takes the band of
 * half a cell around a tetrahedron's two faces in a 4 x 4 x 4 grid on the GPU and checks cells, distances, bits and the count against the
 * dense m2s_generate_grid_sdf of the same call.  Prints "all checks passed". */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "m2s.h"

int main(int argc, char** argv) {
  const float v[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
  const uint32_t idx[6] = {0, 1, 2, 0, 2, 3};
  const uint32_t bad_idx[6] = {0, 1, 2, 0, 2, 4};
  m2s_grid g = {{0.125f, 0.125f, 0.125f}, {0.25f, 0.25f, 0.25f}, {4, 4, 4}};
  m2s_grid gb;
  m2s_band_opts bo = {sizeof(m2s_band_opts), 0.125f, 0.125f};
  m2s_opts o;
  uint32_t bits[16];
  uint64_t cells[64], n_active = 99;
  float dist[64];
  int failures = 0;
  /* every output NULL; NULL grid; NULL mesh; NULL widths */
  if (m2s_narrow_band_sdf(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &g, M2S_SIGN_NORMAL, &bo, NULL, NULL, 0, NULL, NULL, NULL) != M2S_ERR_BAD_ARG) ++failures;
  if (m2s_narrow_band_sdf(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, NULL, M2S_SIGN_NORMAL, &bo, cells, dist, 64, bits, &n_active, NULL) != M2S_ERR_BAD_ARG) ++failures;
  if (m2s_mesh_narrow_band_sdf(NULL, &g, M2S_SIGN_NORMAL, &bo, cells, dist, 64, bits, &n_active, NULL) != M2S_ERR_BAD_ARG) ++failures;
  if (m2s_narrow_band_sdf(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &g, M2S_SIGN_NORMAL, NULL, cells, dist, 64, bits, &n_active, NULL) != M2S_ERR_BAD_ARG) ++failures;
  if (m2s_narrow_band_sdf(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &g, 7, &bo, cells, dist, 64, bits, &n_active, NULL) != M2S_ERR_BAD_ARG) ++failures;
  bo.exterior = -0.5f;
  if (m2s_narrow_band_sdf(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &g, M2S_SIGN_NORMAL, &bo, cells, dist, 64, bits, &n_active, NULL) != M2S_ERR_BAD_ARG) ++failures;
  bo.exterior = 0.125f;
  bo.interior = NAN;
  if (m2s_narrow_band_sdf(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &g, M2S_SIGN_NORMAL, &bo, cells, dist, 64, bits, &n_active, NULL) != M2S_ERR_BAD_ARG) ++failures;
  bo.interior = 0.125f;
  bo.struct_size = 8;
  if (m2s_narrow_band_sdf(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &g, M2S_SIGN_NORMAL, &bo, cells, dist, 64, bits, &n_active, NULL) != M2S_ERR_BAD_ARG) ++failures;
  bo.struct_size = sizeof(m2s_band_opts);
  gb = g;
  gb.cell_count[1] = 0;
  if (m2s_narrow_band_sdf(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &gb, M2S_SIGN_NORMAL, &bo, cells, dist, 64, bits, &n_active, NULL) != M2S_ERR_BAD_ARG) ++failures;
  gb = g;
  gb.cell_size[2] = 0.0f;
  if (m2s_narrow_band_sdf(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &gb, M2S_SIGN_NORMAL, &bo, cells, dist, 64, bits, &n_active, NULL) != M2S_ERR_BAD_ARG) ++failures;
  if (m2s_narrow_band_sdf(v, 4, bad_idx, 6, 4, M2S_TRIANGLE_LIST, &g, M2S_SIGN_NORMAL, &bo, cells, dist, 64, bits, &n_active, NULL) != M2S_ERR_BAD_ARG) ++failures;
  memset(&o, 0, sizeof(o));
  o.struct_size = sizeof(o);
  o.device = -1;
  o.synchronous = 1;
  o.x_end = 2;
  if (m2s_narrow_band_sdf(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &g, M2S_SIGN_NORMAL, &bo, cells, dist, 64, bits, &n_active, &o) != M2S_ERR_BAD_ARG) ++failures;
  if (n_active != 99) ++failures; /* no failed argument check writes it */
  if (m2s_version() != 5) ++failures;
  if (argc > 1) {
    float dense[64];
    uint64_t i, seen = 0;
    uint32_t k;
    if (m2s_generate_grid_sdf(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &g, M2S_SIGN_NORMAL, dense, NULL) != M2S_OK) ++failures;
    if (m2s_narrow_band_sdf(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &g, M2S_SIGN_NORMAL, &bo, cells, dist, 64, bits, &n_active, NULL) != M2S_OK) ++failures;
    for (i = 0; i < 64; ++i) {
      const int want = -bo.interior <= dense[i] && dense[i] <= bo.exterior;
      const uint32_t bit = (bits[i / 4] >> (i % 4)) & 1u; /* nzw = 1: word (i, j), bit k */
      if (bit != (uint32_t)want) ++failures;
      if (want) {
        if (seen >= n_active || cells[seen] != i || memcmp(&dist[seen], &dense[i], 4) != 0) ++failures;
        ++seen;
      }
    }
    if (seen != n_active || seen == 0 || seen == 64) ++failures;
    for (k = 0; k < 16; ++k)
      if (bits[k] >> 4) ++failures; /* padding bits */
    n_active = 0;
    cells[0] = 12345;
    dist[0] = -7.0f;
    if (m2s_narrow_band_sdf(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &g, M2S_SIGN_NORMAL, &bo, cells, dist, seen - 1, NULL, &n_active, NULL) != M2S_ERR_BAD_ARG) ++failures;
    if (n_active != seen || cells[0] != 12345 || dist[0] != -7.0f) ++failures;
  }
  printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
