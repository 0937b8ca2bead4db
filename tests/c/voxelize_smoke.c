/* m2s_voxelize / m2s_mesh_voxelize from plain C (C99, -Wall -Werror): the declarations compile and link, and every answer that is
 * decided before any device work comes out as include/m2s.h states it.  With an argument (the expected number of set cells) it also
 * voxelizes a tetrahedron's two faces into a 4 x 4 x 4 grid on the GPU and checks bits, bytes, cells and the count against each other.
 * Prints "all checks passed". */
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
  m2s_voxelize_opts vo = {sizeof(m2s_voxelize_opts), M2S_VOXELIZE_SURFACE};
  m2s_opts o;
  uint32_t bits[16];
  uint8_t occ[64];
  uint64_t cells[64], n_set = 99;
  int failures = 0;
  /* every output NULL; NULL grid; NULL mesh */
  if (m2s_voxelize(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &g, &vo, NULL, NULL, NULL, 0, NULL, NULL) != M2S_ERR_BAD_ARG) ++failures;
  if (m2s_voxelize(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, NULL, &vo, bits, occ, cells, 64, &n_set, NULL) != M2S_ERR_BAD_ARG) ++failures;
  if (m2s_mesh_voxelize(NULL, &g, &vo, bits, occ, cells, 64, &n_set, NULL) != M2S_ERR_BAD_ARG) ++failures;
  vo.mode = 2;
  if (m2s_voxelize(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &g, &vo, bits, occ, cells, 64, &n_set, NULL) != M2S_ERR_BAD_ARG) ++failures;
  vo.mode = M2S_VOXELIZE_SOLID;
  vo.struct_size = 4;
  if (m2s_voxelize(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &g, &vo, bits, occ, cells, 64, &n_set, NULL) != M2S_ERR_BAD_ARG) ++failures;
  vo.struct_size = sizeof(m2s_voxelize_opts);
  gb = g;
  gb.cell_count[1] = 0;
  if (m2s_voxelize(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &gb, &vo, bits, occ, cells, 64, &n_set, NULL) != M2S_ERR_BAD_ARG) ++failures;
  gb = g;
  gb.cell_size[2] = 0.0f;
  if (m2s_voxelize(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &gb, &vo, bits, occ, cells, 64, &n_set, NULL) != M2S_ERR_BAD_ARG) ++failures;
  gb.cell_size[2] = -0.25f;
  if (m2s_voxelize(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &gb, &vo, bits, occ, cells, 64, &n_set, NULL) != M2S_ERR_BAD_ARG) ++failures;
  if (m2s_voxelize(v, 4, bad_idx, 6, 4, M2S_TRIANGLE_LIST, &g, &vo, bits, occ, cells, 64, &n_set, NULL) != M2S_ERR_BAD_ARG) ++failures;
  memset(&o, 0, sizeof(o));
  o.struct_size = sizeof(o);
  o.device = -1;
  o.synchronous = 1;
  o.x_end = 2;
  if (m2s_voxelize(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &g, &vo, bits, occ, cells, 64, &n_set, &o) != M2S_ERR_BAD_ARG) ++failures;
  if (n_set != 99) ++failures; /* no failed argument check writes it */
  if (m2s_version() != 5) ++failures;
  if (argc > 1) {
    const uint64_t want = strtoull(argv[1], NULL, 0);
    uint64_t i, k, seen = 0;
    vo.mode = M2S_VOXELIZE_SURFACE;
    if (m2s_voxelize(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &g, &vo, bits, occ, cells, 64, &n_set, NULL) != M2S_OK) ++failures;
    if (n_set != want) ++failures;
    for (i = 0; i < 64; ++i) {
      const uint32_t bit = (bits[i / 4] >> (i % 4)) & 1u; /* nzw = 1: word (i, j), bit k */
      if (bit != occ[i] || occ[i] > 1) ++failures;
      if (occ[i]) {
        if (seen >= n_set || cells[seen] != i) ++failures;
        ++seen;
      }
    }
    if (seen != n_set) ++failures;
    for (k = 0; k < 16; ++k)
      if (bits[k] >> 4) ++failures; /* padding bits */
    n_set = 0;
    cells[0] = 12345;
    if (m2s_voxelize(v, 4, idx, 6, 4, M2S_TRIANGLE_LIST, &g, &vo, NULL, NULL, cells, want - 1, &n_set, NULL) != M2S_ERR_BAD_ARG) ++failures;
    if (n_set != want || cells[0] != 12345) ++failures;
  }
  printf(failures ? "FAIL (%d)\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
