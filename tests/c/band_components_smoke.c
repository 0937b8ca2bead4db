/* m2s_band_components and m2s_band_select from plain C (C99, -Wall -Werror): the declarations compile and link, and every answer that is
 * decided without a handle comes out as include/m2s.h states it.  With an argument (anything) it also labels and selects on the GPU, on an
 * 8 x 8 x 8 grid: a slab of 128 cells (i = 0 with the value -1, i = 1 with +1) and one island cell at (7, 7, 7) with the value -0.5 whose
 * row holds seven inactive points with their inside bit set.  Two components; keeping the slab drops the island and clears the seven bits.
 * Prints "all checks passed". */
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
  static uint64_t cells[512];
  static float d[512];
  static uint32_t bits[64], labels[512];
  static const uint8_t keep[2] = {1, 0};
  m2s_band_component comps[4];
  m2s_band_components_opts co;
  m2s_band_select_info info;
  m2s_band_field_opts fo;
  m2s_band *a = NULL, *r = (m2s_band*)&g; /* any non-NULL value: a failed call must reset it */
  uint64_t n = 77;
  int x;
  (void)argv;
  for (x = 0; x < 3; ++x) { g.first_cell[x] = 0.25f; g.cell_size[x] = 0.5f; g.cell_count[x] = 8; }
  co.struct_size = sizeof(co);
  co.connectivity = M2S_CONNECT_6;
  check(sizeof(m2s_band_component) == 48 && sizeof(co) == 8 && sizeof(info) == 32, "the structs' sizes");
  check(M2S_CONNECT_6 == 6 && M2S_CONNECT_18 == 18 && M2S_CONNECT_26 == 26 && M2S_LABEL_NONE == 0xffffffffu, "the constants");
  check(m2s_band_components(NULL, &co, NULL, NULL, NULL, 0, &n) == M2S_ERR_BAD_ARG, "components: NULL handle");
  check(m2s_band_components((const m2s_band*)&g, &co, NULL, NULL, NULL, 0, NULL) == M2S_ERR_BAD_ARG, "components: NULL count");
  co.connectivity = 8;
  check(m2s_band_components((const m2s_band*)&g, &co, NULL, NULL, NULL, 0, &n) == M2S_ERR_BAD_ARG, "components: connectivity 8");
  co.connectivity = M2S_CONNECT_26;
  co.struct_size = 4;
  check(m2s_band_components((const m2s_band*)&g, &co, NULL, NULL, NULL, 0, &n) == M2S_ERR_BAD_ARG, "components: struct_size");
  co.struct_size = sizeof(co);
  check(m2s_band_select(NULL, labels, keep, 2, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "select: NULL handle");
  r = (m2s_band*)&g;
  check(m2s_band_select((const m2s_band*)&g, NULL, keep, 2, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "select: NULL labels");
  r = (m2s_band*)&g;
  check(m2s_band_select((const m2s_band*)&g, labels, NULL, 2, NULL, NULL, &r, NULL) == M2S_ERR_BAD_ARG && r == NULL, "select: NULL keep");
  check(m2s_band_select((const m2s_band*)&g, labels, keep, 2, NULL, NULL, NULL, NULL) == M2S_ERR_BAD_ARG, "select: NULL out");
  check(m2s_version() == 5, "version");
  if (argc > 1) {
    uint64_t k = 0, bytes = 0;
    int bad = 0;
    for (x = 0; x < 128; ++x) { cells[x] = (uint64_t)x; d[x] = x < 64 ? -1.0f : 1.0f; }
    cells[128] = 511;
    d[128] = -0.5f;
    memset(bits, 0, sizeof(bits));
    bits[63] = 0x7fu; /* row (7, 7): k = 0 .. 6 inside, beyond the band */
    fo.struct_size = sizeof(fo);
    fo.background_outside = 0.75f;
    fo.background_inside = 0.5f;
    check(m2s_band_create(&g, cells, d, 129, bits, &fo, NULL, &a) == M2S_OK && a != NULL, "create");
    for (x = 6; x <= 26; x += (x == 6 ? 12 : 8)) {
      co.connectivity = x;
      n = 77;
      check(m2s_band_components(a, &co, NULL, NULL, NULL, 0, &n) == M2S_OK && n == 2, "count only");
      memset(comps, 0xee, sizeof(comps));
      n = 77;
      check(m2s_band_components(a, &co, NULL, labels, comps, 1, &n) == M2S_ERR_BAD_ARG && n == 2 && comps[0].n_cells == 0xeeeeeeeeeeeeeeeeull,
            "a capacity below the count");
      check(m2s_band_components(a, &co, NULL, labels, comps, 4, &n) == M2S_OK && n == 2, "components");
      for (k = 0; k < 128; ++k) bad += labels[k] != 0;
      check(bad == 0 && labels[128] == 1, "labels");
      check(comps[0].first_cell == 0 && comps[0].n_cells == 128 && comps[0].n_negative == 64 && comps[0].lo[0] == 0 && comps[0].lo[1] == 0 &&
            comps[0].lo[2] == 0 && comps[0].hi[0] == 1 && comps[0].hi[1] == 7 && comps[0].hi[2] == 7, "the slab's statistics");
      check(comps[1].first_cell == 511 && comps[1].n_cells == 1 && comps[1].n_negative == 1 && comps[1].lo[0] == 7 && comps[1].lo[1] == 7 &&
            comps[1].lo[2] == 7 && comps[1].hi[0] == 7 && comps[1].hi[1] == 7 && comps[1].hi[2] == 7, "the island's statistics");
    }
    memset(&info, 0, sizeof(info));
    info.struct_size = 8;
    r = (m2s_band*)&g;
    check(m2s_band_select(a, labels, keep, 2, NULL, NULL, &r, &info) == M2S_ERR_BAD_ARG && r == NULL, "select: the info's struct_size");
    info.struct_size = sizeof(info);
    check(m2s_band_select(a, labels, keep, 2, NULL, NULL, &r, &info) == M2S_OK && r != NULL, "select");
    if (r) {
      check(info.n_cells == 128 && info.n_dropped == 1 && info.n_sign_cleared == 7, "select: info");
      check(m2s_band_info(r, NULL, &k, &bytes) == M2S_OK && k == 128 && bytes == 24 * 8 + 4 * k, "select: band_info");
      check(m2s_band_export(r, cells, d, 512, bits, NULL) == M2S_OK, "select: export");
      bad = 0;
      for (x = 0; x < 128; ++x) bad += cells[x] != (uint64_t)x || d[x] != (x < 64 ? -1.0f : 1.0f);
      for (x = 0; x < 64; ++x) bad += bits[x] != (x < 8 ? 0xffu : 0u);
      check(bad == 0, "select: every cell, value and sign bit");
      m2s_band_destroy(r);
    }
    /* keep everything: the identity, and the seven bits stay */
    {
      static const uint8_t all[2] = {1, 1};
      check(m2s_band_select(a, labels, all, 2, NULL, NULL, &r, &info) == M2S_OK && r != NULL, "select all");
      if (r) {
        check(info.n_cells == 129 && info.n_dropped == 0 && info.n_sign_cleared == 0, "select all: info");
        check(m2s_band_export(r, cells, d, 512, bits, NULL) == M2S_OK && bits[63] == 0xffu && cells[128] == 511 && d[128] == -0.5f, "select all: export");
        m2s_band_destroy(r);
      }
    }
    m2s_band_destroy(a);
  }
  if (failures == 0) printf("all checks passed\n");
  return failures ? 1 : 0;
}
