/* Stand-alone driver for the tile-table builder of the on-chip
 * multi-partition traversal (examl_hip_multi_tile_table,
 * examl_amd/csrc/examl_hip.hip), meant to be built with host sanitizers.
 * It makes no GPU call.
 *
 * It generates a few hundred width lists from a fixed seed (zeros, ones,
 * tile - 1 / tile / tile + 1, random widths, and lists whose tile count sits
 * just past the grid cap), runs the builder into exact-size heap arrays and
 * compares every entry with a straightforward recomputation; it also checks
 * that a capacity one short is refused before anything is written.
 *
 * Build and run (host AddressSanitizer + UBSan):
 *   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off \
 *     -Xarch_host -fsanitize=address,undefined \
 *     -Xarch_host -fno-sanitize-recover=undefined \
 *     examl_amd/csrc/examl_hip.hip examl_amd/csrc/model_prep.cpp \
 *     tools/multi_tiles_check.cpp -o build/multi_tiles_check
 *   build/multi_tiles_check
 */
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/examl_hip.h"

static uint64_t g_state = 0x243f6a8885a308d3ULL;

static uint64_t rnd() { /* xorshift64* */
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return g_state * 0x2545f4914f6cdd1dULL;
}

static int check(const std::vector<long> &w, int tile, int caseNo) {
  const int np = (int)w.size();
  /* the straightforward recomputation */
  std::vector<int> wantPart;
  std::vector<long> wantSite;
  for (int p = 0; p < np; p++)
    for (long s = 0; s < w[(size_t)p]; s += tile) {
      wantPart.push_back(p);
      wantSite.push_back(s);
    }
  const int want = (int)wantPart.size();

  /* exact-size heap arrays: an overrun is an ASan report */
  std::vector<int> part((size_t)want);
  std::vector<long> site((size_t)want);
  const int got = examl_hip_multi_tile_table(w.data(), np, tile, part.data(),
                                             site.data(), want);
  if (got != want) {
    printf("case %d: %d tiles, expected %d\n", caseNo, got, want);
    return 1;
  }
  for (int t = 0; t < want; t++)
    if (part[(size_t)t] != wantPart[(size_t)t] ||
        site[(size_t)t] != wantSite[(size_t)t]) {
      printf("case %d: tile %d is (%d, %ld), expected (%d, %ld)\n", caseNo, t,
             part[(size_t)t], site[(size_t)t], wantPart[(size_t)t],
             wantSite[(size_t)t]);
      return 1;
    }
  if (want > 0) {
    /* one short: refused, and nothing may be written (the arrays are one
     * short too) */
    std::vector<int> part1((size_t)want - 1);
    std::vector<long> site1((size_t)want - 1);
    if (examl_hip_multi_tile_table(w.data(), np, tile, part1.data(),
                                   site1.data(), want - 1) != -1) {
      printf("case %d: a capacity one short was accepted\n", caseNo);
      return 1;
    }
  }
  return 0;
}

int main() {
  const int tile = examl_hip_fused_tile_sites();
  const int cap = examl_hip_fused_grid_cap();
  std::vector<std::vector<long>> cases = {
      {}, {0}, {1}, {0, 0, 5}, {(long)tile, (long)tile},
      {(long)tile - 1, (long)tile + 1, 0, 1},
      {(long)tile - 1}, {(long)tile}, {(long)tile + 1},
      /* a tile count just past the grid cap, in one and in three parts */
      {(long)(cap + 9) * tile},
      {(long)cap * tile - 5, 1, (long)8 * tile},
      {(long)(cap / 2) * tile + 1, 0, (long)(cap / 2) * tile, 1},
  };
  const long edge[] = {0, 1, (long)tile - 1, tile, (long)tile + 1,
                       2L * tile - 1, 2L * tile, 2L * tile + 1};
  for (int c = 0; c < 300; c++) {
    const int np = 1 + (int)(rnd() % 24);
    std::vector<long> w((size_t)np);
    for (auto &x : w) {
      const uint64_t k = rnd() % 4;
      if (k == 0)
        x = edge[rnd() % 8];
      else if (k == 1)
        x = (long)(rnd() % 4);
      else
        x = (long)(rnd() % 20000);
    }
    cases.push_back(w);
  }
  long tiles = 0;
  int caseNo = 0;
  for (const auto &w : cases) {
    if (check(w, tile, caseNo)) return 1;
    for (long x : w) tiles += (x + tile - 1) / tile;
    caseNo++;
  }
  /* malformed arguments */
  const long neg[] = {5, -1};
  int dummyP[4];
  long dummyS[4];
  if (examl_hip_multi_tile_table(neg, 2, tile, dummyP, dummyS, 4) != -1 ||
      examl_hip_multi_tile_table(neg, 1, 0, dummyP, dummyS, 4) != -1) {
    printf("malformed arguments were accepted\n");
    return 1;
  }
  printf("ok: %d width lists, %ld tiles, tile %d sites, grid cap %d\n",
         caseNo, tiles, tile, cap);
  return 0;
}
