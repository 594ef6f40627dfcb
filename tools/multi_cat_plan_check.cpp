/* Stand-alone driver for the host-side geometry of the on-chip
 * multi-partition DNA PSR traversal: examl_hip_multi_cat_plan (category
 * offsets and P row length) together with examl_hip_multi_tile_table at the
 * CAT tile size (examl_amd/csrc/examl_dna_cat_mseg.inc, examl_hip.hip),
 * meant to be built with host sanitizers.  It makes no GPU call.
 *
 * From a fixed seed it generates a few hundred (widths, numCats) lists with
 * empty partitions, one-site partitions and widths around the tile, runs
 * both builders into exact-size heap arrays and checks, as the executor and
 * the kernel rely on it: the P blocks of the partitions that have sites are
 * disjoint, in partition order and fill the row exactly; every tile's block
 * lies inside a row of a buffer sized maxOps * numParts * 25 * 32 doubles;
 * an empty partition owns no tile and no categories; numCats outside 1..25
 * on a partition with sites is refused.
 *
 * Build and run (host AddressSanitizer + UBSan):
 *   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off \
 *     -Xarch_host -fsanitize=address,undefined \
 *     -Xarch_host -fno-sanitize-recover=undefined \
 *     examl_amd/csrc/examl_hip.hip examl_amd/csrc/model_prep.cpp \
 *     tools/multi_cat_plan_check.cpp -o build/multi_cat_plan_check
 *   build/multi_cat_plan_check
 */
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/examl_hip.h"

static const int MAXC = 25;
static uint64_t g_state = 0x13198a2e03707344ULL;

static uint64_t rnd() { /* xorshift64* */
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return g_state * 0x2545f4914f6cdd1dULL;
}

static int check(const std::vector<long> &w, const std::vector<int> &nc,
                 int tile, int caseNo) {
  const int np = (int)w.size();
  std::vector<int> catOff((size_t)np);
  long pRow = -1;
  if (examl_hip_multi_cat_plan(np, w.data(), nc.data(), MAXC, catOff.data(),
                               &pRow) != 0) {
    printf("case %d: a valid list was refused\n", caseNo);
    return 1;
  }
  long next = 0, tiles = 0;
  for (int p = 0; p < np; p++) {
    if (catOff[(size_t)p] != next) {
      printf("case %d: catOff[%d] = %d, expected %ld\n", caseNo, p,
             catOff[(size_t)p], next);
      return 1;
    }
    if (w[(size_t)p] > 0) next += nc[(size_t)p];
    tiles += (w[(size_t)p] + tile - 1) / tile;
  }
  if (pRow != 32 * next || pRow > 32L * MAXC * np) {
    printf("case %d: pRow %ld, categories %ld\n", caseNo, pRow, next);
    return 1;
  }
  std::vector<int> part((size_t)tiles);
  std::vector<long> site((size_t)tiles);
  if (examl_hip_multi_tile_table(w.data(), np, tile, part.data(), site.data(),
                                 (int)tiles) != (int)tiles) {
    printf("case %d: tile table\n", caseNo);
    return 1;
  }
  for (long t = 0; t < tiles; t++) {
    const int p = part[(size_t)t];
    /* the block the kernel stages for this tile, and the sites it owns */
    const long lo = 32L * catOff[(size_t)p];
    const long hi = lo + 32L * nc[(size_t)p];
    if (p < 0 || p >= np || w[(size_t)p] == 0 || lo < 0 || hi > pRow ||
        site[(size_t)t] < 0 || site[(size_t)t] >= w[(size_t)p] ||
        site[(size_t)t] % tile != 0) {
      printf("case %d: tile %ld (partition %d, site %ld)\n", caseNo, t, p,
             site[(size_t)t]);
      return 1;
    }
  }
  return 0;
}

int main() {
  const int tile = examl_hip_cat_fused_tile_sites();
  const long edge[] = {0, 1, (long)tile - 1, tile, (long)tile + 1,
                       2L * tile + 5, 3, 65};
  const int cats[] = {1, 7, 25};
  std::vector<std::vector<long>> ws = {
      {1}, {(long)tile - 1, (long)tile + 1, 0, 1}, {3, 65, 2L * tile + 5},
      {0}, {0, 0, 0}, {}};
  for (int c = 0; c < 400; c++) {
    const int np = 1 + (int)(rnd() % 24);
    std::vector<long> w((size_t)np);
    for (auto &x : w) {
      const uint64_t k = rnd() % 4;
      x = k == 0 ? edge[rnd() % 8]
                 : (k == 1 ? (long)(rnd() % 3) : (long)(rnd() % 20000));
    }
    ws.push_back(w);
  }
  int caseNo = 0;
  long parts = 0;
  for (const auto &w : ws) {
    std::vector<int> nc(w.size());
    for (size_t p = 0; p < w.size(); p++)
      /* an empty partition's count is not looked at: give it a bad one */
      nc[p] = w[p] == 0 ? (int)(rnd() % 3) * 40 - 40
                        : (rnd() % 2 ? cats[rnd() % 3] : 1 + (int)(rnd() % MAXC));
    if (check(w, nc, tile, caseNo)) return 1;
    parts += (long)w.size();
    caseNo++;
  }
  /* refused: a category count outside 1..25 where there are sites, a
   * negative width */
  const long w2[] = {5, 9};
  const long wneg[] = {5, -1};
  const int bad0[] = {3, 0}, bad26[] = {26, 3}, ok[] = {3, 3};
  int off[2];
  long row = 0;
  if (examl_hip_multi_cat_plan(2, w2, bad0, MAXC, off, &row) != -1 ||
      examl_hip_multi_cat_plan(2, w2, bad26, MAXC, off, &row) != -1 ||
      examl_hip_multi_cat_plan(2, wneg, ok, MAXC, off, &row) != -1 ||
      examl_hip_multi_cat_plan(2, w2, ok, MAXC, off, &row) != 0 ||
      row != 192) {
    printf("malformed arguments were accepted\n");
    return 1;
  }
  printf("ok: %d lists, %ld partitions, tile %d sites\n", caseNo, parts, tile);
  return 0;
}
