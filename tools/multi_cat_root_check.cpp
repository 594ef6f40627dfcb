/* Stand-alone driver for the unit-table builder of the all-partition DNA PSR
 * root operations (examl_hip_multi_cat_root_units,
 * examl_amd/csrc/examl_dna_cat_mseg.inc), meant to be built with host
 * sanitizers.  It makes no GPU call.
 *
 * Width lists: zeros, ones, 255 / 256 / 257, widths just past
 * grid cap x 256 (where a partition's blocks start to wrap) and a few
 * hundred seeded random lists.  The builder writes into exact-size heap
 * arrays and every entry is compared with a straightforward recomputation;
 * a capacity one short must be refused before anything is written.
 *
 * Build and run (host AddressSanitizer + UBSan):
 *   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off \
 *     -Xarch_host -fsanitize=address,undefined \
 *     -Xarch_host -fno-sanitize-recover=undefined \
 *     examl_amd/csrc/examl_hip.hip examl_amd/csrc/model_prep.cpp \
 *     tools/multi_cat_root_check.cpp -o build/multi_cat_root_check
 *   build/multi_cat_root_check
 */
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/examl_hip.h"

static uint64_t g_state = 0x13198a2e03707344ULL;

static uint64_t rnd() { /* xorshift64* */
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return g_state * 0x2545f4914f6cdd1dULL;
}

static int check(const std::vector<long> &w, int cap, int caseNo) {
  const int np = (int)w.size();
  std::vector<int> wantPrefix, wantPart;
  for (int p = 0; p < np; p++) {
    wantPrefix.push_back((int)wantPart.size());
    long g = (w[(size_t)p] + 255) / 256;
    if (g > cap) g = cap;
    for (long b = 0; b < g; b++) wantPart.push_back(p);
  }
  wantPrefix.push_back((int)wantPart.size());
  const long want = (long)wantPart.size();

  /* count only, then exact-size heap arrays: an overrun is an ASan report */
  std::vector<int> prefix0((size_t)np + 1, -7);
  if (examl_hip_multi_cat_root_units(np, w.data(), prefix0.data(), nullptr,
                                     -1) != want ||
      prefix0 != wantPrefix) {
    printf("case %d: count-only call disagrees\n", caseNo);
    return 1;
  }
  std::vector<int> prefix((size_t)np + 1, -7), part((size_t)want, -7);
  if (examl_hip_multi_cat_root_units(np, w.data(), prefix.data(), part.data(),
                                     want) != want ||
      prefix != wantPrefix || part != wantPart) {
    printf("case %d: unit tables disagree (%ld units)\n", caseNo, want);
    return 1;
  }
  if (want > 0) {
    /* one short: refused, nothing written */
    std::vector<int> prefix1((size_t)np + 1, -7), part1((size_t)want - 1, -7);
    if (examl_hip_multi_cat_root_units(np, w.data(), prefix1.data(),
                                       part1.data(), want - 1) != -1) {
      printf("case %d: a capacity one short was accepted\n", caseNo);
      return 1;
    }
    for (int x : prefix1)
      if (x != -7) {
        printf("case %d: a refused call wrote the prefix\n", caseNo);
        return 1;
      }
    for (int x : part1)
      if (x != -7) {
        printf("case %d: a refused call wrote the unit table\n", caseNo);
        return 1;
      }
  }
  return 0;
}

int main() {
  const int cap = examl_hip_multi_cat_root_grid_cap();
  const long wrap = (long)cap * 256;
  std::vector<std::vector<long>> cases = {
      {}, {0}, {1}, {0, 0, 0}, {1, 1, 1}, {255}, {256}, {257},
      {255, 257, 0, 1, 700}, {256, 256}, {0, 5, 0},
      {wrap}, {wrap + 1}, {wrap + 300, 1}, {1, wrap - 1, 0, wrap + 257},
      {3 * wrap + 5, wrap + 1},
  };
  const long edge[] = {0, 1, 255, 256, 257, 511, 512, 513};
  for (int c = 0; c < 300; c++) {
    const int np = 1 + (int)(rnd() % 24);
    std::vector<long> w((size_t)np);
    for (auto &x : w) {
      const uint64_t k = rnd() % 8;
      if (k < 3)
        x = edge[rnd() % 8];
      else if (k == 3)
        x = wrap - 2 + (long)(rnd() % 600);
      else
        x = (long)(rnd() % 20000);
    }
    cases.push_back(w);
  }
  long units = 0;
  int caseNo = 0;
  for (const auto &w : cases) {
    if (check(w, cap, caseNo)) return 1;
    for (long x : w) {
      const long g = (x + 255) / 256;
      units += g < cap ? g : cap;
    }
    caseNo++;
  }
  /* malformed arguments */
  const long neg[] = {5, -1};
  int pre[3] = {-7, -7, -7}, part[4];
  if (examl_hip_multi_cat_root_units(2, neg, pre, part, 4) != -1 ||
      examl_hip_multi_cat_root_units(-1, neg, pre, part, 4) != -1 ||
      pre[0] != -7) {
    printf("malformed arguments were accepted\n");
    return 1;
  }
  printf("ok: %d width lists, %ld units, grid cap %d\n", caseNo, units, cap);
  return 0;
}
