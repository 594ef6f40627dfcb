/* Stand-alone driver for examl_host_rate_scan_plan
 * (examl_amd/csrc/model_prep.cpp), the slot planner of the per-site rate-scan
 * kernel (examl_amd/csrc/examl_dna_cat_rates.inc), meant to be built with
 * host sanitizers.  It makes no GPU call and links no HIP code.
 *
 * For caterpillar, balanced and random trees of 4 to 300 taxa (the random
 * ones from a fixed seed, children in either order) and for the one-entry
 * list it builds the post-order entry list rooted at tip 1, runs the planner
 * into exact-size heap arrays and replays the list over the slots, checking,
 * as the kernel relies on it: every inner operand is read from the slot that
 * still holds it (no slot is read before it is written, none after it was
 * overwritten), no result lands on a live slot, every slot is below L, and L
 * is the true maximum of results live at once.  Malformed lists (operand not
 * produced, operand consumed twice, ids out of range) must be refused.
 *
 * Build and run (host AddressSanitizer + UBSan):
 *   c++ -O1 -g -std=c++17 -fsanitize=address,undefined \
 *     -fno-sanitize-recover=undefined examl_amd/csrc/model_prep.cpp \
 *     tools/rate_scan_plan_check.cpp -o build/rate_scan_plan_check
 *   build/rate_scan_plan_check
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

enum Shape { CATERPILLAR, BALANCED, RANDOM };

/* post-order entries of the subtree over tips lo..hi (inclusive); returns
 * the subtree's node number */
static int emit(int lo, int hi, Shape sh, int mxtips, int *nextInner,
                std::vector<examl_hip_trav_entry> &out) {
  if (lo == hi) return lo;
  const int cnt = hi - lo + 1;
  int left = sh == CATERPILLAR ? 1
             : sh == BALANCED  ? cnt / 2
                               : 1 + (int)(rnd() % (uint64_t)(cnt - 1));
  const bool swap = sh == RANDOM && (rnd() & 1);
  int a, b;
  if (swap) {
    b = emit(lo + left, hi, sh, mxtips, nextInner, out);
    a = emit(lo, lo + left - 1, sh, mxtips, nextInner, out);
  } else {
    a = emit(lo, lo + left - 1, sh, mxtips, nextInner, out);
    b = emit(lo + left, hi, sh, mxtips, nextInner, out);
  }
  /* the reference puts a lone tip first (TIP_INNER: q is the tip) */
  if (a > mxtips && b <= mxtips) {
    const int t = a;
    a = b;
    b = t;
  }
  examl_hip_trav_entry e = {};
  e.tipCase = (a <= mxtips) + (b <= mxtips) == 2
                  ? EXAML_TIP_TIP
                  : (a <= mxtips ? EXAML_TIP_INNER : EXAML_INNER_INNER);
  e.pNumber = (*nextInner)++;
  e.qNumber = a;
  e.rNumber = b;
  e.qz = e.rz = 0.9;
  out.push_back(e);
  return e.pNumber;
}

static int check(const std::vector<examl_hip_trav_entry> &ops, int mxtips,
                 const char *what) {
  const int n = (int)ops.size();
  int *slot = new int[(size_t)n];
  int L = -1;
  int rc = examl_host_rate_scan_plan(ops.data(), n, mxtips, slot, &L);
  if (rc != 0 || L < 1 || L > n) {
    printf("%s (%d taxa): refused or bad L %d\n", what, mxtips, L);
    delete[] slot;
    return 1;
  }
  std::vector<int> holder((size_t)L, 0);       /* node a slot holds, 0 = dead */
  std::vector<int> slot_of((size_t)(2 * mxtips), -1);
  int live = 0, maxLive = 0, bad = 0;
  for (int k = 0; k < n && !bad; k++) {
    const examl_hip_trav_entry &e = ops[(size_t)k];
    const int in[2] = {e.tipCase == EXAML_INNER_INNER ? e.qNumber : 0,
                       e.tipCase != EXAML_TIP_TIP ? e.rNumber : 0};
    for (int o = 0; o < 2; o++) {
      if (!in[o]) continue;
      const int s = slot_of[(size_t)in[o]];
      if (s < 0 || s >= L || holder[(size_t)s] != in[o]) {
        printf("%s (%d taxa): entry %d reads node %d from a slot that does "
               "not hold it\n", what, mxtips, k, in[o]);
        bad = 1;
        break;
      }
      holder[(size_t)s] = 0;
      live--;
    }
    if (bad) break;
    const int d = slot[k];
    if (d < 0 || d >= L || holder[(size_t)d] != 0) {
      printf("%s (%d taxa): entry %d writes live or out-of-range slot %d\n",
             what, mxtips, k, d);
      bad = 1;
      break;
    }
    holder[(size_t)d] = e.pNumber;
    slot_of[(size_t)e.pNumber] = d;
    if (++live > maxLive) maxLive = live;
  }
  if (!bad && maxLive != L) {
    printf("%s (%d taxa): L = %d, most live at once %d\n", what, mxtips, L,
           maxLive);
    bad = 1;
  }
  delete[] slot;
  return bad;
}

int main() {
  int cases = 0, maxL = 0;
  const char *names[] = {"caterpillar", "balanced", "random"};
  for (int taxa = 4; taxa <= 300; taxa++)
    for (int sh = 0; sh < 3; sh++) {
      std::vector<examl_hip_trav_entry> ops;
      int nextInner = taxa + 1;
      /* rooted at tip 1: the other tips hang below the root's q */
      emit(2, taxa, (Shape)sh, taxa, &nextInner, ops);
      if ((int)ops.size() != taxa - 2) return 2;
      ops.shrink_to_fit();
      if (check(ops, taxa, names[sh])) return 1;
      if (sh == BALANCED) {
        int tmp[300], L = 0;
        examl_host_rate_scan_plan(ops.data(), taxa - 2, taxa, tmp, &L);
        if (L > maxL) maxL = L;
      }
      cases++;
    }
  { /* the one-entry list: three taxa, q = (2, 3) */
    std::vector<examl_hip_trav_entry> ops;
    int nextInner = 4;
    emit(2, 3, CATERPILLAR, 3, &nextInner, ops);
    if (check(ops, 3, "one entry")) return 1;
    cases++;
  }
  /* refused lists */
  {
    std::vector<examl_hip_trav_entry> ops;
    int nextInner = 7, s[8], L = 0;
    emit(2, 6, BALANCED, 6, &nextInner, ops);
    std::vector<examl_hip_trav_entry> twice = ops, early = ops, range = ops;
    twice.push_back(ops.back());         /* operands consumed already */
    early.erase(early.begin());          /* an operand nobody produced */
    range[0].qNumber = 7;                /* a tip id out of range */
    if (examl_host_rate_scan_plan(twice.data(), (int)twice.size(), 6, s, &L) != -1 ||
        examl_host_rate_scan_plan(early.data(), (int)early.size(), 6, s, &L) != -1 ||
        examl_host_rate_scan_plan(range.data(), (int)range.size(), 6, s, &L) != -1 ||
        examl_host_rate_scan_plan(ops.data(), 0, 6, s, &L) != -1) {
      printf("a malformed list was accepted\n");
      return 1;
    }
  }
  printf("ok: %d lists, largest L %d (balanced, 300 taxa and below)\n", cases,
         maxL);
  return 0;
}
