/* Stand-alone driver for the fused-traversal launch planner
 * (examl_hip_fused_plan, examl_amd/csrc/examl_hip.hip), meant to be built
 * with host sanitizers.  It makes no GPU call.
 *
 * Input (stdin), as written by tools/fused_plan_cases.py:
 *   <numCases>
 *   per case:  <numOps> <maxDepth>
 *              numOps lines "tipCase p q r x1 x2 x3"
 * For every case it runs the planner and re-checks the launch partition and
 * the source ranges; it prints one summary line per case.
 *
 * Build and run (host AddressSanitizer + UBSan):
 *   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off \
 *     -Xarch_host -fsanitize=address,undefined \
 *     -Xarch_host -fno-sanitize-recover=undefined \
 *     examl_amd/csrc/examl_hip.hip examl_amd/csrc/model_prep.cpp \
 *     tools/fused_plan_check.cpp -o build/fused_plan_check
 *   python tools/fused_plan_cases.py | build/fused_plan_check
 */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/examl_hip.h"

int main() {
  int ncases = 0;
  if (scanf("%d", &ncases) != 1) return 2;
  long total_ops = 0, total_launches = 0;
  for (int c = 0; c < ncases; c++) {
    int n = 0, depth = 0;
    if (scanf("%d %d", &n, &depth) != 2) return 2;
    std::vector<examl_hip_trav_entry> ops((size_t)n);
    for (auto &o : ops) {
      if (scanf("%d %d %d %d %d %d %d", &o.tipCase, &o.pNumber, &o.qNumber,
                &o.rNumber, &o.x1Slot, &o.x2Slot, &o.x3Slot) != 7)
        return 2;
      o.qz = o.rz = 0.5;
    }
    /* exact-size heap arrays: an overrun is an ASan report */
    std::vector<int> launch((size_t)n), s1((size_t)n), s2((size_t)n);
    const int nl = examl_hip_fused_plan(ops.data(), n, depth, launch.data(),
                                        s1.data(), s2.data());
    if (nl < 0) {
      printf("case %d: rejected (%d)\n", c, nl);
      continue;
    }
    for (int e = 0; e < n; e++) {
      const int prev = e ? launch[(size_t)e - 1] : 0;
      if (launch[(size_t)e] < prev || launch[(size_t)e] > prev + 1 ||
          launch[(size_t)e] >= nl || s1[(size_t)e] < -1 ||
          s1[(size_t)e] >= depth || s2[(size_t)e] < -1 ||
          s2[(size_t)e] >= depth) {
        printf("case %d: bad plan at op %d\n", c, e);
        return 1;
      }
    }
    total_ops += n;
    total_launches += nl;
    printf("case %d: %d ops, depth %d -> %d launch(es)\n", c, n, depth, nl);
  }
  printf("ok: %d cases, %ld ops, %ld launches\n", ncases, total_ops,
         total_launches);
  return 0;
}
