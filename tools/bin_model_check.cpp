/* Stand-alone driver for the binary (two-state) host model math
 * (examl_host_init_gtr_bin and examl_host_core_dtables_bin in
 * examl_amd/csrc/model_prep.cpp, examl_host_make_p and
 * examl_host_calc_diagptable at states = 2), meant to be built with host
 * sanitizers.  It makes no GPU call.
 *
 * It draws a few hundred frequency / alpha / branch-length sets from a fixed
 * seed, frequencies at the FREQ_MIN bound (0.001, examl/axml.h) included,
 * runs every function into exact-size heap arrays, so that a write past the
 * documented sizes (EIGN[2], EV[4], EI[4], tipVector[8], left/right[16],
 * diag[8], dtables[24]) is an error under AddressSanitizer, and checks the
 * structure of what comes back.
 *
 * Build and run (host AddressSanitizer + UBSan):
 *   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off \
 *     -Xarch_host -fsanitize=address,undefined \
 *     -Xarch_host -fno-sanitize-recover=undefined \
 *     examl_amd/csrc/examl_hip.hip examl_amd/csrc/model_prep.cpp \
 *     tools/bin_model_check.cpp -o build/bin_model_check
 *   build/bin_model_check
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/examl_hip.h"

static uint64_t g_state = 0x9e3779b97f4a7c15ULL;

static double rnd01() { /* xorshift64*, 53 bits */
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (double)((g_state * 0x2545f4914f6cdd1dULL) >> 11) / 9007199254740992.0;
}

static int fail(int caseNo, const char *what, double v) {
  fprintf(stderr, "case %d: %s (%.17g)\n", caseNo, what, v);
  return 1;
}

static int check(int caseNo, double f0, double alpha, double z1, double z2,
                 double lz) {
  /* exact-size heap arrays */
  std::vector<double> freqs{f0, 1.0 - f0}, rates1{1.0};
  std::vector<double> EIGN(2), EV(4), EI(4), tv(8), g(4), left(16), right(16),
      diag(8), dtab(24);
  examl_host_init_gtr_bin(freqs.data(), rates1.data(), EIGN.data(), EV.data(),
                          EI.data(), tv.data());
  examl_host_make_gamma_cats(alpha, g.data(), 4);
  if (EIGN[0] != 0.0) return fail(caseNo, "EIGN[0] != 0", EIGN[0]);
  if (!(EIGN[1] > 0.0) || !std::isfinite(EIGN[1]))
    return fail(caseNo, "EIGN[1] not positive", EIGN[1]);
  for (int i = 0; i < 4; i++)
    if (!std::isfinite(EV[i]) || !std::isfinite(EI[i]))
      return fail(caseNo, "EV/EI not finite", EV[i]);
  if (EI[0] != 1.0 || EI[2] != 1.0) return fail(caseNo, "EI column 0", EI[0]);
  /* code 0 empty, codes 1/2 the rows of EV, code 3 their capped sum */
  if (tv[0] != 0.0 || tv[1] != 0.0) return fail(caseNo, "tip code 0", tv[0]);
  for (int j = 0; j < 2; j++) {
    if (tv[2 + j] != std::fmin(EV[j], 0.999999999) ||
        tv[4 + j] != std::fmin(EV[2 + j], 0.999999999))
      return fail(caseNo, "tip codes 1/2", tv[2 + j]);
    if (tv[6 + j] != std::fmin(EV[j] + EV[2 + j], 0.999999999))
      return fail(caseNo, "tip code 3", tv[6 + j]);
  }

  const double l1 = std::log(z1 > 1e-15 ? z1 : 1e-15);
  const double l2 = std::log(z2 > 1e-15 ? z2 : 1e-15);
  examl_host_make_p(l1, l2, g.data(), EI.data(), EIGN.data(), 4, left.data(),
                    right.data(), 2);
  for (int c = 0; c < 4; c++)
    for (int r = 0; r < 2; r++) {
      if (left[c * 4 + r * 2] != 1.0 || right[c * 4 + r * 2] != 1.0)
        return fail(caseNo, "P column 0", left[c * 4 + r * 2]);
      if (left[c * 4 + r * 2 + 1] !=
          std::exp(g[c] * (EIGN[1] * l1)) * EI[r * 2 + 1])
        return fail(caseNo, "P column 1", left[c * 4 + r * 2 + 1]);
    }

  examl_host_calc_diagptable(z1, 2, 4, g.data(), EIGN.data(), diag.data());
  examl_host_core_dtables_bin(EIGN.data(), g.data(), lz, dtab.data());
  for (int c = 0; c < 4; c++) {
    /* exp underflows to exactly 0 on long branches in fast categories */
    if (diag[c * 2] != 1.0 || !(diag[c * 2 + 1] >= 0.0) ||
        !(diag[c * 2 + 1] <= 1.0))
      return fail(caseNo, "diag", diag[c * 2 + 1]);
    if (dtab[c * 2] != 1.0 || dtab[8 + c * 2] != 0.0 ||
        dtab[16 + c * 2] != 0.0)
      return fail(caseNo, "dtable state 0", dtab[c * 2]);
    if (dtab[c * 2 + 1] != std::exp(EIGN[1] * g[c] * lz) ||
        dtab[8 + c * 2 + 1] != EIGN[1] * g[c] ||
        dtab[16 + c * 2 + 1] != EIGN[1] * EIGN[1] * (g[c] * g[c]))
      return fail(caseNo, "dtable state 1", dtab[c * 2 + 1]);
  }
  return 0;
}

int main() {
  const double FREQ_MIN = 0.001;
  int bad = 0, cases = 0;
  /* the bounds first: both frequencies at FREQ_MIN, alpha and z at theirs */
  const double f_edge[] = {FREQ_MIN, 1.0 - FREQ_MIN, 0.5};
  const double a_edge[] = {0.02, 1.0, 1000.0};      /* ALPHA_MIN..ALPHA_MAX */
  const double z_edge[] = {1e-20, 1e-15, 0.9, 1.0 - 1e-6};
  for (double f : f_edge)
    for (double a : a_edge)
      for (double z : z_edge) {
        const double z2 = z_edge[cases % 4];
        bad += check(cases, f, a, z, z2, std::log(z > 1e-15 ? z : 1e-15));
        cases++;
      }
  for (int i = 0; i < 400; i++) {
    const double f = FREQ_MIN + (1.0 - 2.0 * FREQ_MIN) * rnd01();
    const double a =
        std::exp(std::log(0.02) + rnd01() * std::log(1000.0 / 0.02));
    const double z1 = std::exp(-30.0 * rnd01());
    const double z2 = std::exp(-30.0 * rnd01());
    bad += check(cases, f, a, z1, z2, std::log(z1 > 1e-15 ? z1 : 1e-15));
    cases++;
  }
  printf("bin_model_check: %d cases, %d failed\n", cases, bad);
  return bad ? 1 : 0;
}
