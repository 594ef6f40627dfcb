/* ============================================================================
 * examl_prot_cat_rates.inc — the -m PSR per-site rate search for protein
 * (20-state) partitions on the GPU.
 *
 * k_rate_scan_prot_cat replaces the per-site loop of optRateCatPthreads
 * (examl/optimizeModel.c:1798) together with the evaluatePartialGeneric it
 * calls for every candidate rate (examl/evaluatePartialGenericSpecial.c:259,
 * computeVectorGTRCATPROT :493, evaluatePartialGTRCATPROT :618).  The scan is
 * k_rate_scan_dna_cat's, statement for statement; the mapping is not: one
 * lane per site would hold about 100 live doubles at span 20.
 *
 * Four lanes per site.  Lane j = lane & 3 of an aligned quad owns states
 * 5j..5j+4 of its site; a wave holds 16 sites, a block of 256 threads 64.
 * The four lanes of a quad carry identical scan state and compute identical
 * lnL bits, so they enter, continue and leave every loop together; quads of
 * one wave may diverge from each other.  All cross-lane traffic is DPP
 * quad_perm inside a quad, whose lanes are always active together; nothing
 * reads a lane outside its quad and there is no wave-wide vote, so quads past
 * the last site simply do nothing.
 *
 * Per entry a lane computes the exp(EIGN[l]*lz) of its own five states per
 * child (the host's 38 exps spread over the quad), then two quad all-gathers
 * keep the host's summation order (examl_host_evaluate_partial_prot_cat,
 * operation for operation apart from the device's exp and log):
 *   gather d1, d2 (20 each) -> u1/u2 of the lane's own five rows l, even/odd
 *   sums as the host's -> gather the 20 x1px2 -> the lane's own five x3[k],
 *   from 0.0 over l = 0..19 in order.
 *
 * Included by examl_hip.hip (same flags, -ffp-contract=off).
 *
 * Data movement
 *  - EIGN, EI, EV and the 23x20 tipVector: LDS, once per block, one barrier
 *    before the site loop and none after it.  A quad reads EI by row block
 *    (lane pitch 100 doubles) and EV/tipVector by column block (lane pitch 5
 *    doubles): four distinct addresses per instruction, 8-byte reads at
 *    dword offsets 0/200/400/600 resp. 0/10/20/30, which fall into disjoint
 *    banks, each broadcast to the 16 quads.  No padding.
 *  - the entry table (RsOp, shared with the DNA kernel): wave-uniform loads.
 *  - tip codes: one byte per site and tip, the quad's lanes read the same.
 *  - the private CLV stack: L slots of 20 doubles per RESIDENT site laid out
 *    [slot][site][state]; a lane touches only its own 40 bytes, a wave moves
 *    2560 B contiguous.  LDS_SLOTS picks their home: dynamic LDS
 *    (L * 160 B * 64 sites per block) or global scratch sized
 *    gridDim * 64 sites, never n.
 * ==========================================================================*/

#define RP_BLOCK 256
#define RP_SITES (RP_BLOCK / 4) /* per block */
#define RP_MAX_GRID 1024        /* resident sites = 65,536 */
#define RP_EI 20                /* EIGN 20 | EI 400 | EV 400 | tipVector 460 */
#define RP_EV 420
#define RP_TV 820
#define RP_CONST_DOUBLES 1280
#define RP_SLOT_BYTES (20 * 8 * RP_SITES) /* one slot of one block */
/* default: LDS slots while L <= 4 (10 KiB constants + 40 KiB slots keep three
 * blocks on a CU's 160 KiB, the three waves per SIMD the registers allow) */
#define RP_LDS_BUDGET (4 * RP_SLOT_BYTES)
/* static + dynamic LDS of one block stay within 64 KiB whatever the budget */
#define RP_LDS_MAX (64 * 1024 - RP_CONST_DOUBLES * 8)

struct RpArgs {
  const double *consts; /* RP_CONST_DOUBLES */
  const RsOp *ops;
  int numOps, rootTip, rootSlot, max_k;
  double rootLz, logMinlik, lower, upper;
  const unsigned char *tips;
  long tipStride, n;
  const int *wgt;
  double *patrat, *lhs;
  double *scratch;
};

/* the value lane S of the caller's quad holds (quad_perm [S,S,S,S]) */
template <int S> __device__ __forceinline__ double rp_from(double v) {
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), S * 0x55, 0xf,
                                          0xf, true);
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), S * 0x55, 0xf,
                                          0xf, true);
  return __hiloint2double(hi, lo);
}

/* quad all-gather: all[5s + r] = lane s's mine[r] */
__device__ __forceinline__ void rp_gather(const double (&mine)[5],
                                          double (&all)[20]) {
#pragma unroll
  for (int r = 0; r < 5; r++) {
    all[r] = rp_from<0>(mine[r]);
    all[5 + r] = rp_from<1>(mine[r]);
    all[10 + r] = rp_from<2>(mine[r]);
    all[15 + r] = rp_from<3>(mine[r]);
  }
}

/* the lane's five tipVector entries of site's code at tip row `node` */
__device__ __forceinline__ const double *rp_tip(const RpArgs &A,
                                                const double *tv, int node,
                                                long site) {
  const int c = A.tips[(long)node * A.tipStride + site];
  return tv + 20 * (c < 23 ? c : 22);
}

__device__ __forceinline__ void rp_load(double (&x)[5], const double *p) {
#pragma unroll
  for (int r = 0; r < 5; r++) x[r] = p[r];
}

/* evaluatePartialGeneric for one site at rate ki, on the site's quad (the
 * host restatement is examl_host_evaluate_partial_prot_cat).  slots points
 * at the lane's five states of the site's slot 0. */
__device__ __forceinline__ double rp_evaluate(const RpArgs &A,
                                              const double *sc, double *slots,
                                              long slotStride, long site,
                                              int j, double ki) {
  const double *EIGN = sc + 5 * j, *EI = sc + RP_EI + 100 * j,
               *EV = sc + RP_EV + 5 * j, *tv = sc + RP_TV + 5 * j;
  int scale = 0;
  for (int k = 0; k < A.numOps; k++) {
    const RsOp o = A.ops[k]; /* wave-uniform */
    /* EI and EV are re-read from LDS per entry: hoisted out of this loop
     * their 200 doubles would take every register and spill */
    __asm__ volatile("" ::: "memory");
    double m1[5], m2[5], d1[20], d2[20];
    if (o.tc != EXAML_INNER_INNER)
      rp_load(m1, rp_tip(A, tv, o.a, site));
    else
      rp_load(m1, slots + (long)o.a * slotStride);
    if (o.tc == EXAML_TIP_TIP)
      rp_load(m2, rp_tip(A, tv, o.b, site));
    else
      rp_load(m2, slots + (long)o.b * slotStride);
    const double lz1 = o.lq * ki, lz2 = o.lr * ki;
#pragma unroll
    for (int r = 0; r < 5; r++) {
      double e1 = exp(EIGN[r] * lz1), e2 = exp(EIGN[r] * lz2);
      if (r == 0 && j == 0) e1 = e2 = 1.0; /* state 0, as on the host */
      m1[r] *= e1;
      m2[r] *= e2;
    }
    rp_gather(m1, d1);
    rp_gather(m2, d2);
    double px[5], x1px2[20];
#pragma unroll
    for (int r = 0; r < 5; r++) {
      double u1e = 0, u1o = 0, u2e = 0, u2o = 0;
#pragma unroll
      for (int kk = 0; kk < 20; kk += 2) {
        u1e += d1[kk] * EI[20 * r + kk];
        u1o += d1[kk + 1] * EI[20 * r + kk + 1];
        u2e += d2[kk] * EI[20 * r + kk];
        u2o += d2[kk + 1] * EI[20 * r + kk + 1];
      }
      px[r] = (u1e + u1o) * (u2e + u2o);
    }
    rp_gather(px, x1px2);
    double x3[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int l = 0; l < 20; l++)
#pragma unroll
      for (int r = 0; r < 5; r++) x3[r] += x1px2[l] * EV[20 * l + r];
    int small = 1;
#pragma unroll
    for (int r = 0; r < 5; r++)
      small &= (x3[r] < MINLIKELIHOOD && x3[r] > -MINLIKELIHOOD);
    /* AND over the quad: lane ^ 1 (quad_perm [1,0,3,2]), then lane ^ 2 */
    small &= __builtin_amdgcn_mov_dpp(small, 0xB1, 0xf, 0xf, true);
    small &= __builtin_amdgcn_mov_dpp(small, 0x4E, 0xf, 0xf, true);
    if (small) {
#pragma unroll
      for (int r = 0; r < 5; r++) x3[r] *= TWOTOTHE256;
      scale++;
    }
    double *p3 = slots + (long)o.dst * slotStride;
#pragma unroll
    for (int r = 0; r < 5; r++) p3[r] = x3[r];
  }
  /* evaluatePartialGTRCATPROT tail (:618): lz = log(root_z); the reference's
   * zmin clamp there is dead code, as the host restates */
  double x1[5], x2[5], m[5], all[20];
  rp_load(x1, rp_tip(A, tv, A.rootTip, site));
  rp_load(x2, slots + (long)A.rootSlot * slotStride);
  const double lz = A.rootLz * ki;
#pragma unroll
  for (int r = 0; r < 5; r++) {
    double d = exp(EIGN[r] * lz);
    if (r == 0 && j == 0) d = 1.0;
    m[r] = x1[r] * x2[r] * d;
  }
  rp_gather(m, all);
  double term = 0.0;
#pragma unroll
  for (int l = 0; l < 20; l++) term += all[l];
  term = log(fabs(term)) + (scale * A.logMinlik);
  return term * A.wgt[site];
}

/* The scan loop of k_rate_scan_dna_cat around rp_evaluate; a quad's four
 * lanes run it in lockstep, lane 0 stores. */
template <bool LDS_SLOTS>
__global__ __launch_bounds__(RP_BLOCK) void k_rate_scan_prot_cat(RpArgs A) {
  __shared__ double sc[RP_CONST_DOUBLES];
  extern __shared__ double rp_lds[];
  for (int i = threadIdx.x; i < RP_CONST_DOUBLES; i += RP_BLOCK)
    sc[i] = A.consts[i];
  __syncthreads();
  const int j = threadIdx.x & 3, t = threadIdx.x >> 2;
  const long sites = (long)gridDim.x * RP_SITES;
  const long gsite = (long)blockIdx.x * RP_SITES + t;
  double *slots = LDS_SLOTS ? rp_lds + (t * 20 + 5 * j)
                            : A.scratch + (gsite * 20 + 5 * j);
  const long slotStride = LDS_SLOTS ? 20 * RP_SITES : 20 * sites;
  const double eps = 0.00001;
  for (long i = gsite; i < A.n; i += sites) {
    const double r0 = A.patrat[i];
    double l0 = 0.0, left_lh = 0.0, right_lh = 0.0;
    double left_rate = r0, right_rate = r0, rate = r0;
    int phase = 0, k = 0;
    for (;;) {
      const double v = rp_evaluate(A, sc, slots, slotStride, i, j, rate);
      if (phase == 0) {
        l0 = left_lh = right_lh = v;
        phase = 1;
        k = 1;
      } else if (phase == 1) {
        if (v > left_lh && fabs(left_lh - v) > eps) {
          left_lh = v;
          left_rate = rate;
          k++;
        } else {
          phase = 2;
          k = 1;
        }
      } else {
        if (v > right_lh && fabs(right_lh - v) > eps) {
          right_lh = v;
          right_rate = rate;
          k++;
        } else {
          break;
        }
      }
      if (phase == 1) {
        rate = r0 - (double)k * A.lower;
        if (k > A.max_k || !(rate > 0.0001)) {
          phase = 2;
          k = 1;
        }
      }
      if (phase == 2) {
        if (k > A.max_k) break;
        rate = r0 + (double)k * A.upper;
      }
    }
    if (j != 0) continue;
    if (right_lh > l0 || left_lh > l0) {
      if (right_lh > left_lh) {
        A.patrat[i] = right_rate;
        A.lhs[i] = right_lh;
      } else {
        A.patrat[i] = left_rate;
        A.lhs[i] = left_lh;
      }
    } else {
      A.lhs[i] = l0;
    }
  }
}

/* --- host side -------------------------------------------------------------*/

static int rp_grid(long n) {
  const long g = (n + RP_SITES - 1) / RP_SITES;
  return (int)(g < RP_MAX_GRID ? (g > 0 ? g : 1) : RP_MAX_GRID);
}

static bool rp_in_lds(int L, int ldsBudgetBytes) {
  long budget = ldsBudgetBytes < 0 ? RP_LDS_BUDGET : ldsBudgetBytes;
  if (budget > RP_LDS_MAX) budget = RP_LDS_MAX;
  return (long)L * RP_SLOT_BYTES <= budget;
}

extern "C" long examl_hip_rate_scan_prot_table_bytes(int numOps) {
  return RP_CONST_DOUBLES * 8L + (long)numOps * (long)sizeof(RsOp);
}

extern "C" long examl_hip_rate_scan_prot_scratch_bytes(int L, long n,
                                                       int ldsBudgetBytes) {
  if (rp_in_lds(L, ldsBudgetBytes)) return 0;
  return (long)L * RP_SLOT_BYTES * rp_grid(n);
}

extern "C" int examl_hip_rate_scan_prot_sites(void) {
  return RP_SITES * RP_MAX_GRID;
}

extern "C" int examl_hip_rate_scan_prot_cat(
    const examl_hip_trav_entry *ops, int numOps, int mxtips,
    int rootTipNumber, int rootQNumber, double root_z, const double *EIGN,
    const double *EI, const double *EV, const double *tipVector,
    const unsigned char *dev_tips, long tipStrideBytes, const int *dev_wgt,
    long n, double lower_spacing, double upper_spacing, int max_k,
    int ldsBudgetBytes, double *dev_patrat, double *dev_lhs, void *dev_table,
    long tableBytes, void *dev_scratch, long scratchBytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  g_rate_kernel_launches = 0;
  if (!g_use_rate_kernel) return 0;
  (void)hipGetLastError();
  if (n < 1 || numOps < 1 || rootTipNumber < 1 || rootTipNumber > mxtips ||
      max_k < 0 || tipStrideBytes < n)
    return set_err(hipErrorInvalidValue, "rate_scan_prot: arguments");
  std::vector<int> slot((size_t)numOps);
  int L = 0;
  if (examl_host_rate_scan_plan(ops, numOps, mxtips, slot.data(), &L) != 0)
    return set_err(hipErrorInvalidValue, "rate_scan_prot: entry list");
  const bool inLds = rp_in_lds(L, ldsBudgetBytes);
  const size_t need = (size_t)examl_hip_rate_scan_prot_table_bytes(numOps);
  if ((size_t)tableBytes < need ||
      scratchBytes <
          examl_hip_rate_scan_prot_scratch_bytes(L, n, ldsBudgetBytes))
    return set_err(hipErrorInvalidValue, "rate_scan_prot: buffer sizes");

  void *buf = nullptr;
  if (int rc = rs_stage_acquire(need, &buf)) return rc;
  double *c = (double *)buf;
  memcpy(c, EIGN, 20 * 8);
  memcpy(c + RP_EI, EI, 400 * 8);
  memcpy(c + RP_EV, EV, 400 * 8);
  memcpy(c + RP_TV, tipVector, 460 * 8);
  const int rootSlot =
      rs_fill_ops(ops, numOps, mxtips, rootQNumber, slot.data(),
                  (RsOp *)(c + RP_CONST_DOUBLES));
  if (rootSlot < 0)
    return set_err(hipErrorInvalidValue,
                   "rate_scan_prot: root q not in the list");
  if (int rc = rs_stage_upload(dev_table, need, s)) return rc;

  RpArgs A;
  A.consts = (const double *)dev_table;
  A.ops = (const RsOp *)((const double *)dev_table + RP_CONST_DOUBLES);
  A.numOps = numOps;
  A.rootTip = rootTipNumber;
  A.rootSlot = rootSlot;
  A.max_k = max_k;
  A.rootLz = log(root_z);
  A.logMinlik = log(MINLIKELIHOOD);
  A.lower = lower_spacing;
  A.upper = upper_spacing;
  A.tips = dev_tips;
  A.tipStride = tipStrideBytes;
  A.n = n;
  A.wgt = dev_wgt;
  A.patrat = dev_patrat;
  A.lhs = dev_lhs;
  A.scratch = (double *)dev_scratch;
  const int grid = rp_grid(n);
  if (inLds)
    hipLaunchKernelGGL(k_rate_scan_prot_cat<true>, dim3(grid), dim3(RP_BLOCK),
                       (size_t)L * RP_SLOT_BYTES, s, A);
  else
    hipLaunchKernelGGL(k_rate_scan_prot_cat<false>, dim3(grid),
                       dim3(RP_BLOCK), 0, s, A);
  CHK(hipGetLastError());
  g_rate_kernel_launches = 1;
  g_rate_slot_home = inLds ? 0 : 1;
  return 0;
}
