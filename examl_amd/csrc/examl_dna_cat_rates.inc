/* ============================================================================
 * examl_dna_cat_rates.inc — the -m PSR per-site rate search on the GPU.
 *
 * k_rate_scan_dna_cat replaces the per-site loop of optRateCatPthreads
 * (examl/optimizeModel.c:1798) together with the evaluatePartialGeneric it
 * calls for every candidate rate (examl/evaluatePartialGenericSpecial.c:259,
 * computeVectorGTRCAT :924, evaluatePartialGTRCAT :998).  One lane owns one
 * site and runs that site's whole search: every candidate rate is a complete
 * post-order walk of the tree for that one site.
 *
 * Included by examl_hip.hip (same flags, -ffp-contract=off: the candidate
 * rates r0 -/+ k*spacing and all CLV arithmetic round as the host's do).
 *
 * Data movement
 *  - EIGN, EI, EV and the 16x4 tipVector: LDS, once per block.
 *  - the entry table (tip rows / slots and the two hoisted log branch
 *    lengths of each entry): the index is wave-uniform, so every read is a
 *    wave-wide scalar load.
 *  - tip codes: one byte per lane and tip, coalesced.
 *  - the private CLV stack: L slots of 32 bytes per RESIDENT lane, laid out
 *    [slot][lane] so a wave moves 2 KiB contiguous.  LDS_SLOTS picks their
 *    home: dynamic LDS (L * 32 B * RS_BLOCK) or global scratch sized
 *    gridDim * RS_BLOCK lanes, never n.
 * A lane reads and writes only its own slot elements and there is no vote or
 * shuffle, so lanes past the last site simply do nothing.
 * ==========================================================================*/

#define RS_BLOCK 64        /* one wave per block: no barrier after start */
#define RS_MAX_GRID 4096   /* resident lanes = 262,144 (<= MAX_GRID blocks) */
#define RS_CONST_DOUBLES 100 /* EIGN 4 | EI 16 | EV 16 | tipVector 64 */
#define RS_LDS_BUDGET (16 * 1024) /* default: LDS slots while L <= 8 */

/* one entry as the kernel reads it; a = x1's tip row or slot, b = x2's */
struct RsOp {
  int tc, a, b, dst;
  double lq, lr; /* log(max(qz, zmin)), log(max(rz, zmin)) */
};

struct RsArgs {
  const double *consts; /* RS_CONST_DOUBLES */
  const RsOp *ops;
  int numOps, rootTip, rootSlot, max_k;
  double rootLz, logMinlik, lower, upper;
  const unsigned char *tips;
  long tipStride, n;
  const int *wgt;
  double *patrat, *lhs;
  v4d *scratch;
};

/* evaluatePartialGeneric for one site at rate ki (the host restatement is
 * examl_host_evaluate_partial_dna_cat, index for index) */
template <bool LDS_SLOTS>
__device__ __forceinline__ double rs_evaluate(const RsArgs &A,
                                              const double *sc, v4d *slots,
                                              long slotStride, long site,
                                              double ki) {
  const double *EIGN = sc, *EI = sc + 4, *EV = sc + 20, *tv = sc + 36;
  int scale = 0;
  for (int k = 0; k < A.numOps; k++) {
    const RsOp o = A.ops[k]; /* wave-uniform */
    v4d x1, x2;
    if (o.tc != EXAML_INNER_INNER) {
      const double *t = tv + 4 * (A.tips[(long)o.a * A.tipStride + site] & 15);
      x1 = (v4d){t[0], t[1], t[2], t[3]};
    } else {
      x1 = slots[(long)o.a * slotStride];
    }
    if (o.tc == EXAML_TIP_TIP) {
      const double *t = tv + 4 * (A.tips[(long)o.b * A.tipStride + site] & 15);
      x2 = (v4d){t[0], t[1], t[2], t[3]};
    } else {
      x2 = slots[(long)o.b * slotStride];
    }
    const double lz1 = o.lq * ki, lz2 = o.lr * ki;
    double d1[3], d2[3], x1px2[4];
#pragma unroll
    for (int j = 0; j < 3; j++) {
      d1[j] = x1[j + 1] * exp(EIGN[j + 1] * lz1);
      d2[j] = x2[j + 1] * exp(EIGN[j + 1] * lz2);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      double u1 = x1[0], u2 = x2[0];
#pragma unroll
      for (int kk = 0; kk < 3; kk++) {
        u1 += d1[kk] * EI[j * 4 + kk + 1];
        u2 += d2[kk] * EI[j * 4 + kk + 1];
      }
      x1px2[j] = u1 * u2;
    }
    v4d x3 = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int kk = 0; kk < 4; kk++) x3[kk] += x1px2[j] * EV[4 * j + kk];
    if (x3[0] < MINLIKELIHOOD && x3[0] > -MINLIKELIHOOD &&
        x3[1] < MINLIKELIHOOD && x3[1] > -MINLIKELIHOOD &&
        x3[2] < MINLIKELIHOOD && x3[2] > -MINLIKELIHOOD &&
        x3[3] < MINLIKELIHOOD && x3[3] > -MINLIKELIHOOD) {
      x3 *= TWOTOTHE256;
      scale++;
    }
    slots[(long)o.dst * slotStride] = x3;
  }
  /* evaluatePartialGTRCAT tail (:998): lz = log(root_z), no zmin clamp */
  const double *x1 = tv + 4 * (A.tips[(long)A.rootTip * A.tipStride + site] & 15);
  const v4d x2 = slots[(long)A.rootSlot * slotStride];
  const double lz = A.rootLz * ki;
  const double d0 = exp(EIGN[1] * lz), dd1 = exp(EIGN[2] * lz),
               dd2 = exp(EIGN[3] * lz);
  double term = x1[0] * x2[0];
  term += x1[1] * x2[1] * d0;
  term += x1[2] * x2[2] * dd1;
  term += x1[3] * x2[3] * dd2;
  term = log(fabs(term)) + (scale * A.logMinlik);
  return term * A.wgt[site];
}

/* The scan of optRateCatPthreads (optimizeModel.c:1798) as one loop around
 * one evaluation: phase 0 evaluates at r0, phase 1 walks down by
 * lower_spacing, phase 2 walks up by upper_spacing.  Lanes of a wave that
 * are in different phases still share every evaluation. */
template <bool LDS_SLOTS>
__global__ __launch_bounds__(RS_BLOCK) void k_rate_scan_dna_cat(RsArgs A) {
  __shared__ double sc[RS_CONST_DOUBLES];
  extern __shared__ v4d rs_lds[];
  for (int i = threadIdx.x; i < RS_CONST_DOUBLES; i += RS_BLOCK)
    sc[i] = A.consts[i];
  __syncthreads();
  const long lanes = (long)gridDim.x * RS_BLOCK;
  const long gtid = (long)blockIdx.x * RS_BLOCK + threadIdx.x;
  v4d *slots = LDS_SLOTS ? rs_lds + threadIdx.x : A.scratch + gtid;
  const long slotStride = LDS_SLOTS ? RS_BLOCK : lanes;
  const double eps = 0.00001;
  for (long i = gtid; i < A.n; i += lanes) {
    const double r0 = A.patrat[i];
    double l0 = 0.0, left_lh = 0.0, right_lh = 0.0;
    double left_rate = r0, right_rate = r0, rate = r0;
    int phase = 0, k = 0;
    for (;;) {
      const double v = rs_evaluate<LDS_SLOTS>(A, sc, slots, slotStride, i, rate);
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

static bool g_use_rate_kernel = true;
static thread_local int g_rate_kernel_launches = 0;
static thread_local int g_rate_slot_home = 0; /* 0 = LDS, 1 = global */

extern "C" void examl_hip_use_rate_kernel(int on) {
  g_use_rate_kernel = on != 0;
}
extern "C" int examl_hip_rate_kernel_launches(void) {
  return g_rate_kernel_launches;
}
extern "C" int examl_hip_rate_scan_slot_home(void) { return g_rate_slot_home; }

static int rs_grid(long n) {
  const long g = (n + RS_BLOCK - 1) / RS_BLOCK;
  return (int)(g < RS_MAX_GRID ? (g > 0 ? g : 1) : RS_MAX_GRID);
}

static bool rs_in_lds(int L, int ldsBudgetBytes) {
  const long budget = ldsBudgetBytes < 0 ? RS_LDS_BUDGET : ldsBudgetBytes;
  return (long)L * 32 * RS_BLOCK <= budget;
}

extern "C" long examl_hip_rate_scan_table_bytes(int numOps) {
  return RS_CONST_DOUBLES * 8L + (long)numOps * (long)sizeof(RsOp);
}

extern "C" long examl_hip_rate_scan_scratch_bytes(int L, long n,
                                                  int ldsBudgetBytes) {
  if (rs_in_lds(L, ldsBudgetBytes)) return 0;
  return (long)L * 32 * RS_BLOCK * rs_grid(n);
}

extern "C" int examl_hip_rate_scan_lanes(void) {
  return RS_BLOCK * RS_MAX_GRID;
}

/* pinned staging of the table: refilled only after the previous copy out of
 * it has finished */
struct RsStage {
  void *buf;
  size_t cap;
  hipEvent_t ev;
  bool busy;
};
static thread_local RsStage g_rs_stage = {nullptr, 0, nullptr, false};

/* the staging buffer, idle and with room for `need` bytes */
static int rs_stage_acquire(size_t need, void **buf) {
  RsStage &st = g_rs_stage;
  if (!st.ev) CHK(hipEventCreateWithFlags(&st.ev, hipEventDisableTiming));
  if (st.busy) CHK(hipEventSynchronize(st.ev));
  st.busy = false;
  if (need > st.cap) {
    if (st.buf) CHK(hipHostFree(st.buf));
    st.buf = nullptr;
    st.cap = 0;
    CHK(hipHostMalloc(&st.buf, 2 * need));
    st.cap = 2 * need;
  }
  *buf = st.buf;
  return 0;
}

static int rs_stage_upload(void *dev_table, size_t need, hipStream_t s) {
  RsStage &st = g_rs_stage;
  CHK(hipMemcpyAsync(dev_table, st.buf, need, hipMemcpyHostToDevice, s));
  CHK(hipEventRecord(st.ev, s));
  st.busy = true;
  return 0;
}

/* the entry table as the kernels read it; returns the slot of the root's q,
 * the one result nobody consumed, or -1 */
static int rs_fill_ops(const examl_hip_trav_entry *ops, int numOps,
                       int mxtips, int rootQNumber, const int *slot,
                       RsOp *t) {
  std::vector<int> slot_of_node((size_t)(2 * mxtips), -1);
  for (int k = 0; k < numOps; k++) {
    const examl_hip_trav_entry &e = ops[k];
    /* tips are read by node id (row of dev_tips); inner operands by the
     * slot of the entry that produced them — the planner has checked that
     * one did and that the ids are in range */
    t[k].tc = e.tipCase;
    t[k].a = e.tipCase != EXAML_INNER_INNER
                 ? e.qNumber : slot_of_node[(size_t)e.qNumber];
    t[k].b = e.tipCase == EXAML_TIP_TIP
                 ? e.rNumber : slot_of_node[(size_t)e.rNumber];
    t[k].dst = slot[k];
    t[k].lq = (e.qz > ZMIN) ? log(e.qz) : log(ZMIN);
    t[k].lr = (e.rz > ZMIN) ? log(e.rz) : log(ZMIN);
    slot_of_node[(size_t)e.pNumber] = slot[k];
  }
  if (rootQNumber > mxtips && rootQNumber <= 2 * mxtips - 2)
    return slot_of_node[(size_t)rootQNumber];
  return -1;
}

extern "C" int examl_hip_rate_scan_dna_cat(
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
    return set_err(hipErrorInvalidValue, "rate_scan: arguments");
  std::vector<int> slot((size_t)numOps);
  int L = 0, rootSlot = -1;
  if (examl_host_rate_scan_plan(ops, numOps, mxtips, slot.data(), &L) != 0)
    return set_err(hipErrorInvalidValue, "rate_scan: entry list");
  const bool inLds = rs_in_lds(L, ldsBudgetBytes);
  const size_t need = (size_t)examl_hip_rate_scan_table_bytes(numOps);
  if ((size_t)tableBytes < need ||
      scratchBytes < examl_hip_rate_scan_scratch_bytes(L, n, ldsBudgetBytes))
    return set_err(hipErrorInvalidValue, "rate_scan: buffer sizes");

  void *buf = nullptr;
  if (int rc = rs_stage_acquire(need, &buf)) return rc;
  double *c = (double *)buf;
  memcpy(c, EIGN, 4 * 8);
  memcpy(c + 4, EI, 16 * 8);
  memcpy(c + 20, EV, 16 * 8);
  memcpy(c + 36, tipVector, 64 * 8);
  rootSlot = rs_fill_ops(ops, numOps, mxtips, rootQNumber, slot.data(),
                         (RsOp *)(c + RS_CONST_DOUBLES));
  if (rootSlot < 0)
    return set_err(hipErrorInvalidValue, "rate_scan: root q not in the list");
  if (int rc = rs_stage_upload(dev_table, need, s)) return rc;

  RsArgs A;
  A.consts = (const double *)dev_table;
  A.ops = (const RsOp *)((const double *)dev_table + RS_CONST_DOUBLES);
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
  A.scratch = (v4d *)dev_scratch;
  const int grid = rs_grid(n);
  if (inLds)
    hipLaunchKernelGGL(k_rate_scan_dna_cat<true>, dim3(grid), dim3(RS_BLOCK),
                       (size_t)L * 32 * RS_BLOCK, s, A);
  else
    hipLaunchKernelGGL(k_rate_scan_dna_cat<false>, dim3(grid), dim3(RS_BLOCK),
                       0, s, A);
  CHK(hipGetLastError());
  g_rate_kernel_launches = 1;
  g_rate_slot_home = inLds ? 0 : 1;
  return 0;
}
