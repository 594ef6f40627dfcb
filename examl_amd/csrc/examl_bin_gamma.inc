/* ============================================================================
 * examl_bin_gamma.inc — binary (two-state, BINARY/MORPHOLOGICAL) GTRGAMMA
 * kernels and their L0 launchers.  Included by examl_hip.hip, which provides
 * NV_BLOCK, MAX_GRID, grid_for, v2d, the constants, k_reduce_lnl/k_reduce_2
 * and CHK.
 *
 * Layout: a site's span is 8 doubles, x[site*8 + cat*2 + state]; P blocks
 * are left[cat*4 + row*2 + col] | right[...] (16 + 16 doubles); tipVector
 * is [code*2 + state], codes 0..3.
 *
 * Mapping: one lane per (site, cat) as in the DNA kernels, so a lane moves
 * one 16-byte pair per operand and a wave touches 1 KiB contiguous per
 * vector op; the 4 lanes of a site are 4-aligned (units = 4n), which is what
 * the rescale ballot and the per-site shuffles rely on.
 * ==========================================================================*/

/* --- newview ---------------------------------------------------------------
 * Restates newviewGTRGAMMA_BINARY (newviewGenericSpecial.c:6034) expression
 * by expression, per (site, cat k):
 *   x3[j] = 0
 *   for l in 0,1:  al = x1[0]*L[k][l][0] + x1[1]*L[k][l][1]   (mul, hadd)
 *                  ar = x2[0]*R[k][l][0] + x2[1]*R[k][l][1]
 *                  x3[j] += (al*ar) * EV[2*l + j]
 * The accumulator starts at zero and is added to, as the reference's
 * _mm_setzero_pd / _mm_add_pd does, so signed zeros agree.  A tip operand's
 * al/ar comes from an LDS table of the same dot product over tipVector.
 * Rescale (TIP_INNER / INNER_INNER only, :6111-6138): if all 8 |x3| of the
 * site are strictly below 2^-256, the 8 are multiplied by 2^256 and
 * wgt[site] is added to the entry's scaler increment by one lane per site.
 */
template <int TC, bool NT>
__global__ __launch_bounds__(NV_BLOCK) void k_newview_bin_gamma(
    const double *__restrict__ x1, const double *__restrict__ x2,
    double *__restrict__ x3, const double *__restrict__ P,
    const double *__restrict__ EV, const double *__restrict__ tipVec,
    const unsigned char *__restrict__ tipX1,
    const unsigned char *__restrict__ tipX2, const int *__restrict__ wgt,
    long n, unsigned int *__restrict__ scalerInc) {
  __shared__ double sL[16], sR[16], sEV[4], sTV[8];
  /* tip tables: entry (code, cat, row), 4 codes x 4 cats x 2 rows */
  __shared__ double sU1[TC != EXAML_INNER_INNER ? 32 : 1];
  __shared__ double sU2[TC == EXAML_TIP_TIP ? 32 : 1];

  const int tid = threadIdx.x;
  if (tid < 16) {
    sL[tid] = P[tid];
    sR[tid] = P[16 + tid];
  }
  if (tid < 8) sTV[tid] = tipVec[tid];
  if (tid < 4) sEV[tid] = EV[tid];
  __syncthreads();

  if (TC != EXAML_INNER_INNER) {
    if (tid < 32) {
      const int code = tid >> 3, cat = (tid >> 1) & 3, row = tid & 1;
      const double *tv = &sTV[code * 2];
      const double *pl = &sL[cat * 4 + row * 2];
      sU1[tid] = tv[0] * pl[0] + tv[1] * pl[1];
      if (TC == EXAML_TIP_TIP) {
        const double *pr = &sR[cat * 4 + row * 2];
        sU2[tid] = tv[0] * pr[0] + tv[1] * pr[1];
      }
    }
    __syncthreads();
  }

  const long units = n * 4;
  const int lane = tid & 63;
  for (long idx = (long)blockIdx.x * NV_BLOCK + tid; idx < units;
       idx += (long)gridDim.x * NV_BLOCK) {
    const long site = idx >> 2;
    const int cat = (int)(idx & 3);
    double al[2], ar[2];

    if (TC == EXAML_INNER_INNER) {
      const v2d xl = *reinterpret_cast<const v2d *>(&x1[idx * 2]);
      const v2d xr = *reinterpret_cast<const v2d *>(&x2[idx * 2]);
#pragma unroll
      for (int l = 0; l < 2; l++) {
        const double *pl = &sL[cat * 4 + l * 2];
        const double *pr = &sR[cat * 4 + l * 2];
        al[l] = xl.x * pl[0] + xl.y * pl[1];
        ar[l] = xr.x * pr[0] + xr.y * pr[1];
      }
    } else if (TC == EXAML_TIP_INNER) {
      const int code = tipX1[site] & 3;
      const v2d xr = *reinterpret_cast<const v2d *>(&x2[idx * 2]);
#pragma unroll
      for (int l = 0; l < 2; l++) {
        const double *pr = &sR[cat * 4 + l * 2];
        al[l] = sU1[code * 8 + cat * 2 + l];
        ar[l] = xr.x * pr[0] + xr.y * pr[1];
      }
    } else {
      const int c1 = tipX1[site] & 3, c2 = tipX2[site] & 3;
#pragma unroll
      for (int l = 0; l < 2; l++) {
        al[l] = sU1[c1 * 8 + cat * 2 + l];
        ar[l] = sU2[c2 * 8 + cat * 2 + l];
      }
    }

    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int l = 0; l < 2; l++) {
      const double t = al[l] * ar[l];
      a0 += t * sEV[l * 2 + 0];
      a1 += t * sEV[l * 2 + 1];
    }

    if (TC != EXAML_TIP_TIP) {
      /* site-wide rescale vote over the site's 4 lanes */
      const bool small =
          (fabs(a0) < MINLIKELIHOOD) & (fabs(a1) < MINLIKELIHOOD);
      const unsigned long long m = __ballot(small);
      if (((m >> (lane & ~3)) & 0xFULL) == 0xFULL) {
        a0 *= TWOTOTHE256;
        a1 *= TWOTOTHE256;
        if ((lane & 3) == 0) atomicAdd(scalerInc, (unsigned int)wgt[site]);
      }
    }
    if (NT)
      __builtin_nontemporal_store((v2d){a0, a1},
                                  reinterpret_cast<v2d *>(&x3[idx * 2]));
    else
      *reinterpret_cast<v2d *>(&x3[idx * 2]) = (v2d){a0, a1};
  }
}

/* --- evaluate --------------------------------------------------------------
 * Restates evaluateGTRGAMMA_BINARY (evaluateGenericSpecial.c:1074):
 *   termv = {0, 0};  for cat j: termv += (x1[j] * x2[j]) * diag[j]   (pairs)
 *   lnL  += wgt[i] * log(0.25 * fabs(termv[0] + termv[1]))
 * Each lane forms its cat's pair; the first lane of the site gathers the
 * four pairs and adds them in cat order, then adds the two halves.
 */
template <bool TIP>
__global__ __launch_bounds__(NV_BLOCK) void k_evaluate_bin_gamma(
    const double *__restrict__ x1, const double *__restrict__ x2,
    const double *__restrict__ tipVec, const unsigned char *__restrict__ tipX1,
    const int *__restrict__ wgt, const double *__restrict__ diag, long n,
    double *__restrict__ partials) {
  __shared__ double sD[8], sTV[8], sRed[NV_BLOCK / 64];
  const int tid = threadIdx.x;
  if (tid < 8) {
    sD[tid] = diag[tid];
    if (TIP) sTV[tid] = tipVec[tid];
  }
  __syncthreads();

  const long units = n * 4;
  const int lane = tid & 63;
  double acc = 0.0;
  for (long idx = (long)blockIdx.x * NV_BLOCK + tid; idx < units;
       idx += (long)gridDim.x * NV_BLOCK) {
    const long site = idx >> 2;
    const int cat = (int)(idx & 3);
    const v2d b = *reinterpret_cast<const v2d *>(&x2[idx * 2]);
    double p0, p1;
    if (TIP) {
      const double *tv = &sTV[(tipX1[site] & 3) * 2];
      p0 = (tv[0] * b.x) * sD[cat * 2 + 0];
      p1 = (tv[1] * b.y) * sD[cat * 2 + 1];
    } else {
      const v2d a = *reinterpret_cast<const v2d *>(&x1[idx * 2]);
      p0 = (a.x * b.x) * sD[cat * 2 + 0];
      p1 = (a.y * b.y) * sD[cat * 2 + 1];
    }
    double t0 = 0.0, t1 = 0.0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      t0 += __shfl(p0, j, 4);
      t1 += __shfl(p1, j, 4);
    }
    if ((lane & 3) == 0)
      acc += (double)wgt[site] * log(0.25 * fabs(t0 + t1));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if (lane == 0) sRed[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = 0;
#pragma unroll
    for (int w = 0; w < NV_BLOCK / 64; w++) s += sRed[w];
    partials[blockIdx.x] = s; /* deterministic 2-pass reduction */
  }
}

/* --- sum (makenewz precompute) ---------------------------------------------
 * Restates sumGAMMA_BINARY (makenewzGenericSpecial.c:1543): the per-cat
 * pair product, a tip operand being the same tipVector pair in every cat.
 */
template <int TC>
__global__ __launch_bounds__(NV_BLOCK) void k_sum_bin_gamma(
    double *__restrict__ sum, const double *__restrict__ x1,
    const double *__restrict__ x2, const double *__restrict__ tipVec,
    const unsigned char *__restrict__ tipX1,
    const unsigned char *__restrict__ tipX2, long n) {
  __shared__ double sTV[8];
  const int tid = threadIdx.x;
  if (TC != EXAML_INNER_INNER) {
    if (tid < 8) sTV[tid] = tipVec[tid];
    __syncthreads();
  }

  const long units = n * 4;
  for (long idx = (long)blockIdx.x * NV_BLOCK + tid; idx < units;
       idx += (long)gridDim.x * NV_BLOCK) {
    const long site = idx >> 2;
    v2d a, b;
    if (TC == EXAML_TIP_TIP) {
      const double *t1 = &sTV[(tipX1[site] & 3) * 2];
      const double *t2 = &sTV[(tipX2[site] & 3) * 2];
      a = (v2d){t1[0], t1[1]};
      b = (v2d){t2[0], t2[1]};
    } else if (TC == EXAML_TIP_INNER) {
      const double *t1 = &sTV[(tipX1[site] & 3) * 2];
      a = (v2d){t1[0], t1[1]};
      b = *reinterpret_cast<const v2d *>(&x2[idx * 2]);
    } else {
      a = *reinterpret_cast<const v2d *>(&x1[idx * 2]);
      b = *reinterpret_cast<const v2d *>(&x2[idx * 2]);
    }
    *reinterpret_cast<v2d *>(&sum[idx * 2]) = (v2d){a.x * b.x, a.y * b.y};
  }
}

/* --- core (NR derivatives) -------------------------------------------------
 * Restates coreGTRGAMMA_BINARY (makenewzGenericSpecial.c:1464), per site:
 *   a0 = a1 = a2 = {0, 0}
 *   for cat j: tmp = d0[j]*sum[j]; a0 += tmp; a1 += tmp*d1[j]; a2 += tmp*d2[j]
 *   a* = a*[0] + a*[1]                                             (hadd)
 *   inv = 1/|a0|; d1 = a1*inv; d2 = a2*inv
 *   dlnL += w*d1; d2lnL += w*(d2 - d1*d1)
 * dtab = {d0[8], d1[8], d2[8]} from examl_host_core_dtables_bin.
 */
__global__ __launch_bounds__(NV_BLOCK) void k_core_bin_gamma(
    const double *__restrict__ sum, const double *__restrict__ dtab,
    const int *__restrict__ wgt, long n, double *__restrict__ partials) {
  __shared__ double sD[24], sRed[2][NV_BLOCK / 64];
  const int tid = threadIdx.x;
  if (tid < 24) sD[tid] = dtab[tid];
  __syncthreads();

  const long units = n * 4;
  const int lane = tid & 63;
  double accD1 = 0.0, accD2 = 0.0;
  for (long idx = (long)blockIdx.x * NV_BLOCK + tid; idx < units;
       idx += (long)gridDim.x * NV_BLOCK) {
    const long site = idx >> 2;
    const int cat = (int)(idx & 3);
    const v2d s = *reinterpret_cast<const v2d *>(&sum[idx * 2]);
    const double t0 = sD[cat * 2 + 0] * s.x, t1 = sD[cat * 2 + 1] * s.y;
    const double u0 = t0 * sD[8 + cat * 2 + 0], u1 = t1 * sD[8 + cat * 2 + 1];
    const double v0 = t0 * sD[16 + cat * 2 + 0],
                 v1 = t1 * sD[16 + cat * 2 + 1];
    double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0, a20 = 0.0, a21 = 0.0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      a00 += __shfl(t0, j, 4);
      a01 += __shfl(t1, j, 4);
      a10 += __shfl(u0, j, 4);
      a11 += __shfl(u1, j, 4);
      a20 += __shfl(v0, j, 4);
      a21 += __shfl(v1, j, 4);
    }
    if ((lane & 3) == 0) {
      const double inv = 1.0 / fabs(a00 + a01);
      const double d1 = (a10 + a11) * inv, d2 = (a20 + a21) * inv;
      const double w = (double)wgt[site];
      accD1 += w * d1;
      accD2 += w * (d2 - d1 * d1);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    accD1 += __shfl_down(accD1, off);
    accD2 += __shfl_down(accD2, off);
  }
  if (lane == 0) {
    sRed[0][tid >> 6] = accD1;
    sRed[1][tid >> 6] = accD2;
  }
  __syncthreads();
  if (tid == 0) {
    double s1 = 0, s2 = 0;
#pragma unroll
    for (int w = 0; w < NV_BLOCK / 64; w++) {
      s1 += sRed[0][w];
      s2 += sRed[1][w];
    }
    partials[2 * blockIdx.x] = s1; /* deterministic 2-pass reduction */
    partials[2 * blockIdx.x + 1] = s2;
  }
}

/* --- L0 launchers ----------------------------------------------------------
 * Streaming stores start where a CLV is 8 MB, the byte size at which the DNA
 * kernels start (n >= 65536 there).  The threshold is a model until
 * someone measures near it; examl_hip_bin_force_nt overrides it for A/B
 * runs (DESIGN.md §7e).
 */
#define BIN_NT_SITES 131072L
static int g_bin_nt_mode = -1;

extern "C" void examl_hip_bin_force_nt(int mode) {
  g_bin_nt_mode = mode < 0 ? -1 : (mode ? 1 : 0);
  examl_hip_graphs_clear(); /* cached graphs hold the other kernel variant */
}

extern "C" int examl_hip_bin_nt_threshold(void) { return (int)BIN_NT_SITES; }

static inline bool bin_nt(long n) {
  return g_bin_nt_mode < 0 ? n >= BIN_NT_SITES : g_bin_nt_mode != 0;
}

#define NV_BIN(TCV, NTV)                                                     \
  hipLaunchKernelGGL((k_newview_bin_gamma<TCV, NTV>), dim3(grid),            \
                     dim3(NV_BLOCK), 0, s, x1, x2, x3, P, EV, tipVec, tipX1, \
                     tipX2, wgt, n, scalerInc)

/* one binary newview launch; P = left | right (32 doubles).  Returns -1 for
 * a bad tipCase (nothing launched), else 0; the caller reads
 * hipGetLastError. */
static int launch_newview_bin(int tipCase, hipStream_t s, const double *x1,
                              const double *x2, double *x3, const double *P,
                              const double *EV, const double *tipVec,
                              const unsigned char *tipX1,
                              const unsigned char *tipX2, const int *wgt,
                              long n, unsigned int *scalerInc) {
  const int grid = grid_for(n * 4);
  const bool nt = bin_nt(n);
  switch (tipCase) {
  case EXAML_TIP_TIP:
    if (nt) NV_BIN(EXAML_TIP_TIP, true);
    else NV_BIN(EXAML_TIP_TIP, false);
    return 0;
  case EXAML_TIP_INNER:
    if (nt) NV_BIN(EXAML_TIP_INNER, true);
    else NV_BIN(EXAML_TIP_INNER, false);
    return 0;
  case EXAML_INNER_INNER:
    if (nt) NV_BIN(EXAML_INNER_INNER, true);
    else NV_BIN(EXAML_INNER_INNER, false);
    return 0;
  default:
    snprintf(g_err, sizeof(g_err), "newview_bin: bad tipCase %d", tipCase);
    return -1;
  }
}
#undef NV_BIN

extern "C" int examl_hip_newview_bin_gamma(
    int tipCase, const double *x1, const double *x2, double *x3,
    const double *EV, const double *tipVec, const unsigned char *tipX1,
    const unsigned char *tipX2, long n, const double *left,
    const double *right, const int *wgt, unsigned int *scalerInc,
    void *stream) {
  if (n <= 0) return 0;
  (void)hipGetLastError(); /* clear stale per-thread error (e.g. torch probes) */
  if (right != left + 16) {
    snprintf(g_err, sizeof(g_err),
             "newview_bin: right must be left+16 (one 32-double P block)");
    return -1;
  }
  if (launch_newview_bin(tipCase, (hipStream_t)stream, x1, x2, x3, left, EV,
                         tipVec, tipX1, tipX2, wgt, n, scalerInc) != 0)
    return -1;
  CHK(hipGetLastError());
  return 0;
}

extern "C" int examl_hip_evaluate_bin_gamma(
    const int *wgt, const double *x1, const double *x2, const double *tipVec,
    const unsigned char *tipX1, long n, const double *diag,
    const unsigned int *gsP, const unsigned int *gsQ, double log_minlik,
    double *dev_partials, double *lnl, void *stream) {
  if (n <= 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  (void)hipGetLastError(); /* clear stale per-thread error (e.g. torch probes) */
  const int grid = grid_for(n * 4);
  if (tipX1)
    hipLaunchKernelGGL((k_evaluate_bin_gamma<true>), dim3(grid),
                       dim3(NV_BLOCK), 0, s, x1, x2, tipVec, tipX1, wgt, diag,
                       n, dev_partials);
  else
    hipLaunchKernelGGL((k_evaluate_bin_gamma<false>), dim3(grid),
                       dim3(NV_BLOCK), 0, s, x1, x2, tipVec, tipX1, wgt, diag,
                       n, dev_partials);
  CHK(hipGetLastError());
  hipLaunchKernelGGL(k_reduce_lnl, dim3(1), dim3(NV_BLOCK), 0, s,
                     dev_partials, grid, gsP, gsQ, log_minlik, lnl);
  CHK(hipGetLastError());
  return 0;
}

extern "C" int examl_hip_sum_bin_gamma(int tipCase, double *sum,
                                       const double *x1, const double *x2,
                                       const double *tipVec,
                                       const unsigned char *tipX1,
                                       const unsigned char *tipX2, long n,
                                       void *stream) {
  if (n <= 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  (void)hipGetLastError(); /* clear stale per-thread error (e.g. torch probes) */
  const int grid = grid_for(n * 4);
  switch (tipCase) {
  case EXAML_TIP_TIP:
    hipLaunchKernelGGL((k_sum_bin_gamma<EXAML_TIP_TIP>), dim3(grid),
                       dim3(NV_BLOCK), 0, s, sum, x1, x2, tipVec, tipX1,
                       tipX2, n);
    break;
  case EXAML_TIP_INNER:
    hipLaunchKernelGGL((k_sum_bin_gamma<EXAML_TIP_INNER>), dim3(grid),
                       dim3(NV_BLOCK), 0, s, sum, x1, x2, tipVec, tipX1,
                       tipX2, n);
    break;
  case EXAML_INNER_INNER:
    hipLaunchKernelGGL((k_sum_bin_gamma<EXAML_INNER_INNER>), dim3(grid),
                       dim3(NV_BLOCK), 0, s, sum, x1, x2, tipVec, tipX1,
                       tipX2, n);
    break;
  default:
    snprintf(g_err, sizeof(g_err), "sum_bin: bad tipCase %d", tipCase);
    return -1;
  }
  CHK(hipGetLastError());
  return 0;
}

extern "C" int examl_hip_core_bin_gamma(long n, const double *sum,
                                        const double *dtab, const int *wgt,
                                        double *dev_partials, double *out2,
                                        void *stream) {
  if (n <= 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  (void)hipGetLastError(); /* clear stale per-thread error (e.g. torch probes) */
  const int grid = grid_for(n * 4);
  hipLaunchKernelGGL(k_core_bin_gamma, dim3(grid), dim3(NV_BLOCK), 0, s, sum,
                     dtab, wgt, n, dev_partials);
  CHK(hipGetLastError());
  hipLaunchKernelGGL(k_reduce_2, dim3(1), dim3(NV_BLOCK), 0, s, dev_partials,
                     grid, out2);
  CHK(hipGetLastError());
  return 0;
}
