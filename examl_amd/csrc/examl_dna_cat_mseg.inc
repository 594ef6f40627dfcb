/* ============================================================================
 * examl_dna_cat_mseg.inc — on-chip DNA PSR (CAT) traversal over ALL
 * partitions: kernel k_newview_dna_cat_mseg_fused, its host executor and the
 * examl_hip_multi_cat_* C ABI.  Included by examl_hip.hip, which provides
 * FusedProg / fused_plan / fused_build_prog, the CATF_* geometry,
 * launch_newview_dna_cat, examl_host_make_p, the tile-table builder,
 * FinMetaL / k_scaler_finalize_mseg, hostP_get and with_graph.
 *
 * The kernel joins the arithmetic and lane mapping of k_newview_dna_cat_fused
 * (one lane = one site = 4 doubles, CATF_SITES sites per tile, P rows padded
 * to CATF_PROW, operands MEM / REG / LDS by ctl) to the tile walk of
 * k_newview_dna_mseg_fused (tile table, descriptors, masked partitions,
 * at most FUSED_GRID_CAP blocks striding over the tiles).
 *
 * P in the device buffer: entry e owns one row of pRow = 32 * sum(numCats)
 * doubles; partition p's block is left[16 nc_p] | right[16 nc_p] at
 * 32 * catOff[p], catOff the prefix sum of numCats over the partitions that
 * have sites.  numCats is a per-call operand of a partition.
 *
 * LDS per block: stack FUSED_D * 256 * 32 B = 32768, P 2 * 25 * 34 * 8 =
 * 13600, EV + tipVector 2 * 640 = 1280: 47648 B, three blocks per CU.
 * EV and tipVector are double buffered like P because a block's next tile
 * may belong to another partition: the idle buffer is written while the
 * last entry of the current tile computes, and it was last read a whole
 * tile (>= 1 barrier) ago.
 *
 * Barrier rules: ONE __syncthreads per entry, reached by every thread on
 * every entry of every tile the block runs.  Which tiles a block runs
 * depends on blockIdx, gridDim, the tile table and the active flags only,
 * the entry loop on prog.count only.  Lanes past a partition's last site
 * are predicated off (`live`) for loads, stores and atomics.  No
 * return/continue/break inside the loops.  A block whose tiles are all
 * masked executes the prologue barrier and nothing else, and dereferences
 * no partition buffer.  The prefetch after a block's last tile re-reads
 * entry 0's P block of the current partition and forms no site address.
 * ==========================================================================*/

struct MCatDesc { /* one partition's operands for one call; the strides and
                   * the width are ints (checked at create): fewer SGPRs */
  double *clv;
  const unsigned char *tips;
  const int *wgt;
  const int *cptr;
  const double *EV, *tipVec;
  int clvStride, tipStride;
  int n;
  int numCats;
  int catOff; /* first category row of this partition in an entry's P row */
};

/* destination of element j of a P block (left[16 nc] | right[16 nc]) in the
 * padded LDS rows; -1 when the block has no element j */
__device__ __forceinline__ int catm_pdst(int j, int nc) {
  const int half = nc * 16;
  const int side = j >= half;
  const int jj = j - side * half;
  return j < 2 * half ? (jj >> 4) * CATF_PROW + side * 16 + (jj & 15) : -1;
}

/* Streaming stores: k_newview_dna_cat's rule per partition (n >= 262144),
 * and every partition when the launch stores more than FUSED_STREAM_BYTES
 * (streamAll).  Neither threshold has been measured for this kernel. */
#define CATM_STREAM_SITES 262144L

/* The kernel is fp64 throughout; the attribute keeps the compiler from
 * choosing gfx950's packed-fp32 forms for anything in it (device pass only:
 * the host compiler does not know the feature). */
#if defined(__HIP_DEVICE_COMPILE__)
#define CATM_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define CATM_NO_PK_F32
#endif

template <bool NT>
__global__ __launch_bounds__(NV_BLOCK) CATM_NO_PK_F32 void
k_newview_dna_cat_mseg_fused(
    const FusedProg prog, const MCatDesc *__restrict__ parts, int numParts,
    const int *__restrict__ tilePart, const long *__restrict__ tileSite0,
    int numTiles, const double *__restrict__ pbuf, long pRow,
    unsigned int *__restrict__ inc, const double *__restrict__ active,
    int streamAll) {
  __shared__ double sEV[2][16], sTV[2][64];
  __shared__ __attribute__((aligned(16))) double sP[2][MAX_CAT * CATF_PROW];
  __shared__ v2d sStk[FUSED_D][2][NV_BLOCK];

  const int tid = threadIdx.x;
  const int count = prog.count;

  /* this block's first unmasked tile */
  long t = blockIdx.x;
  while (t < numTiles && active[tilePart[t]] == 0.0) t += gridDim.x;
  const bool any = t < numTiles;
  int part = any ? tilePart[t] : 0;
  long s0 = any ? tileSite0[t] : 0;
  MCatDesc d = parts[part];

  /* stage entry 0 of that tile into the buffers 0.  A block with no tile
   * stages nothing: the descriptor it holds may be an empty partition's. */
  int c1 = 0, c2 = 0, cat = 0;
  if (any) {
    if (tid < 64) sTV[0][tid] = d.tipVec[tid];
    if (tid < 16) sEV[0][tid] = d.EV[tid];
    const double *P = pbuf + (long)prog.base * pRow + 32L * d.catOff;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int j = tid + k * NV_BLOCK;
      const int dst = catm_pdst(j, d.numCats);
      if (dst >= 0) sP[0][dst] = P[j];
    }
    const int tc0 = (int)(prog.ctl[0] & 3u);
    const long site0 = s0 + tid;
    const bool live0 = site0 < d.n;
    if (live0) cat = d.cptr[site0];
    if (tc0 != EXAML_INNER_INNER && live0)
      c1 = d.tips[(long)prog.x1[0] * d.tipStride + site0];
    if (tc0 == EXAML_TIP_TIP && live0)
      c2 = d.tips[(long)prog.x2[0] * d.tipStride + site0];
  }
  __syncthreads();

  int buf = 0, evb = 0;
  double r0 = 0, r1 = 0, r2 = 0, r3 = 0; /* previous entry's result (REG) */

  while (t < numTiles) {
    const bool nt = NT && (streamAll || d.n >= CATM_STREAM_SITES);
    for (int e = 0; e < count; e++) {
      const unsigned int ctl = prog.ctl[e];
      const int tc = (int)(ctl & 3u);

      /* ---- what comes next: entry e+1 of this tile, or entry 0 of the
       * block's next unmasked tile, possibly in another partition ---- */
      const bool last = e + 1 == count;
      const int en = last ? 0 : e + 1;
      long tn = t;
      if (last)
        do
          tn += gridDim.x;
        while (tn < numTiles && active[tilePart[tn]] == 0.0);
      const bool more = tn < numTiles;
      const int partn = (last && more) ? tilePart[tn] : part;
      const long s0n = (last && more) ? tileSite0[tn] : s0;
      const bool swap = partn != part;
      /* the next tile's site arrays and P geometry (the rest of its
       * descriptor is fetched when the block gets there) */
      const unsigned char *tipsn = d.tips;
      const int *cptrn = d.cptr;
      int tipStriden = d.tipStride, nn = d.n;
      int ncn = d.numCats, catOffn = d.catOff;
      if (swap) {
        tipsn = parts[partn].tips;
        cptrn = parts[partn].cptr;
        tipStriden = parts[partn].tipStride;
        nn = parts[partn].n;
        ncn = parts[partn].numCats;
        catOffn = parts[partn].catOff;
      }

      /* ---- prefetch: the next entry's P block and tip codes, the next
       * tile's categories, the next partition's EV / tipVector ---- */
      const int tcn = (int)(prog.ctl[en] & 3u);
      const double *Pn = pbuf + (long)(prog.base + en) * pRow + 32L * catOffn;
      double pn[4], evn = 0, tvn = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int j = tid + k * NV_BLOCK;
        pn[k] = 0;
        if (j < 32 * ncn) pn[k] = Pn[j];
      }
      if (swap) {
        if (tid < 64) tvn = parts[partn].tipVec[tid];
        if (tid < 16) evn = parts[partn].EV[tid];
      }
      int c1n = 0, c2n = 0, catn = 0;
      {
        const long siten = s0n + tid;
        const bool liven = (!last || more) && siten < nn;
        if (last && liven) catn = cptrn[siten];
        if (tcn != EXAML_INNER_INNER && liven)
          c1n = tipsn[(long)prog.x1[en] * tipStriden + siten];
        if (tcn == EXAML_TIP_TIP && liven)
          c2n = tipsn[(long)prog.x2[en] * tipStriden + siten];
      }

      /* ---- entry e on this tile: k_newview_dna_cat's expressions ---- */
      {
        const long site = s0 + tid;
        const bool live = site < d.n;
        const double *le = &sP[buf][cat * CATF_PROW];
        const double *ri = le + 16;
        const double *ev = sEV[evb];
        const double *tv = sTV[evb];
        double a[4], b[4];
        if (tc == EXAML_TIP_TIP) {
          const double *t1 = &tv[4 * c1];
          const double *t2 = &tv[4 * c2];
#pragma unroll
          for (int s = 0; s < 4; s++) {
            a[s] = t1[s];
            b[s] = t2[s];
          }
        } else {
          /* x2 is an inner operand in both remaining cases */
          const unsigned int k2 = (ctl >> 4) & 3u;
          if (k2 == FSRC_REG) {
            b[0] = r0; b[1] = r1; b[2] = r2; b[3] = r3;
          } else if (k2 == FSRC_LDS) {
            const int sl = (int)((ctl >> 10) & 15u);
            const v2d lo = sStk[sl][0][tid], hi = sStk[sl][1][tid];
            b[0] = lo.x; b[1] = lo.y; b[2] = hi.x; b[3] = hi.y;
          } else {
            double4 v = make_double4(0, 0, 0, 0);
            if (live)
              v = *reinterpret_cast<const double4 *>(
                  &d.clv[(long)prog.x2[e] * d.clvStride + site * 4]);
            b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
          }
          if (tc == EXAML_INNER_INNER) {
            const unsigned int k1 = (ctl >> 2) & 3u;
            if (k1 == FSRC_REG) {
              a[0] = r0; a[1] = r1; a[2] = r2; a[3] = r3;
            } else if (k1 == FSRC_LDS) {
              const int sl = (int)((ctl >> 6) & 15u);
              const v2d lo = sStk[sl][0][tid], hi = sStk[sl][1][tid];
              a[0] = lo.x; a[1] = lo.y; a[2] = hi.x; a[3] = hi.y;
            } else {
              double4 v = make_double4(0, 0, 0, 0);
              if (live)
                v = *reinterpret_cast<const double4 *>(
                    &d.clv[(long)prog.x1[e] * d.clvStride + site * 4]);
              a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
            }
          } else {
            const double *t1 = &tv[4 * c1];
            a[0] = t1[0]; a[1] = t1[1]; a[2] = t1[2]; a[3] = t1[3];
          }
        }

        double v0 = 0, v1 = 0, v2 = 0, v3 = 0;
#pragma unroll
        for (int l = 0; l < 4; l++) {
          const double u1 = (a[0] * le[l * 4] + a[1] * le[l * 4 + 1]) +
                            (a[2] * le[l * 4 + 2] + a[3] * le[l * 4 + 3]);
          const double u2 = (b[0] * ri[l * 4] + b[1] * ri[l * 4 + 1]) +
                            (b[2] * ri[l * 4 + 2] + b[3] * ri[l * 4 + 3]);
          const double tt = u1 * u2;
          v0 += tt * ev[l * 4 + 0];
          v1 += tt * ev[l * 4 + 1];
          v2 += tt * ev[l * 4 + 2];
          v3 += tt * ev[l * 4 + 3];
        }

        if (tc != EXAML_TIP_TIP) {
          /* the site's whole span is in this lane: a thread-local verdict */
          if (live & (fabs(v0) < MINLIKELIHOOD) & (fabs(v1) < MINLIKELIHOOD) &
              (fabs(v2) < MINLIKELIHOOD) & (fabs(v3) < MINLIKELIHOOD)) {
            v0 *= TWOTOTHE256;
            v1 *= TWOTOTHE256;
            v2 *= TWOTOTHE256;
            v3 *= TWOTOTHE256;
            /* rare: the weight array is looked up here, not kept live */
            atomicAdd(inc + (size_t)(prog.base + e) * numParts + part,
                      (unsigned int)parts[part].wgt[site]);
          }
        }

        if (live) {
          double *x3 = &d.clv[(long)prog.x3[e] * d.clvStride + site * 4];
          if (nt)
            __builtin_nontemporal_store((v4d){v0, v1, v2, v3},
                                        reinterpret_cast<v4d *>(x3));
          else
            *reinterpret_cast<double4 *>(x3) = make_double4(v0, v1, v2, v3);
        }
        if (ctl & (1u << 14)) {
          const int sl = (int)((ctl >> 16) & 15u);
          sStk[sl][0][tid] = (v2d){v0, v1};
          sStk[sl][1][tid] = (v2d){v2, v3};
        }
        r0 = v0; r1 = v1; r2 = v2; r3 = v3;
      }

      /* ---- write the next entry's staging into the other buffers (P: last
       * read before the previous barrier; EV / tipVector: a whole tile
       * ago) ---- */
      const int nb = buf ^ 1;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int dst = catm_pdst(tid + k * NV_BLOCK, ncn);
        if (dst >= 0) sP[nb][dst] = pn[k];
      }
      if (swap) {
        if (tid < 64) sTV[evb ^ 1][tid] = tvn;
        if (tid < 16) sEV[evb ^ 1][tid] = evn;
      }
      c1 = c1n;
      c2 = c2n;
      if (last) cat = catn;
      __syncthreads();
      buf = nb;
      if (swap) {
        evb ^= 1;
        d = parts[partn];
      }
      part = partn;
      s0 = s0n;
      t = tn;
    }
  }
}

/* the scaler increments of a call, cleared by a kernel so that the clear is
 * a kernel node of a captured graph */
__global__ void k_clear_u32(unsigned int *__restrict__ p, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0u;
}

/* ---------------------------------------------------------------------------
 * Root operations over ALL partitions: evaluate, sum and core of the DNA CAT
 * family as one kernel per call plus one reduction block per partition
 * (evaluateIterative / makenewzIterative / execCore partition loops,
 * evaluateGenericSpecial.c:403, makenewzGenericSpecial.c:885).
 *
 * Unit of work = (partition p, virtual block b).  Partition p of n_p sites
 * owns g_p = grid_for(n_p) consecutive units, the very grid its own engine
 * launches; a width-0 partition owns none.  The launch has sum(g_p) blocks;
 * block u reads p = unitPart[u] and b = u - unitPrefix[p] (two dependent
 * scalar loads) and runs the per-engine kernel's loop
 *   i = b * 256 + tid;  i < n_p;  i += g_p * 256
 * with the per-engine kernel's expressions, shuffle ladder and 4-wave add,
 * so partials[u] holds what block b of the engine's own launch would have
 * written and the reduction adds the same g_p numbers in the same order:
 * bit-identical by construction, wrapping partitions included.
 *
 * Barrier rules: the unit, and with it every loop bound and the early exit
 * of a masked partition, depend on blockIdx, the unit tables and the active
 * flags only.  A masked block returns before the first barrier and forms no
 * address of its partition; every thread of a live block reaches every
 * barrier; lanes past n_p run no loop iteration, so they load and store
 * nothing.
 *
 * Tables (host-made, libm exp) sit at tabs + p * CATR_TAB: numCats x 4 diag
 * doubles for evaluate, d[numCats x 4] | e1[4] | e2[4] | rptr[numCats] for
 * core.  LDS rows keep the 32-byte pitch of the per-engine kernels.
 * ------------------------------------------------------------------------ */

#define CATR_TAB (MAX_CAT * 4 + 8 + MAX_CAT) /* table doubles per partition */

struct CatrUnit {
  int p, b, g;
};

__device__ __forceinline__ CatrUnit catr_unit(
    const int *__restrict__ unitPart, const int *__restrict__ unitPrefix) {
  CatrUnit u;
  u.p = unitPart[blockIdx.x];
  const int u0 = unitPrefix[u.p];
  u.g = unitPrefix[u.p + 1] - u0;
  u.b = (int)blockIdx.x - u0;
  return u;
}

/* k_evaluate_dna_cat over all partitions */
template <bool TIP>
__global__ __launch_bounds__(NV_BLOCK) CATM_NO_PK_F32 void
k_evaluate_dna_cat_mseg(const MCatDesc *__restrict__ parts,
                        const int *__restrict__ unitPart,
                        const int *__restrict__ unitPrefix,
                        const double *__restrict__ active,
                        const double *__restrict__ tabs, int x1Slot,
                        int x2Slot, int tipSlot,
                        double *__restrict__ partials) {
  const CatrUnit u = catr_unit(unitPart, unitPrefix);
  if (active[u.p] == 0.0) return;
  __shared__ double sD[MAX_CAT * 4], sTV[TIP ? 64 : 1], sRed[NV_BLOCK / 64];
  const MCatDesc d = parts[u.p];
  const double *__restrict__ diag = tabs + (long)u.p * CATR_TAB;
  const int tid = threadIdx.x;
  for (int j = tid; j < d.numCats * 4; j += NV_BLOCK) sD[j] = diag[j];
  if (TIP && tid < 64) sTV[tid] = d.tipVec[tid];
  __syncthreads();
  const int *__restrict__ cptr = d.cptr;
  const int *__restrict__ wgt = d.wgt;
  const double *__restrict__ x2 = d.clv + (long)x2Slot * d.clvStride;
  const double *__restrict__ x1 =
      TIP ? nullptr : d.clv + (long)x1Slot * d.clvStride;
  const unsigned char *__restrict__ tipX1 =
      TIP ? d.tips + (long)tipSlot * d.tipStride : nullptr;
  const long n = d.n;
  const int lane = tid & 63;
  double acc = 0.0;
  for (long i = (long)u.b * NV_BLOCK + tid; i < n;
       i += (long)u.g * NV_BLOCK) {
    const double *dg = &sD[4 * cptr[i]];
    const double4 b = *reinterpret_cast<const double4 *>(&x2[i * 4]);
    double t0, t1;
    if (TIP) {
      const double *t = &sTV[4 * tipX1[i]];
      t0 = t[0] * b.x * dg[0] + t[2] * b.z * dg[2];
      t1 = t[1] * b.y * dg[1] + t[3] * b.w * dg[3];
    } else {
      const double4 a = *reinterpret_cast<const double4 *>(&x1[i * 4]);
      t0 = a.x * b.x * dg[0] + a.z * b.z * dg[2];
      t1 = a.y * b.y * dg[1] + a.w * b.w * dg[3];
    }
    acc += (double)wgt[i] * log(fabs(t0 + t1));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if (lane == 0) sRed[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = 0;
#pragma unroll
    for (int w = 0; w < NV_BLOCK / 64; w++) s += sRed[w];
    partials[blockIdx.x] = s;
  }
}

/* k_sum_dna_cat over all partitions, into each partition's own sum buffer */
template <int TC>
__global__ __launch_bounds__(NV_BLOCK) CATM_NO_PK_F32 void
k_sum_dna_cat_mseg(const MCatDesc *__restrict__ parts,
                   const int *__restrict__ unitPart,
                   const int *__restrict__ unitPrefix,
                   const double *__restrict__ active,
                   double *const *__restrict__ sums, int x1Slot, int x2Slot,
                   int tipSlot, int tipSlot2) {
  const CatrUnit u = catr_unit(unitPart, unitPrefix);
  if (active[u.p] == 0.0) return;
  __shared__ double sTV[64];
  const MCatDesc d = parts[u.p];
  const int tid = threadIdx.x;
  if (TC != EXAML_INNER_INNER && tid < 64) sTV[tid] = d.tipVec[tid];
  if (TC != EXAML_INNER_INNER) __syncthreads();
  double *__restrict__ sum = sums[u.p];
  const double *__restrict__ x1 =
      TC == EXAML_INNER_INNER ? d.clv + (long)x1Slot * d.clvStride : nullptr;
  const double *__restrict__ x2 =
      TC != EXAML_TIP_TIP ? d.clv + (long)x2Slot * d.clvStride : nullptr;
  const unsigned char *__restrict__ tipX1 =
      TC != EXAML_INNER_INNER ? d.tips + (long)tipSlot * d.tipStride : nullptr;
  const unsigned char *__restrict__ tipX2 =
      TC == EXAML_TIP_TIP ? d.tips + (long)tipSlot2 * d.tipStride : nullptr;
  const long n = d.n;
  for (long i = (long)u.b * NV_BLOCK + tid; i < n;
       i += (long)u.g * NV_BLOCK) {
    double4 a, b;
    if (TC == EXAML_TIP_TIP) {
      const double *t1 = &sTV[4 * tipX1[i]];
      const double *t2 = &sTV[4 * tipX2[i]];
      a = make_double4(t1[0], t1[1], t1[2], t1[3]);
      b = make_double4(t2[0], t2[1], t2[2], t2[3]);
    } else if (TC == EXAML_TIP_INNER) {
      const double *t1 = &sTV[4 * tipX1[i]];
      a = make_double4(t1[0], t1[1], t1[2], t1[3]);
      b = *reinterpret_cast<const double4 *>(&x2[i * 4]);
    } else {
      a = *reinterpret_cast<const double4 *>(&x1[i * 4]);
      b = *reinterpret_cast<const double4 *>(&x2[i * 4]);
    }
    *reinterpret_cast<double4 *>(&sum[i * 4]) =
        make_double4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
  }
}

/* k_core_dna_cat over all partitions */
__global__ __launch_bounds__(NV_BLOCK) CATM_NO_PK_F32 void
k_core_dna_cat_mseg(const MCatDesc *__restrict__ parts,
                    const int *__restrict__ unitPart,
                    const int *__restrict__ unitPrefix,
                    const double *__restrict__ active,
                    const double *__restrict__ tabs,
                    const double *const *__restrict__ sums,
                    double *__restrict__ partials) {
  const CatrUnit u = catr_unit(unitPart, unitPrefix);
  if (active[u.p] == 0.0) return;
  __shared__ double sD[MAX_CAT * 4], sE1[4], sE2[4], sRp[MAX_CAT],
      sRed[2][NV_BLOCK / 64];
  const MCatDesc d = parts[u.p];
  const double *__restrict__ dtab = tabs + (long)u.p * CATR_TAB;
  const int numCats = d.numCats;
  const int tid = threadIdx.x;
  for (int j = tid; j < numCats * 4; j += NV_BLOCK) sD[j] = dtab[j];
  if (tid < 4) {
    sE1[tid] = dtab[numCats * 4 + tid];
    sE2[tid] = dtab[numCats * 4 + 4 + tid];
  }
  for (int j = tid; j < numCats; j += NV_BLOCK)
    sRp[j] = dtab[numCats * 4 + 8 + j];
  __syncthreads();
  const double *__restrict__ sum = sums[u.p];
  const int *__restrict__ cptr = d.cptr;
  const int *__restrict__ wgt = d.wgt;
  const long n = d.n;
  const int lane = tid & 63;
  double accD1 = 0.0, accD2 = 0.0;
  for (long i = (long)u.b * NV_BLOCK + tid; i < n;
       i += (long)u.g * NV_BLOCK) {
    const int cat = cptr[i];
    const double *d1 = &sD[4 * cat];
    const double r = sRp[cat];
    const double w = (double)wgt[i];
    const double wr1 = r * w, wr2 = r * r * w;
    const double4 s4 = *reinterpret_cast<const double4 *>(&sum[i * 4]);
    const double te0 = d1[0] * s4.x, to0 = d1[1] * s4.y;
    const double te1 = d1[2] * s4.z, to1 = d1[3] * s4.w;
    const double a0 = (te0 + te1) + (to0 + to1);
    const double a1 = (te0 * sE1[0] + te1 * sE1[2]) +
                      (to0 * sE1[1] + to1 * sE1[3]);
    const double a2 = (te0 * sE2[0] + te1 * sE2[2]) +
                      (to0 * sE2[1] + to1 * sE2[3]);
    const double inv = 1.0 / fabs(a0);
    const double dl = a1 * inv, d2l = a2 * inv;
    accD1 += wr1 * dl;
    accD2 += wr2 * (d2l - dl * dl);
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
    partials[2 * blockIdx.x] = s1;
    partials[2 * blockIdx.x + 1] = s2;
  }
}

/* k_reduce_lnl per partition: block p folds its g_p partials with the
 * strided accumulate and the LDS tree of k_reduce_lnl and adds the scaler
 * undo of that partition.  The output is 0 + s, what k_reduce_lnl leaves in
 * a cleared cell; a masked partition gets the 0 alone.  (The GAMMA executors
 * own the names k_reduce_lnl_mseg / k_reduce_2_mseg, hence _cat_.) */
__global__ __launch_bounds__(NV_BLOCK) void k_reduce_lnl_cat_mseg(
    const double *__restrict__ partials, const int *__restrict__ unitPrefix,
    const double *__restrict__ active,
    unsigned int *const *__restrict__ gsArr, int pNumber, int qNumber,
    double log_minlik, double *__restrict__ lnl) {
  const int p = blockIdx.x;
  const int tid = threadIdx.x;
  if (active[p] == 0.0) {
    if (tid == 0) lnl[p] = 0.0;
    return;
  }
  __shared__ double sred[NV_BLOCK];
  const int u0 = unitPrefix[p], nblocks = unitPrefix[p + 1] - u0;
  double v = 0;
  for (int i = tid; i < nblocks; i += NV_BLOCK) v += partials[u0 + i];
  sred[tid] = v;
  __syncthreads();
  for (int off = NV_BLOCK / 2; off > 0; off >>= 1) {
    if (tid < off) sred[tid] += sred[tid + off];
    __syncthreads();
  }
  if (tid == 0) {
    const unsigned int *gs = gsArr[p];
    double s = sred[0];
    s += ((double)gs[pNumber] + (double)gs[qNumber]) * log_minlik;
    double o = 0.0;
    o += s;
    lnl[p] = o;
  }
}

/* k_reduce_2 per partition, into out[2p], out[2p + 1] */
__global__ __launch_bounds__(NV_BLOCK) void k_reduce_2_cat_mseg(
    const double *__restrict__ partials, const int *__restrict__ unitPrefix,
    const double *__restrict__ active, double *__restrict__ out) {
  const int p = blockIdx.x;
  const int tid = threadIdx.x;
  if (active[p] == 0.0) {
    if (tid < 2) out[2 * p + tid] = 0.0;
    return;
  }
  __shared__ double sred[2][NV_BLOCK];
  const int u0 = unitPrefix[p], nblocks = unitPrefix[p + 1] - u0;
  double v1 = 0, v2 = 0;
  for (int i = tid; i < nblocks; i += NV_BLOCK) {
    v1 += partials[2 * (u0 + i)];
    v2 += partials[2 * (u0 + i) + 1];
  }
  sred[0][tid] = v1;
  sred[1][tid] = v2;
  __syncthreads();
  for (int off = NV_BLOCK / 2; off > 0; off >>= 1) {
    if (tid < off) {
      sred[0][tid] += sred[0][tid + off];
      sred[1][tid] += sred[1][tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double o1 = 0.0, o2 = 0.0;
    o1 += sred[0][0];
    o2 += sred[1][0];
    out[2 * p] = o1;
    out[2 * p + 1] = o2;
  }
}

/* ---------------------------------------------------------------------------
 * Host side
 * ------------------------------------------------------------------------ */

/* P-row geometry of one call: catOff[p] = categories of the partitions in
 * front of p that have sites (an empty partition owns no P block), *pRow =
 * doubles per entry.  -1 for a malformed list or numCats outside
 * 1..maxCat on a partition that has sites.  Plain host code, no GPU call. */
extern "C" int examl_hip_multi_cat_plan(int numParts, const long *widths,
                                        const int *numCats, int maxCat,
                                        int *catOff, long *pRow) {
  if (numParts < 0 || maxCat < 1) return -1;
  int off = 0;
  for (int p = 0; p < numParts; p++) {
    if (widths[p] < 0) return -1;
    catOff[p] = off;
    if (widths[p] == 0) continue;
    if (numCats[p] < 1 || numCats[p] > maxCat) return -1;
    off += numCats[p];
  }
  *pRow = 32L * off;
  return 0;
}

/* Unit tables of the root operations, plain host code, no GPU call:
 * partition p owns g_p = grid_for(widths[p]) units (none for width 0), in
 * partition order.  prefixOut[numParts + 1] gets the running sum of g_p;
 * unitPartOut[cap] the partition of every unit (cap < 0: no unit table is
 * written).  Returns sum(g_p), or -1 before anything is written when it
 * exceeds a cap >= 0 or INT_MAX, or a width is negative. */
extern "C" long examl_hip_multi_cat_root_units(int numParts,
                                               const long *widths,
                                               int *prefixOut,
                                               int *unitPartOut, long cap) {
  if (numParts < 0) return -1;
  long total = 0;
  for (int p = 0; p < numParts; p++) {
    if (widths[p] < 0) return -1;
    total += widths[p] > 0 ? grid_for(widths[p]) : 0;
    if (total > 0x7fffffffL) return -1;
  }
  if (cap >= 0 && total > cap) return -1;
  if (cap < 0) unitPartOut = nullptr;
  long u = 0;
  for (int p = 0; p < numParts; p++) {
    prefixOut[p] = (int)u;
    const int g = widths[p] > 0 ? grid_for(widths[p]) : 0;
    for (int b = 0; unitPartOut && b < g; b++) unitPartOut[u + b] = p;
    u += g;
  }
  prefixOut[numParts] = (int)u;
  return total;
}

extern "C" int examl_hip_multi_cat_root_grid_cap(void) { return MAX_GRID; }

struct examl_hip_multi_cat {
  int numParts = 0, maxOps = 0;
  std::vector<long> widths, clvStride, tipStride;
  std::vector<double *> clv;
  std::vector<const unsigned char *> tips;
  std::vector<const int *> wgt;
  std::vector<unsigned int *> scalers;
  std::vector<const double *> EV, tipVec;
  int *d_tilePart = nullptr;
  long *d_tileSite0 = nullptr;
  int numTiles = 0;
  long totalSites = 0;
  bool anyWide = false; /* some partition streams its stores */
  unsigned int **d_gsArr = nullptr;
  unsigned int *d_inc = nullptr;
  /* per-call block, one upload: [MCatDesc x numParts | active x numParts |
   * P rows], in doubles */
  double *d_call = nullptr;
  long actOff = 0, pOff = 0, callDoubles = 0;
  int lastFused = 0;
  double lastHostPms = 0; /* host time of the last call's make_p loop */
  /* root operations: unit tables (built once), block partials (2 per unit)
   * and the per-call block, one upload:
   * [MCatDesc x numParts | active x numParts | sum pointers x numParts |
   *  tables CATR_TAB x numParts], in doubles */
  std::vector<int> unitPrefix;
  int numUnits = 0;
  int *d_unitPrefix = nullptr, *d_unitPart = nullptr;
  double *d_rootPartials = nullptr;
  double *d_root = nullptr;
  long rSumOff = 0, rTabOff = 0, rootDoubles = 0;
  int lastRoot = 0;
};

extern "C" void examl_hip_multi_cat_destroy(void *vh) {
  examl_hip_multi_cat *h = (examl_hip_multi_cat *)vh;
  if (!h) return;
  examl_hip_graphs_clear(); /* cached graphs may bind these buffers */
  hipFree(h->d_tilePart);
  hipFree(h->d_tileSite0);
  hipFree(h->d_gsArr);
  hipFree(h->d_inc);
  hipFree(h->d_call);
  hipFree(h->d_unitPrefix);
  hipFree(h->d_unitPart);
  hipFree(h->d_rootPartials);
  hipFree(h->d_root);
  delete h;
}

extern "C" int examl_hip_multi_cat_fused_launches(void *vh) {
  return vh ? ((examl_hip_multi_cat *)vh)->lastFused : 0;
}

extern "C" double examl_hip_multi_cat_host_p_ms(void *vh) {
  return vh ? ((examl_hip_multi_cat *)vh)->lastHostPms : 0.0;
}

extern "C" int examl_hip_multi_cat_create(
    int numParts, const long *widths, double *const *dev_clvs,
    const long *clvStrides, const unsigned char *const *dev_tips,
    const long *tipStrides, const int *const *dev_wgts,
    unsigned int *const *dev_scalers, const double *const *dev_EVs,
    const double *const *dev_tipVecs, int maxOps, void **out) {
  if (numParts < 1 || maxOps < 1) {
    snprintf(g_err, sizeof(g_err), "multi_cat_create: numParts %d maxOps %d",
             numParts, maxOps);
    return -1;
  }
  const long tiles = multi_tile_count(widths, numParts, CATF_SITES);
  if (tiles < 0) {
    snprintf(g_err, sizeof(g_err), "multi_cat_create: bad widths");
    return -1;
  }
  (void)hipGetLastError();
  examl_hip_multi_cat *h = new examl_hip_multi_cat();
  h->numParts = numParts;
  h->maxOps = maxOps;
  for (int p = 0; p < numParts; p++) {
    if (widths[p] > 0x7fffffffL || clvStrides[p] < 0 ||
        clvStrides[p] > 0x7fffffffL || tipStrides[p] < 0 ||
        tipStrides[p] > 0x7fffffffL) {
      delete h;
      snprintf(g_err, sizeof(g_err),
               "multi_cat_create: partition %d: width or stride past 2^31",
               p);
      return -1;
    }
    h->widths.push_back(widths[p]);
    h->clv.push_back(dev_clvs[p]);
    h->clvStride.push_back(clvStrides[p]);
    h->tips.push_back(dev_tips[p]);
    h->tipStride.push_back(tipStrides[p]);
    h->wgt.push_back(dev_wgts[p]);
    h->scalers.push_back(dev_scalers[p]);
    h->EV.push_back(dev_EVs[p]);
    h->tipVec.push_back(dev_tipVecs[p]);
    if (widths[p] >= CATM_STREAM_SITES) h->anyWide = true;
    h->totalSites += widths[p];
  }
  const long descDoubles =
      ((long)numParts * (long)sizeof(MCatDesc) + 7) / 8;
  h->actOff = descDoubles;
  h->pOff = descDoubles + numParts;
  h->callDoubles = h->pOff + (long)maxOps * numParts * MAX_CAT * 32;
  hipError_t e = hipSuccess;
#define MCHK(call)                                                           \
  do {                                                                       \
    e = (call);                                                              \
    if (e != hipSuccess) {                                                   \
      examl_hip_multi_cat_destroy(h);                                        \
      return set_err(e, #call);                                              \
    }                                                                        \
  } while (0)
  MCHK(hipMalloc(&h->d_call, (size_t)h->callDoubles * sizeof(double)));
  MCHK(hipMalloc(&h->d_inc,
                 (size_t)maxOps * numParts * sizeof(unsigned int)));
  MCHK(hipMalloc(&h->d_gsArr, (size_t)numParts * sizeof(unsigned int *)));
  MCHK(hipMemcpy(h->d_gsArr, h->scalers.data(),
                 (size_t)numParts * sizeof(unsigned int *),
                 hipMemcpyHostToDevice));
  if (tiles > 0) {
    std::vector<int> tpart((size_t)tiles);
    std::vector<long> tsite((size_t)tiles);
    h->numTiles = examl_hip_multi_tile_table(widths, numParts, CATF_SITES,
                                             tpart.data(), tsite.data(),
                                             (int)tiles);
    if (h->numTiles != (int)tiles) {
      examl_hip_multi_cat_destroy(h);
      snprintf(g_err, sizeof(g_err), "multi_cat_create: tile table");
      return -1;
    }
    MCHK(hipMalloc(&h->d_tilePart, (size_t)tiles * sizeof(int)));
    MCHK(hipMalloc(&h->d_tileSite0, (size_t)tiles * sizeof(long)));
    MCHK(hipMemcpy(h->d_tilePart, tpart.data(), (size_t)tiles * sizeof(int),
                   hipMemcpyHostToDevice));
    MCHK(hipMemcpy(h->d_tileSite0, tsite.data(),
                   (size_t)tiles * sizeof(long), hipMemcpyHostToDevice));
  }
  /* root operations */
  h->unitPrefix.assign((size_t)numParts + 1, 0);
  const long units = examl_hip_multi_cat_root_units(
      numParts, widths, h->unitPrefix.data(), nullptr, -1);
  if (units < 0) {
    examl_hip_multi_cat_destroy(h);
    snprintf(g_err, sizeof(g_err), "multi_cat_create: unit table");
    return -1;
  }
  h->numUnits = (int)units;
  h->rSumOff = h->pOff; /* descriptors | active, as in d_call */
  h->rTabOff = h->rSumOff + numParts;
  h->rootDoubles = h->rTabOff + (long)numParts * CATR_TAB;
  MCHK(hipMalloc(&h->d_root, (size_t)h->rootDoubles * sizeof(double)));
  MCHK(hipMalloc(&h->d_unitPrefix, ((size_t)numParts + 1) * sizeof(int)));
  MCHK(hipMemcpy(h->d_unitPrefix, h->unitPrefix.data(),
                 ((size_t)numParts + 1) * sizeof(int),
                 hipMemcpyHostToDevice));
  if (units > 0) {
    std::vector<int> upart((size_t)units);
    if (examl_hip_multi_cat_root_units(numParts, widths, h->unitPrefix.data(),
                                       upart.data(), units) != units) {
      examl_hip_multi_cat_destroy(h);
      snprintf(g_err, sizeof(g_err), "multi_cat_create: unit table");
      return -1;
    }
    MCHK(hipMalloc(&h->d_unitPart, (size_t)units * sizeof(int)));
    MCHK(hipMemcpy(h->d_unitPart, upart.data(), (size_t)units * sizeof(int),
                   hipMemcpyHostToDevice));
    MCHK(hipMalloc(&h->d_rootPartials, (size_t)units * 2 * sizeof(double)));
  }
#undef MCHK
  *out = h;
  return 0;
}

extern "C" int examl_hip_newview_traversal_multi_cat(
    void *vh, const examl_hip_trav_entry *ops, int numOps,
    const double *const *EIGNs, const double *const *EIs,
    const double *const *perSiteRates, const int *numCats,
    const int *const *dev_cptrs, const unsigned char *activeMask,
    const double *qzOv, const double *rzOv, void *stream) {
  examl_hip_multi_cat *h = (examl_hip_multi_cat *)vh;
  if (!h) {
    snprintf(g_err, sizeof(g_err), "traversal_multi_cat: null handle");
    return -1;
  }
  h->lastFused = 0;
  if (numOps <= 0) return 0;
  const int NP = h->numParts;
  if (numOps > h->maxOps) {
    snprintf(g_err, sizeof(g_err),
             "traversal_multi_cat: numOps %d > maxOps %d", numOps, h->maxOps);
    return -1;
  }
  std::vector<int> catOff((size_t)NP);
  long pRow = 0;
  if (examl_hip_multi_cat_plan(NP, h->widths.data(), numCats, MAX_CAT,
                               catOff.data(), &pRow) != 0) {
    snprintf(g_err, sizeof(g_err),
             "traversal_multi_cat: numCats outside 1..%d", MAX_CAT);
    return -1;
  }
  for (int e = 0; e < numOps; e++)
    if (ops[e].tipCase < EXAML_TIP_TIP || ops[e].tipCase > EXAML_INNER_INNER) {
      snprintf(g_err, sizeof(g_err), "traversal_multi_cat: bad tipCase %d",
               ops[e].tipCase);
      return -1;
    }
  hipStream_t s = (hipStream_t)stream;
  (void)hipGetLastError();

  /* planner launches; every one of them, a one-entry launch included, is
   * ONE kernel over all partitions.  Rejected lists, HIP-event profiling
   * and either switch off run the per-partition loop over the per-entry
   * kernel instead. */
  std::vector<FusedPlanOp> plan;
  std::vector<FusedProg> progs;
  std::vector<int> lens;
  const bool fused = h->numTiles > 0 && g_multi_fused && g_use_fused &&
                     !g_prof_on &&
                     fused_plan(ops, numOps, FUSED_D, FUSED_MAX_OPS, plan) > 0;
  if (fused)
    for (int e = 0, len; e < numOps; e += len) {
      len = 1;
      while (e + len < numOps &&
             plan[(size_t)(e + len)].launch == plan[(size_t)e].launch)
        len++;
      progs.emplace_back();
      fused_build_prog(ops, plan, e, len, &progs.back());
      lens.push_back(len);
    }
  h->lastFused = (int)progs.size();
  std::vector<int> level;
  const int numLevels = trav_levels(ops, numOps, level);

  /* pinned stage = the device block: descriptors, active flags, P rows
   * (newviewGenericSpecial.c:982-1044 per partition, libm exp) */
  HostPSlot *slot = hostP_get(h->d_call, (size_t)h->callDoubles);
  double *st = slot->buf;
  MCatDesc *desc = reinterpret_cast<MCatDesc *>(st);
  std::vector<unsigned char> live((size_t)NP);
  for (int p = 0; p < NP; p++) {
    live[(size_t)p] = h->widths[p] > 0 && (!activeMask || activeMask[p]);
    desc[p] = {h->clv[p], h->tips[p], h->wgt[p], dev_cptrs[p], h->EV[p],
               h->tipVec[p], (int)h->clvStride[p], (int)h->tipStride[p],
               (int)h->widths[p], h->widths[p] > 0 ? numCats[p] : 0,
               catOff[(size_t)p]};
    st[h->actOff + p] = live[(size_t)p] ? 1.0 : 0.0;
  }
  double *hostP = st + h->pOff;
  const auto tp0 = std::chrono::steady_clock::now();
  for (int e = 0; e < numOps; e++)
    for (int p = 0; p < NP; p++) {
      if (!live[(size_t)p]) continue;
      double qz = qzOv ? qzOv[(size_t)e * NP + p] : ops[e].qz;
      double rz = rzOv ? rzOv[(size_t)e * NP + p] : ops[e].rz;
      qz = (qz > ZMIN) ? log(qz) : log(ZMIN);
      rz = (rz > ZMIN) ? log(rz) : log(ZMIN);
      double *blk = hostP + (size_t)e * pRow + 32L * catOff[(size_t)p];
      examl_host_make_p(qz, rz, perSiteRates[p], EIs[p], EIGNs[p], numCats[p],
                        blk, blk + 16L * numCats[p], 4);
    }
  h->lastHostPms = std::chrono::duration<double, std::milli>(
                       std::chrono::steady_clock::now() - tp0)
                       .count();

  /* graph key: the list, the handle, the path, and everything a captured
   * launch or copy binds by value: P row geometry, masks (the loop path
   * launches per active partition) and the category arrays */
  const bool want_graph =
      g_use_graphs && !g_prof_on && s != nullptr && numOps >= 8;
  unsigned long long key = 0;
  if (want_graph) {
    key = trav_key(ops, numOps, h->totalSites, h, h->d_tilePart, h->d_call,
                   nullptr, nullptr, nullptr, h->d_gsArr, h->d_inc, (void *)s,
                   2000 + (fused ? 1 : 0));
    for (int p = 0; p < NP; p++) {
      key = (key ^ (unsigned long long)(uintptr_t)dev_cptrs[p]) *
            1099511628211ULL;
      key = (key ^ (unsigned long long)(desc[p].numCats * 2 +
                                        live[(size_t)p])) *
            1099511628211ULL;
    }
  }

  const double *d_active = h->d_call + h->actOff;
  const double *d_P = h->d_call + h->pOff;
  const MCatDesc *d_parts = reinterpret_cast<const MCatDesc *>(h->d_call);
  return with_graph(key, want_graph, s, [&]() -> int {
    hipError_t err = hipMemcpyAsync(
        h->d_call, st, (size_t)(h->pOff + numOps * pRow) * sizeof(double),
        hipMemcpyHostToDevice, s);
    if (err != hipSuccess) return set_err(err, "multi_cat upload");
    (void)hipEventRecord(slot->ev, s);
    slot->ev_valid = true;
    const long nInc = (long)numOps * NP;
    hipLaunchKernelGGL(k_clear_u32, dim3((unsigned)((nInc + 255) / 256)),
                       dim3(256), 0, s, h->d_inc, nInc);
    err = hipGetLastError();
    if (err != hipSuccess) return set_err(err, "multi_cat inc clear");

    if (fused) {
      /* stream order carries the dependencies between launches */
      const int fgrid =
          h->numTiles < FUSED_GRID_CAP ? h->numTiles : FUSED_GRID_CAP;
      for (size_t i = 0; i < progs.size(); i++) {
        /* bytes this launch stores: len CLVs of 4 doubles per site */
        const int streamAll =
            (long)lens[i] * h->totalSites * 32 > FUSED_STREAM_BYTES;
        with_flag(streamAll || h->anyWide, [&](auto ntc) {
          hipLaunchKernelGGL(
              (k_newview_dna_cat_mseg_fused<decltype(ntc)::value>),
              dim3(fgrid), dim3(NV_BLOCK), 0, s, progs[i], d_parts, NP,
              h->d_tilePart, h->d_tileSite0, h->numTiles, d_P, pRow, h->d_inc,
              d_active, streamAll);
        });
        err = hipGetLastError();
        if (err != hipSuccess) return set_err(err, "multi_cat fused launch");
      }
    } else {
      /* the per-partition loop (newviewIterative's, :939) */
      for (int p = 0; p < NP; p++) {
        if (!live[(size_t)p]) continue;
        for (int e = 0; e < numOps; e++) {
          TravOperands o;
          if (trav_operands(ops[e].tipCase, ops[e].x1Slot, ops[e].x2Slot,
                            h->clv[p], h->clvStride[p], h->tips[p],
                            h->tipStride[p], "traversal_multi_cat", &o) != 0)
            return -1;
          launch_newview_dna_cat(
              ops[e].tipCase, s, h->EV[p], dev_cptrs[p], o.x1, o.x2,
              h->clv[p] + (long)ops[e].x3Slot * h->clvStride[p], h->tipVec[p],
              o.t1, o.t2, h->wgt[p], h->widths[p],
              d_P + (size_t)e * pRow + 32L * catOff[(size_t)p], numCats[p],
              h->d_inc + (size_t)e * NP + p);
          err = hipGetLastError();
          if (err != hipSuccess) return set_err(err, "multi_cat loop launch");
        }
      }
    }

    /* recursive scaler accumulation per partition
     * (newviewGenericSpecial.c:1503) */
    for (int base = 0; base < numOps; base += FIN_CHUNK) {
      FinMetaL m;
      m.count = (numOps - base < FIN_CHUNK) ? (numOps - base) : FIN_CHUNK;
      m.base = base;
      m.numLevels = numLevels;
      for (int e = 0; e < m.count; e++) {
        m.p[e] = ops[base + e].pNumber;
        m.q[e] = ops[base + e].qNumber;
        m.r[e] = ops[base + e].rNumber;
        m.lvl[e] = (short)level[(size_t)(base + e)];
      }
      hipLaunchKernelGGL(k_scaler_finalize_mseg, dim3(NP), dim3(64), 0, s, m,
                         h->d_inc, NP, h->d_gsArr, d_active);
      err = hipGetLastError();
      if (err != hipSuccess) return set_err(err, "multi_cat finalize");
    }
    return 0;
  });
}

/* ---------------------------------------------------------------------------
 * Root operations: host executors
 * ------------------------------------------------------------------------ */

extern "C" int examl_hip_multi_cat_root_kernels(void *vh) {
  return vh ? ((examl_hip_multi_cat *)vh)->lastRoot : 0;
}

/* Checks a call's categories and fills the descriptors and active flags of
 * the pinned stage of d_root; hostP_get waits for the stage's previous copy
 * first.  live[p] = the partition has sites and is not masked. */
static HostPSlot *catr_stage(examl_hip_multi_cat *h, const char *who,
                             const int *numCats, const int *const *dev_cptrs,
                             const unsigned char *activeMask,
                             std::vector<unsigned char> &live) {
  const int NP = h->numParts;
  std::vector<int> catOff((size_t)NP);
  long pRow = 0;
  if (examl_hip_multi_cat_plan(NP, h->widths.data(), numCats, MAX_CAT,
                               catOff.data(), &pRow) != 0) {
    snprintf(g_err, sizeof(g_err), "%s: numCats outside 1..%d", who, MAX_CAT);
    return nullptr;
  }
  HostPSlot *slot = hostP_get(h->d_root, (size_t)h->rootDoubles);
  MCatDesc *desc = reinterpret_cast<MCatDesc *>(slot->buf);
  live.assign((size_t)NP, 0);
  for (int p = 0; p < NP; p++) {
    live[(size_t)p] = h->widths[p] > 0 && (!activeMask || activeMask[p]);
    desc[p] = {h->clv[p], h->tips[p], h->wgt[p], dev_cptrs[p], h->EV[p],
               h->tipVec[p], (int)h->clvStride[p], (int)h->tipStride[p],
               (int)h->widths[p], h->widths[p] > 0 ? numCats[p] : 0,
               catOff[(size_t)p]};
    slot->buf[h->actOff + p] = live[(size_t)p] ? 1.0 : 0.0;
  }
  return slot;
}

/* the ONE copy of a call: the first `doubles` of the stage */
static int catr_upload(examl_hip_multi_cat *h, HostPSlot *slot, long doubles,
                       hipStream_t s) {
  hipError_t err =
      hipMemcpyAsync(h->d_root, slot->buf, (size_t)doubles * sizeof(double),
                     hipMemcpyHostToDevice, s);
  if (err != hipSuccess) return set_err(err, "multi_cat root upload");
  (void)hipEventRecord(slot->ev, s);
  slot->ev_valid = true;
  return 0;
}

/* a live partition without a sum buffer is refused before anything runs */
static bool catr_null_sum(const examl_hip_multi_cat *h, const char *who,
                          double *const *dev_sums,
                          const std::vector<unsigned char> &live) {
  for (int p = 0; p < h->numParts; p++)
    if (live[(size_t)p] && !dev_sums[p]) {
      snprintf(g_err, sizeof(g_err), "%s: partition %d has no sum buffer",
               who, p);
      return true;
    }
  return false;
}

static bool catr_fused(const examl_hip_multi_cat *h) {
  return h->numUnits > 0 && g_multi_fused && g_use_fused;
}

/* the loop path accumulates into its outputs like the engines' kernels */
static int catr_clear(double *dev, int doubles, hipStream_t s) {
  hipLaunchKernelGGL(k_clear_u32, dim3((unsigned)((2 * doubles + 255) / 256)),
                     dim3(256), 0, s, (unsigned int *)dev, 2L * doubles);
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : set_err(err, "multi_cat root clear");
}

extern "C" int examl_hip_evaluate_root_multi_cat(
    void *vh, int rootTipCase, int pNumber, int qNumber, int x1Slot,
    int x2Slot, int tipSlot, const double *zs, const double *const *EIGNs,
    const double *const *perSiteRates, const int *numCats,
    const int *const *dev_cptrs, const unsigned char *activeMask,
    double *dev_lnl, void *stream) {
  examl_hip_multi_cat *h = (examl_hip_multi_cat *)vh;
  if (!h) {
    snprintf(g_err, sizeof(g_err), "evaluate_root_multi_cat: null handle");
    return -1;
  }
  h->lastRoot = 0;
  if (rootTipCase != EXAML_TIP_INNER && rootTipCase != EXAML_INNER_INNER) {
    snprintf(g_err, sizeof(g_err), "evaluate_root_multi_cat: bad tipCase %d",
             rootTipCase);
    return -1;
  }
  const int NP = h->numParts;
  std::vector<unsigned char> live;
  HostPSlot *slot = catr_stage(h, "evaluate_root_multi_cat", numCats,
                               dev_cptrs, activeMask, live);
  if (!slot) return -1;
  hipStream_t s = (hipStream_t)stream;
  (void)hipGetLastError();
  double *d_tabs = h->d_root + h->rTabOff;

  if (!catr_fused(h)) {
    /* evaluateIterative's partition loop over the per-engine launches */
    if (catr_clear(dev_lnl, NP, s) != 0) return -1;
    for (int p = 0; p < NP; p++) {
      if (!live[(size_t)p]) continue;
      if (examl_hip_evaluate_root_dna_cat_x(
              rootTipCase, pNumber, qNumber, x1Slot, x2Slot, tipSlot, zs[p],
              EIGNs[p], perSiteRates[p], numCats[p], h->tipVec[p],
              dev_cptrs[p], h->clv[p], h->clvStride[p], h->tips[p],
              h->tipStride[p], h->wgt[p], h->widths[p], h->scalers[p],
              d_tabs + (long)p * CATR_TAB,
              h->d_rootPartials + h->unitPrefix[(size_t)p], dev_lnl + p,
              stream) != 0)
        return -1;
    }
    return 0;
  }

  for (int p = 0; p < NP; p++)
    if (live[(size_t)p])
      examl_host_calc_diagptable(
          zs[p], 4, numCats[p], perSiteRates[p], EIGNs[p],
          slot->buf + h->rTabOff + (long)p * CATR_TAB);
  if (catr_upload(h, slot, h->rootDoubles, s) != 0) return -1;
  const MCatDesc *d_parts = reinterpret_cast<const MCatDesc *>(h->d_root);
  const double *d_active = h->d_root + h->actOff;
  with_flag(rootTipCase == EXAML_TIP_INNER, [&](auto tip) {
    hipLaunchKernelGGL((k_evaluate_dna_cat_mseg<decltype(tip)::value>),
                       dim3(h->numUnits), dim3(NV_BLOCK), 0, s, d_parts,
                       h->d_unitPart, h->d_unitPrefix, d_active, d_tabs,
                       x1Slot, x2Slot, tipSlot, h->d_rootPartials);
  });
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_err(err, "multi_cat evaluate launch");
  hipLaunchKernelGGL(k_reduce_lnl_cat_mseg, dim3(NP), dim3(NV_BLOCK), 0, s,
                     h->d_rootPartials, h->d_unitPrefix, d_active, h->d_gsArr,
                     pNumber, qNumber, log(MINLIKELIHOOD), dev_lnl);
  err = hipGetLastError();
  if (err != hipSuccess) return set_err(err, "multi_cat evaluate reduce");
  h->lastRoot = 1;
  return 0;
}

extern "C" int examl_hip_sum_root_multi_cat(
    void *vh, int rootTipCase, int x1Slot, int x2Slot, int tipSlot,
    int tipSlot2, const int *numCats, const int *const *dev_cptrs,
    double *const *dev_sums, const unsigned char *activeMask, void *stream) {
  examl_hip_multi_cat *h = (examl_hip_multi_cat *)vh;
  if (!h) {
    snprintf(g_err, sizeof(g_err), "sum_root_multi_cat: null handle");
    return -1;
  }
  h->lastRoot = 0;
  if (rootTipCase < EXAML_TIP_TIP || rootTipCase > EXAML_INNER_INNER) {
    snprintf(g_err, sizeof(g_err), "sum_root_multi_cat: bad tipCase %d",
             rootTipCase);
    return -1;
  }
  const int NP = h->numParts;
  std::vector<unsigned char> live;
  HostPSlot *slot = catr_stage(h, "sum_root_multi_cat", numCats, dev_cptrs,
                               activeMask, live);
  if (!slot) return -1;
  if (catr_null_sum(h, "sum_root_multi_cat", dev_sums, live)) return -1;
  hipStream_t s = (hipStream_t)stream;
  (void)hipGetLastError();

  if (!catr_fused(h)) {
    for (int p = 0; p < NP; p++) {
      if (!live[(size_t)p]) continue;
      if (examl_hip_sum_root_dna_cat(rootTipCase, x1Slot, x2Slot, tipSlot,
                                     tipSlot2, h->tipVec[p], h->clv[p],
                                     h->clvStride[p], h->tips[p],
                                     h->tipStride[p], dev_sums[p],
                                     h->widths[p], stream) != 0)
        return -1;
    }
    return 0;
  }

  memcpy(slot->buf + h->rSumOff, dev_sums, (size_t)NP * sizeof(double *));
  if (catr_upload(h, slot, h->rTabOff, s) != 0) return -1;
  const MCatDesc *d_parts = reinterpret_cast<const MCatDesc *>(h->d_root);
  const double *d_active = h->d_root + h->actOff;
  double *const *d_sums =
      reinterpret_cast<double *const *>(h->d_root + h->rSumOff);
#define CATR_SUM(TC)                                                         \
  hipLaunchKernelGGL((k_sum_dna_cat_mseg<TC>), dim3(h->numUnits),            \
                     dim3(NV_BLOCK), 0, s, d_parts, h->d_unitPart,           \
                     h->d_unitPrefix, d_active, d_sums, x1Slot, x2Slot,      \
                     tipSlot, tipSlot2)
  switch (rootTipCase) {
  case EXAML_TIP_TIP: CATR_SUM(EXAML_TIP_TIP); break;
  case EXAML_TIP_INNER: CATR_SUM(EXAML_TIP_INNER); break;
  default: CATR_SUM(EXAML_INNER_INNER);
  }
#undef CATR_SUM
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_err(err, "multi_cat sum launch");
  h->lastRoot = 1;
  return 0;
}

extern "C" int examl_hip_core_root_multi_cat(
    void *vh, const double *lzs, const double *const *EIGNs,
    const double *const *perSiteRates, const int *numCats,
    const int *const *dev_cptrs, double *const *dev_sums,
    const unsigned char *activeMask, double *dev_out2, void *stream) {
  examl_hip_multi_cat *h = (examl_hip_multi_cat *)vh;
  if (!h) {
    snprintf(g_err, sizeof(g_err), "core_root_multi_cat: null handle");
    return -1;
  }
  h->lastRoot = 0;
  const int NP = h->numParts;
  std::vector<unsigned char> live;
  HostPSlot *slot = catr_stage(h, "core_root_multi_cat", numCats, dev_cptrs,
                               activeMask, live);
  if (!slot) return -1;
  if (catr_null_sum(h, "core_root_multi_cat", dev_sums, live)) return -1;
  hipStream_t s = (hipStream_t)stream;
  (void)hipGetLastError();
  double *d_tabs = h->d_root + h->rTabOff;

  if (!catr_fused(h)) {
    /* execCore's partition loop over the per-engine launches */
    if (catr_clear(dev_out2, 2 * NP, s) != 0) return -1;
    for (int p = 0; p < NP; p++) {
      if (!live[(size_t)p]) continue;
      if (examl_hip_core_root_dna_cat(
              h->widths[p], dev_sums[p], EIGNs[p], perSiteRates[p],
              numCats[p], lzs[p], h->wgt[p], dev_cptrs[p],
              d_tabs + (long)p * CATR_TAB,
              h->d_rootPartials + 2L * h->unitPrefix[(size_t)p],
              dev_out2 + 2 * p, stream) != 0)
        return -1;
    }
    return 0;
  }

  for (int p = 0; p < NP; p++)
    if (live[(size_t)p])
      examl_host_core_dtables_dna_cat(
          EIGNs[p], perSiteRates[p], numCats[p], lzs[p],
          slot->buf + h->rTabOff + (long)p * CATR_TAB);
  memcpy(slot->buf + h->rSumOff, dev_sums, (size_t)NP * sizeof(double *));
  if (catr_upload(h, slot, h->rootDoubles, s) != 0) return -1;
  const MCatDesc *d_parts = reinterpret_cast<const MCatDesc *>(h->d_root);
  const double *d_active = h->d_root + h->actOff;
  const double *const *d_sums =
      reinterpret_cast<const double *const *>(h->d_root + h->rSumOff);
  hipLaunchKernelGGL(k_core_dna_cat_mseg, dim3(h->numUnits), dim3(NV_BLOCK),
                     0, s, d_parts, h->d_unitPart, h->d_unitPrefix, d_active,
                     d_tabs, d_sums, h->d_rootPartials);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_err(err, "multi_cat core launch");
  hipLaunchKernelGGL(k_reduce_2_cat_mseg, dim3(NP), dim3(NV_BLOCK), 0, s,
                     h->d_rootPartials, h->d_unitPrefix, d_active, dev_out2);
  err = hipGetLastError();
  if (err != hipSuccess) return set_err(err, "multi_cat core reduce");
  h->lastRoot = 1;
  return 0;
}
