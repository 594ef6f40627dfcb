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
