/* ============================================================================
 * examl_prot_gamma_mseg.inc — on-chip protein GAMMA traversal over all
 * partitions.
 *
 * k_newview_prot_gamma_mseg_fused is to k_newview_prot_mseg what
 * k_newview_dna_mseg_fused is to k_newview_dna_mseg, with the design of
 * k_newview_prot_gamma_fused (examl_prot_gamma_fused.inc, whose PGF_*
 * geometry, pgf_dot, pgf_load and pgf_tip it uses): one launch runs a run of
 * traversal entries per PGF_SITES-site tile, for every partition, eight lanes
 * on a site, each child CLV handed to its parent on chip (every x3 is still
 * stored to its partition's pool).  Included by examl_hip.hip behind the
 * multi-partition handle (same flags, -ffp-contract=off).
 *
 * Entry tables.  k_newview_prot_mseg stages 3200 doubles of P in every block
 * of every (entry, partition) and rebuilds a tip child's 23 x 80 ump table
 * there.  k_prot_gamma_tables_mseg runs ahead of the fused launch, in the
 * same stream and graph, one block per (entry of the run, child, partition):
 * it writes the LDS-ready half k_prot_gamma_tables writes, from the P block
 * k_make_p_mseg left at pbuf[((base+e)*numParts+p)*3200] and the partition's
 * tipVector, into the handle's table scratch at
 *   tab[(e * numParts + p) * PGF_TAB + h * PGF_HALF],  e = entry in the run.
 * The scratch holds min(maxOps, FUSED_MAX_OPS) entries, the longest run the
 * planner emits; successive runs of a call reuse it in stream order.
 *
 * What the partition axis adds to the fused kernel:
 *   - a tile table (examl_hip_multi_tile_table at PGF_SITES) maps tile ->
 *     (partition, first site in it); tiles never straddle partitions, so a
 *     tile's 8-lane groups are whole and a tile has ONE model;
 *   - per-partition operands come from the descriptor array (MPartDesc), the
 *     scaler increment of (entry e, partition p) is inc[(base+e)*numParts+p];
 *   - sEV belongs to a partition: it is restaged when the block's tile lies
 *     in another partition than the tile sEV was staged for, behind a
 *     barrier of its own (the previous tile's last entry may still be
 *     reading it); the first barrier of the entry loop publishes it;
 *   - tiles of masked partitions (active[part] == 0) are skipped as if they
 *     were not in the table.
 * Math, summation order, rescale vote and stores are those of
 * k_newview_prot_gamma_fused, which restates k_newview_prot_gamma, whose twin
 * k_newview_prot_mseg is: with the same P block the results are bit-identical
 * to the level path, FMA and no-FMA.
 *
 * Barrier discipline (as in examl_prot_gamma_fused.inc): every barrier is
 * reached by every thread of the block.  The tile loop depends on blockIdx,
 * gridDim and numTiles only; whether a tile runs and whether sEV is restaged
 * depend on the tile table and the active flags only (block-uniform); the
 * entry loop on prog.count only; sites past the partition's width are
 * predicated off as whole 8-lane groups; there is no return/continue/break
 * inside the loops.
 * ==========================================================================*/

/* one block per (entry of the run, child, partition): the child's half of
 * the (entry, partition) table block */
template <bool FAST>
__global__ __launch_bounds__(NV_BLOCK) void k_prot_gamma_tables_mseg(
    const FusedProg prog, const MPartDesc *__restrict__ parts, int numParts,
    const double *__restrict__ pbuf, const double *__restrict__ active,
    double *__restrict__ tab) {
  __shared__ double sP[PGF_PLEN], sTV[460];
  const int tid = threadIdx.x;
  const int e = blockIdx.x, h = blockIdx.y, p = blockIdx.z;
  /* masked or empty partition (whose buffers may never have been
   * allocated): block-uniform, ahead of the barrier */
  if (active[p] == 0.0 || parts[p].n == 0) return;
  const double *P =
      pbuf + ((long)(prog.base + e) * numParts + p) * 3200 + h * 1600;
  const double *tipVec = parts[p].tipVec;
  double *out = tab + ((long)e * numParts + p) * PGF_TAB + h * PGF_HALF;
  for (int j = tid; j < PGF_PLEN; j += NV_BLOCK) {
    const int pc = j / PGF_CSTR, pr = j % PGF_CSTR;
    sP[j] = pr < 400 ? P[pc * 400 + pr] : 0.0;
  }
  for (int j = tid; j < 460; j += NV_BLOCK) sTV[j] = tipVec[j];
  __syncthreads();
  if (pgf_tip((int)(prog.ctl[e] & 3u), h)) {
    /* k_newview_prot_mseg's ump loop */
    for (int j = tid; j < 23 * 80; j += NV_BLOCK) {
      const int code = j / 80, k = j % 80;
      const int kc = k / 20, kl = k % 20;
      out[j] = dot20o<FAST>(&sTV[20 * code], &sP[kc * PGF_CSTR + kl * 20]);
    }
  } else {
    for (int j = tid; j < PGF_PLEN; j += NV_BLOCK) out[j] = sP[j];
  }
}

/* A pointer read from a descriptor is a generic one to the compiler.  The
 * partitions' buffers are device memory: saying so gets global loads and
 * stores (uniform base + lane offset) instead of flat ones, which also count
 * against the LDS wait counter. */
template <class T>
__device__ __forceinline__ T *pgm_global(T *p) {
  return (T *)(__attribute__((address_space(1))) T *)p;
}

template <bool FAST>
__global__ __launch_bounds__(PGF_BLOCK) void k_newview_prot_gamma_mseg_fused(
    const FusedProg prog, const MPartDesc *__restrict__ parts, int numParts,
    const int *__restrict__ tilePart, const long *__restrict__ tileSite0,
    int numTiles, const double *__restrict__ tab,
    unsigned int *__restrict__ inc, const double *__restrict__ active) {
  __shared__ __attribute__((aligned(16))) double sEV[400];
  __shared__ __attribute__((aligned(16))) double sT[PGF_TAB];
  __shared__ v2d sStk[PGF_STK ? PGF_STK : 1][PGF_STK ? 5 : 1]
                     [PGF_STK ? PGF_BLOCK : 1];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int cat = (tid >> 1) & 3, half = tid & 1;
  const int count = prog.count;

  int evPart = -1; /* the partition sEV holds */

  for (int t = blockIdx.x; t < numTiles; t += gridDim.x) {
    const int part = tilePart[t];
    /* block-uniform: a masked partition's tiles do nothing at all */
    if (active[part] != 0.0) {
      const MPartDesc d = parts[part];
      double *const clv = pgm_global(d.clv);
      const unsigned char *const tips = pgm_global(d.tips);
      if (part != evPart) {
        __syncthreads(); /* the previous tile's readers of sEV are done */
        const double *const EV = pgm_global(d.EV);
        for (int i = tid; i < 400; i += PGF_BLOCK) sEV[i] = EV[i];
        evPart = part;
      }
      const long site = tileSite0[t] + (tid >> 3);
      const bool live = site < d.n; /* the whole 8-lane group alike */
      /* the lane's first column of its (site, cat) row in a pool slot */
      const long col = (site * 4 + cat) * 20 + 2 * half;
      const double *ptab = tab + (long)part * PGF_TAB;
      /* previous entry's result (REG); a run's first entry never reads it,
       * so it is not carried from tile to tile */
      double rr[10];
#pragma unroll
      for (int s = 0; s < 10; s++) rr[s] = 0.0;

      for (int e = 0; e < count; e++) {
        const unsigned int ctl = prog.ctl[e];
        const int tc = (int)(ctl & 3u);
        const unsigned int k1 = (ctl >> 2) & 3u, k2 = (ctl >> 4) & 3u;

        /* ---- operands that come from memory, ahead of the barriers ---- */
        double xl[10], xr[10];
        int c1 = 0, c2 = 0;
        if (live) {
          if (tc != EXAML_INNER_INNER)
            c1 = tips[(long)prog.x1[e] * d.tipStride + site];
          else if (k1 == FSRC_MEM)
            pgf_load(xl, &clv[(long)prog.x1[e] * d.clvStride + col]);
          if (tc == EXAML_TIP_TIP)
            c2 = tips[(long)prog.x2[e] * d.tipStride + site];
          else if (k2 == FSRC_MEM)
            pgf_load(xr, &clv[(long)prog.x2[e] * d.clvStride + col]);
        }

        /* ---- the (entry, partition) table block into LDS ---- */
        __syncthreads(); /* the previous entry's readers are done; sEV */
        {
          const v2d *src = reinterpret_cast<const v2d *>(
              ptab + (long)e * numParts * PGF_TAB);
          v2d *dst = reinterpret_cast<v2d *>(sT);
          const int n0 = (pgf_tip(tc, 0) ? PGF_HALF : PGF_PLEN) / 2;
          const int n1 = (pgf_tip(tc, 1) ? PGF_HALF : PGF_PLEN) / 2;
          for (int i = tid; i < n0; i += PGF_BLOCK) dst[i] = src[i];
          for (int i = tid; i < n1; i += PGF_BLOCK)
            dst[PGF_HALF / 2 + i] = src[PGF_HALF / 2 + i];
        }
        __syncthreads();

        /* ---- entry e on the lane's (site, cat, half) ---- */
        if (live) {
          if (tc == EXAML_INNER_INNER && k1 != FSRC_MEM) {
            if (k1 == FSRC_REG) {
#pragma unroll
              for (int s = 0; s < 10; s++) xl[s] = rr[s];
            } else if (PGF_STK) {
#pragma unroll
              for (int j = 0; j < 5; j++) {
                const v2d v = sStk[(ctl >> 6) & 15u][j][tid];
                xl[2 * j] = v.x;
                xl[2 * j + 1] = v.y;
              }
            }
          }
          if (tc != EXAML_TIP_TIP && k2 != FSRC_MEM) {
            if (k2 == FSRC_REG) {
#pragma unroll
              for (int s = 0; s < 10; s++) xr[s] = rr[s];
            } else if (PGF_STK) {
#pragma unroll
              for (int j = 0; j < 5; j++) {
                const v2d v = sStk[(ctl >> 10) & 15u][j][tid];
                xr[2 * j] = v.x;
                xr[2 * j + 1] = v.y;
              }
            }
          }

          double acc[10];
#pragma unroll
          for (int s = 0; s < 10; s++) acc[s] = 0.0;
          const double *u1t = &sT[80 * c1 + cat * 20];
          const double *u2t = &sT[PGF_HALF + 80 * c2 + cat * 20];
          const double *pl = &sT[cat * PGF_CSTR + 2 * half];
          const double *pr = &sT[PGF_HALF + cat * PGF_CSTR + 2 * half];
          const double *ev = &sEV[2 * half];
          for (int l = 0; l < 20; l++) {
            const double u1 = tc == EXAML_INNER_INNER
                                  ? pgf_dot<FAST>(xl, pl + l * 20, half)
                                  : u1t[l];
            const double u2 = tc == EXAML_TIP_TIP
                                  ? u2t[l]
                                  : pgf_dot<FAST>(xr, pr + l * 20, half);
            const double tt = u1 * u2;
#pragma unroll
            for (int j = 0; j < 5; j++) {
              const v2d v =
                  *reinterpret_cast<const v2d *>(ev + l * 20 + 4 * j);
              if (FAST) {
                acc[2 * j] = fma(tt, v.x, acc[2 * j]);
                acc[2 * j + 1] = fma(tt, v.y, acc[2 * j + 1]);
              } else {
                acc[2 * j] += tt * v.x;
                acc[2 * j + 1] += tt * v.y;
              }
            }
          }

          if (tc != EXAML_TIP_TIP) {
            /* all 80 span entries below the threshold = all eight lanes of
             * the site vote small */
            bool small = true;
#pragma unroll
            for (int s = 0; s < 10; s++)
              small &= (fabs(acc[s]) < MINLIKELIHOOD);
            const unsigned long long m = __ballot(small);
            if (((m >> (lane & ~7)) & 0xFFULL) == 0xFFULL) {
#pragma unroll
              for (int s = 0; s < 10; s++) acc[s] *= TWOTOTHE256;
              if ((lane & 7) == 0)
                atomicAdd(inc + (size_t)(prog.base + e) * numParts + part,
                          (unsigned int)pgm_global(d.wgt)[site]);
            }
          }

          double *out = &clv[(long)prog.x3[e] * d.clvStride + col];
#pragma unroll
          for (int j = 0; j < 5; j++)
            *reinterpret_cast<v2d *>(out + 4 * j) =
                (v2d){acc[2 * j], acc[2 * j + 1]};
          if (PGF_STK && (ctl & (1u << 14))) {
#pragma unroll
            for (int j = 0; j < 5; j++)
              sStk[(ctl >> 16) & 15u][j][tid] =
                  (v2d){acc[2 * j], acc[2 * j + 1]};
          }
#pragma unroll
          for (int s = 0; s < 10; s++) rr[s] = acc[s];
        }
      }
    }
  }
}

/* --- host side: glue behind examl_hip_newview_traversal_multi ------------- */

/* blocks of a launch: the blocks the device holds at once */
static int multi_prot_fused_grid_cap(void) {
  static int cap = 0;
  if (cap > 0) return cap;
  int dev = 0, cus = 0, per_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                            dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(
          &per_cu, k_newview_prot_gamma_mseg_fused<false>, PGF_BLOCK, 0) !=
          hipSuccess ||
      cus < 1 || per_cu < 1) {
    (void)hipGetLastError();
    return 0;
  }
  return cap = cus * per_cu;
}

/* entries of the handle's table scratch: the longest run of the planner */
static long multi_prot_tab_entries(int maxOps) {
  return maxOps < FUSED_MAX_OPS ? maxOps : FUSED_MAX_OPS;
}

/* Tile table at PGF_SITES, partition descriptors and table scratch of a
 * 20-state handle, built once at create.  A handle with no site, too wide
 * for the table, without a device to size the grid on or whose scratch
 * cannot be allocated keeps the level path: numTiles stays 0 and nothing
 * stays allocated.  -> 0, or -1 with g_err set for a failed copy. */
static int multi_prot_fused_setup(examl_hip_multi *h) {
  const int NP = h->numParts;
  const long tiles = multi_tile_count(h->widths.data(), NP, PGF_SITES);
  if (tiles <= 0 || multi_prot_fused_grid_cap() < 1) return 0;
  std::vector<int> tpart((size_t)tiles);
  std::vector<long> tsite((size_t)tiles);
  if (examl_hip_multi_tile_table(h->widths.data(), NP, PGF_SITES,
                                 tpart.data(), tsite.data(),
                                 (int)tiles) != (int)tiles) {
    snprintf(g_err, sizeof(g_err), "multi_create: tile table");
    return -1;
  }
  std::vector<MPartDesc> desc((size_t)NP);
  for (int p = 0; p < NP; p++)
    desc[(size_t)p] = {h->clv[p],       h->clvStride[p], h->tips[p],
                       h->tipStride[p], h->wgt[p],       h->EV[p],
                       h->tipVec[p],    h->widths[p]};
  const size_t tabBytes = (size_t)multi_prot_tab_entries(h->maxOps) * NP *
                          PGF_TAB * sizeof(double);
  if (hipMalloc(&h->d_protTab, tabBytes) != hipSuccess ||
      hipMalloc(&h->d_tilePart, (size_t)tiles * sizeof(int)) != hipSuccess ||
      hipMalloc(&h->d_tileSite0, (size_t)tiles * sizeof(long)) !=
          hipSuccess ||
      hipMalloc(&h->d_parts, (size_t)NP * sizeof(MPartDesc)) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(h->d_protTab);
    (void)hipFree(h->d_tilePart);
    (void)hipFree(h->d_tileSite0);
    (void)hipFree(h->d_parts);
    h->d_protTab = nullptr;
    h->d_tilePart = nullptr;
    h->d_tileSite0 = nullptr;
    h->d_parts = nullptr;
    return 0;
  }
  hipError_t e = hipMemcpy(h->d_tilePart, tpart.data(),
                           (size_t)tiles * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(h->d_tileSite0, tsite.data(), (size_t)tiles * sizeof(long),
                  hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(h->d_parts, desc.data(), (size_t)NP * sizeof(MPartDesc),
                  hipMemcpyHostToDevice);
  if (e != hipSuccess) return set_err(e, "multi_create: prot tile table");
  h->numTiles = (int)tiles;
  return 0;
}

/* one run of >= 2 entries on a 20-state handle: its tables, then the run */
static void launch_prot_gamma_mseg_fused(const examl_hip_multi *h,
                                         const FusedProg &pg,
                                         const double *d_active,
                                         hipStream_t s) {
  const int cap = multi_prot_fused_grid_cap();
  const int grid = h->numTiles < cap ? h->numTiles : cap;
  with_flag(g_fast_math, [&](auto fast) {
    hipLaunchKernelGGL((k_prot_gamma_tables_mseg<decltype(fast)::value>),
                       dim3(pg.count, 2, h->numParts), dim3(NV_BLOCK), 0, s,
                       pg, h->d_parts, h->numParts, h->d_pbuf, d_active,
                       h->d_protTab);
    hipLaunchKernelGGL(
        (k_newview_prot_gamma_mseg_fused<decltype(fast)::value>), dim3(grid),
        dim3(PGF_BLOCK), 0, s, pg, h->d_parts, h->numParts, h->d_tilePart,
        h->d_tileSite0, h->numTiles, h->d_protTab, h->d_inc, d_active);
  });
}

extern "C" int examl_hip_multi_prot_fused_launches(void *vh) {
  return vh ? ((examl_hip_multi *)vh)->lastProtFused : 0;
}

extern "C" int examl_hip_multi_prot_fused_grid_cap(void) {
  return multi_prot_fused_grid_cap();
}
