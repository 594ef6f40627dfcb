/* ============================================================================
 * examl_prot_cat_fused.inc — on-chip protein CAT (PSR) traversal.
 *
 * k_newview_prot_cat_fused is to k_newview_prot_cat what
 * k_newview_dna_cat_fused is to k_newview_dna_cat: a run of traversal entries
 * per tile of sites, each child CLV handed to its parent on chip (every x3 is
 * still stored to the pool), operand sources MEM / REG / LDS resolved by
 * fused_plan and carried by FusedProg.  Included by examl_hip.hip below
 * examl_prot_cat_rates.inc, whose quad helper rp_from it shares (same flags,
 * -ffp-contract=off).
 *
 * Four lanes per site.  Lane j = lane & 3 of an aligned quad owns five of its
 * site's 20 states, pc_own(j, 0..4): the five doubles it loads of an inner
 * operand, the five rows l of u1/u2 it computes, the five x3[s] it
 * accumulates, rescales and stores, and its 40 bytes of a stack slot.  Per
 * entry:
 *   quad all-gather of each inner operand's 5 -> 20 (a tip operand is its
 *   sTV row, read whole by every lane) ->
 *   m[r] = dot20o<false>(a, left[cat][l]) * dot20o<false>(b, right[cat][l])
 *   for the lane's own rows l: 200 doubles of P per lane, not 800 ->
 *   quad all-gather of the 20 products -> x3[s] from 0.0 over l = 0..19 in
 *   order for the lane's own s -> rescale verdict ANDed over the quad by DPP,
 *   lane 0 of the quad does the atomicAdd.
 * These are k_newview_prot_cat's expressions one for one, so CLVs and scaler
 * counts keep their bits whichever lane computes them.  No matrix
 * instructions: an MFMA would fuse and reorder the four k-products of
 * dot20o, and fp64 MFMA is rate-equal to VALU on gfx950 (DESIGN §8).
 *
 * A tile is the block's PCATF_SITES sites (one quad each).  Once per tile the
 * block ranks the tile's sites by (category, index) in LDS and quad q takes
 * site tile_base + sOrd[q] for every entry of the run (PCATF_SORT): P stays
 * in global memory (25 categories x 800 doubles per entry do not fit LDS),
 * and a wave's 16 quads then read two or three category blocks instead of up
 * to 16, same-category lanes with the same j the same addresses.  The order
 * comes from the live cptr at every launch; nothing about a site's result
 * depends on the quad that computes it.  Sites past n rank last (category
 * MAX_CAT) and their quads do nothing.
 *
 * The operand stack is sStk[slot][quad][20]; a lane reads and writes only its
 * own five states of its own quad's row, so the stack needs no barrier, and
 * neither does an entry.  Barriers stand at the tile head only (two with the
 * ordering, one without); every thread reaches them: the tile loop depends
 * on blockIdx/gridDim only, quads past n are predicated off as a whole
 * (their four lanes together, so every DPP read stays inside active lanes),
 * and there is no return/continue/break inside the loops.  sCat is double
 * buffered by tile parity: a wave that runs ahead writes the next tile's
 * categories while a slower one may still read this tile's.
 *
 * Prefetch: the next entry's tip codes during the current entry; the next
 * tile's cptr (thread i < PCATF_SITES holds site i's) during the tile's last
 * entry.  Entry 0's tip codes are read after the ordering, which decides the
 * quad's site.
 * ==========================================================================*/

#ifndef PCATF_SITES
#define PCATF_SITES 64 /* sites per tile = quads per block (64 | 128) */
#endif
#define PCATF_BLOCK (4 * PCATF_SITES)
#ifndef PCATF_D
/* stack slots: depth x PCATF_SITES x 160 B = 40 KiB either way, which with
 * EV, tipVector and the order tables keeps three blocks of 256 threads on a
 * CU's 160 KiB */
#define PCATF_D (PCATF_SITES == 64 ? 4 : 2)
#endif
#ifndef PCATF_SORT
#define PCATF_SORT 1 /* category-ordered tile (DESIGN §7l) */
#endif
#ifndef PCATF_AHEAD
#define PCATF_AHEAD 2 /* P rows of 20 doubles in flight per lane */
#endif

static_assert(PCATF_SITES == 64 || PCATF_SITES == 128, "tile size");
static_assert(PCATF_D >= 1 && PCATF_D <= 16, "ctl holds 4-bit stack slots");
static_assert(PCATF_D * PCATF_SITES * 160 + 860 * 8 + PCATF_SITES * 12 <=
                  64 * 1024,
              "LDS of one block");

/* the r-th state (and P row) of lane j of a quad */
__device__ __forceinline__ int pc_own(int j, int r) {
  return r < 4 ? 4 * j + r : 16 + j;
}

/* quad all-gather: all[pc_own(s, r)] = lane s's mine[r] */
__device__ __forceinline__ void pc_gather(const double (&mine)[5],
                                          double (&all)[20]) {
#pragma unroll
  for (int r = 0; r < 4; r++) {
    all[r] = rp_from<0>(mine[r]);
    all[4 + r] = rp_from<1>(mine[r]);
    all[8 + r] = rp_from<2>(mine[r]);
    all[12 + r] = rp_from<3>(mine[r]);
  }
  all[16] = rp_from<0>(mine[4]);
  all[17] = rp_from<1>(mine[4]);
  all[18] = rp_from<2>(mine[4]);
  all[19] = rp_from<3>(mine[4]);
}

/* lane j's five doubles of the 20-double row at p (32-byte aligned) */
__device__ __forceinline__ void pc_load(double (&x)[5], const double *p,
                                        int j) {
  const v4d v = *reinterpret_cast<const v4d *>(p + 4 * j);
  x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  x[4] = p[16 + j];
}

__device__ __forceinline__ void pc_store(double *p, int j,
                                         const double (&x)[5]) {
  *reinterpret_cast<v4d *>(p + 4 * j) = (v4d){x[0], x[1], x[2], x[3]};
  p[16 + j] = x[4];
}

/* dot20o<false> of a with the 20-double P row at p (32-byte aligned), the
 * row fetched as five 32-byte loads */
__device__ __forceinline__ double pc_dot_row(const double (&a)[20],
                                             const double *p) {
  double row[20];
#pragma unroll
  for (int c = 0; c < 5; c++) {
    const v4d v = reinterpret_cast<const v4d *>(p)[c];
    row[4 * c] = v.x; row[4 * c + 1] = v.y;
    row[4 * c + 2] = v.z; row[4 * c + 3] = v.w;
  }
  return dot20o<false>(a, row);
}

/* lane j's five states of an inner operand by its ctl source: the previous
 * entry's result, the quad's row of a stack slot, or the pool */
__device__ __forceinline__ void pc_fetch(double (&mine)[5], unsigned int kind,
                                         const double (&reg)[5],
                                         const double *stk, const double *mem,
                                         int j) {
  if (kind == FSRC_REG) {
#pragma unroll
    for (int r = 0; r < 5; r++) mine[r] = reg[r];
  } else if (kind == FSRC_LDS) {
    pc_load(mine, stk, j);
  } else {
    pc_load(mine, mem, j);
  }
}

__global__ __launch_bounds__(PCATF_BLOCK) void k_newview_prot_cat_fused(
    const FusedProg prog, double *__restrict__ clv, long clvStride,
    const unsigned char *__restrict__ tips, long tipStride,
    const double *__restrict__ pbuf, int numCats,
    const double *__restrict__ EV, const double *__restrict__ tipVec,
    const int *__restrict__ cptr, const int *__restrict__ wgt, long n,
    unsigned int *__restrict__ scalerInc) {
  __shared__ double sEV[400], sTV[460];
  __shared__ __attribute__((aligned(32)))
  double sStk[PCATF_D][PCATF_SITES][20];
  __shared__ int sCat[2][PCATF_SITES];
#if PCATF_SORT
  __shared__ int sOrd[PCATF_SITES];
#endif

  const int tid = threadIdx.x;
  const int j = tid & 3, q = tid >> 2;
  const int count = prog.count;
  const long tiles = (n + PCATF_SITES - 1) / PCATF_SITES;
  const long pblk = (long)numCats * 800;

  for (int i = tid; i < 400; i += PCATF_BLOCK) sEV[i] = EV[i];
  for (int i = tid; i < 460; i += PCATF_BLOCK) sTV[i] = tipVec[i];
  /* thread i < PCATF_SITES: the category of site i of the block's next tile;
   * MAX_CAT past n */
  int catn = MAX_CAT;
  if (tid < PCATF_SITES) {
    const long s0 = (long)blockIdx.x * PCATF_SITES + tid;
    if (s0 < n) catn = cptr[s0];
  }
  double rr[5] = {0, 0, 0, 0, 0}; /* previous entry's result (REG) */
  int par = 0;

  for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
    /* ---- the tile's order (the first barrier also publishes sEV/sTV) ---- */
    if (tid < PCATF_SITES) sCat[par][tid] = catn;
    __syncthreads();
#if PCATF_SORT
    if (tid < PCATF_SITES) {
      /* rank of the key (category, index) among the tile's: a counting sort
       * without bins, stable and free of atomics */
      const int key = catn * PCATF_SITES + tid;
      int rank = 0;
#pragma unroll 8
      for (int k = 0; k < PCATF_SITES; k++)
        rank += (sCat[par][k] * PCATF_SITES + k) < key;
      sOrd[rank] = tid;
    }
    __syncthreads();
    const int os = sOrd[q];
#else
    const int os = q;
#endif
    const int cat = sCat[par][os];
    par ^= 1;
    const long site = t * PCATF_SITES + os;
    const bool active = site < n; /* the whole quad alike */

    int c1 = 0, c2 = 0;
    {
      const int tc0 = (int)(prog.ctl[0] & 3u);
      if (active && tc0 != EXAML_INNER_INNER)
        c1 = tips[(long)prog.x1[0] * tipStride + site];
      if (active && tc0 == EXAML_TIP_TIP)
        c2 = tips[(long)prog.x2[0] * tipStride + site];
    }

    for (int e = 0; e < count; e++) {
      const unsigned int ctl = prog.ctl[e];
      const int tc = (int)(ctl & 3u);

      /* ---- prefetch: the next entry's tip codes, or after the last entry
       * the categories of the block's next tile ---- */
      int c1n = 0, c2n = 0;
      if (e + 1 < count) {
        const int tcn = (int)(prog.ctl[e + 1] & 3u);
        if (active && tcn != EXAML_INNER_INNER)
          c1n = tips[(long)prog.x1[e + 1] * tipStride + site];
        if (active && tcn == EXAML_TIP_TIP)
          c2n = tips[(long)prog.x2[e + 1] * tipStride + site];
      } else if (tid < PCATF_SITES) {
        const long sn = (t + gridDim.x) * PCATF_SITES + tid;
        catn = sn < n ? cptr[sn] : MAX_CAT;
      }

      /* ---- entry e on the quad's site ---- */
      if (active) {
        /* EV is re-read from LDS per entry: with no barrier in this loop its
         * 100 doubles per lane would be hoisted out of it and spill */
        __asm__ volatile("" ::: "memory");
        const double *P = pbuf + (long)(prog.base + e) * pblk;
        double *row = &sStk[0][q][0];
        /* the lane's five states of each inner operand */
        double m1[5], m2[5] = {0, 0, 0, 0, 0}, a[20], b[20], d[10], m[5],
               tt[20];
        if (tc == EXAML_INNER_INNER)
          pc_fetch(m1, (ctl >> 2) & 3u, rr,
                   row + ((ctl >> 6) & 15u) * (PCATF_SITES * 20),
                   &clv[(long)prog.x1[e] * clvStride + site * 20], j);
        if (tc != EXAML_TIP_TIP)
          pc_fetch(m2, (ctl >> 4) & 3u, rr,
                   row + ((ctl >> 10) & 15u) * (PCATF_SITES * 20),
                   &clv[(long)prog.x2[e] * clvStride + site * 20], j);
        if (tc == EXAML_INNER_INNER) {
          pc_gather(m1, a);
        } else {
#pragma unroll
          for (int k = 0; k < 20; k++) a[k] = sTV[20 * c1 + k];
        }
        /* the lane's ten 20-dots, five left rows then five right ones, as a
         * chain: the offset of row k is made to wait for dot k - PCATF_AHEAD,
         * so at most that many rows are in flight.  Left alone, the compiler
         * issues the 200 doubles of an entry at once and spills them. */
#pragma unroll
        for (int k = 0; k < 10; k++) {
          long off = (k < 5 ? 0L : (long)numCats * 400) + cat * 400L +
                     pc_own(j, k % 5) * 20;
          if (k >= PCATF_AHEAD)
            __asm__ volatile("" : "+v"(off) : "v"(d[k - PCATF_AHEAD]));
          if (k == 5) {
            /* the right operand takes the left one's registers: its gather
             * waits for the last left dot */
            int c = c2;
            __asm__ volatile(""
                             : "+v"(c), "+v"(m2[0]), "+v"(m2[1]), "+v"(m2[2]),
                               "+v"(m2[3]), "+v"(m2[4])
                             : "v"(d[4]));
            if (tc == EXAML_TIP_TIP) {
#pragma unroll
              for (int i = 0; i < 20; i++) b[i] = sTV[20 * c + i];
            } else {
              pc_gather(m2, b);
            }
          }
          d[k] = pc_dot_row(k < 5 ? a : b, P + off);
        }
#pragma unroll
        for (int r = 0; r < 5; r++) m[r] = d[r] * d[5 + r];
        pc_gather(m, tt);
        /* the lane's EV columns are read once the products are there, not
         * 100 doubles ahead of them */
        int je = j;
        __asm__ volatile("" : "+v"(je) : "v"(m[4]));
        double x[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int l = 0; l < 20; l++)
#pragma unroll
          for (int r = 0; r < 5; r++)
            x[r] += tt[l] * sEV[20 * l + pc_own(je, r)];

        if (tc != EXAML_TIP_TIP) {
          int small = 1;
#pragma unroll
          for (int r = 0; r < 5; r++) small &= (fabs(x[r]) < MINLIKELIHOOD);
          /* AND over the quad: lane ^ 1 (quad_perm [1,0,3,2]), then lane ^ 2 */
          small &= __builtin_amdgcn_mov_dpp(small, 0xB1, 0xf, 0xf, true);
          small &= __builtin_amdgcn_mov_dpp(small, 0x4E, 0xf, 0xf, true);
          if (small) {
#pragma unroll
            for (int r = 0; r < 5; r++) x[r] *= TWOTOTHE256;
            if (j == 0)
              atomicAdd(scalerInc + prog.base + e, (unsigned int)wgt[site]);
          }
        }

        pc_store(&clv[(long)prog.x3[e] * clvStride + site * 20], j, x);
        if (ctl & (1u << 14))
          pc_store(row + ((ctl >> 16) & 15u) * (PCATF_SITES * 20), j, x);
#pragma unroll
        for (int r = 0; r < 5; r++) rr[r] = x[r];
      }
      c1 = c1n;
      c2 = c2n;
    }
  }
}

/* --- host side: glue behind examl_hip_newview_traversal_prot_cat ---------- */

static int prot_cat_fused_depth(void) { return PCATF_D; }

/* one run of >= 2 entries of the traversal c (P block: numCats x 800) */
static void launch_prot_cat_fused(const FusedProg &pg, const TravCall &c,
                                  int numCats) {
  const long tiles = (c.n + PCATF_SITES - 1) / PCATF_SITES;
  const int grid = (int)(tiles < FUSED_GRID_CAP ? tiles : FUSED_GRID_CAP);
  hipLaunchKernelGGL(k_newview_prot_cat_fused, dim3(grid), dim3(PCATF_BLOCK),
                     0, c.stream, pg, c.clv, c.clvStride, c.tips, c.tipStride,
                     c.pbuf, numCats, c.EV, c.tipVec, c.cptr, c.wgt, c.n,
                     c.inc);
}

extern "C" int examl_hip_prot_cat_fused_tile_sites(void) {
  return PCATF_SITES;
}

extern "C" int examl_hip_prot_cat_fused_depth(void) { return PCATF_D; }

extern "C" int examl_hip_prot_cat_fused_launches(void) {
  return g_prot_cat_fused_launches;
}
