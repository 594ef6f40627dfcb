/* ============================================================================
 * examl_prot_gamma_fused.inc — on-chip protein GAMMA traversal.
 *
 * k_newview_prot_gamma_fused is to k_newview_prot_gamma what
 * k_newview_prot_cat_fused is to k_newview_prot_cat: a run of traversal
 * entries per tile of sites, each child CLV handed to its parent on chip
 * (every x3 is still stored to the pool), operand sources MEM / REG / LDS
 * resolved by fused_plan and carried by FusedProg.  Included by
 * examl_hip.hip (same flags, -ffp-contract=off).
 *
 * Entry tables.  k_newview_prot_gamma stages 2 x 1600 doubles of P in every
 * block of every entry and, for a tip child, rebuilds that child's 23 x 80
 * ump table in every block.  Here k_prot_gamma_tables runs ahead of the
 * fused launch, in the same stream and graph, one block per (entry, child):
 * it writes one LDS-ready block of 2 x PGF_HALF doubles per entry into device
 * scratch, half 0 for the left child, half 1 for the right one:
 *   inner child: its P half with the cat stride padded to 404 (1616 doubles);
 *   tip child:   ump[code][cat * 20 + l] = dot20o<FAST>(tipVec[code], P row),
 *                the expression and the LDS operands of the per-entry kernel,
 *                so the same bits (1840 doubles).
 * The fused kernel copies an entry's block into LDS as it is.
 *
 * Eight lanes per site, for all three tip cases: lane & 7 = cat * 2 + half,
 * the split-lane mapping of k_newview_prot_gamma's INNER_INNER branch.  A
 * lane owns the states c = 4j + 2 * half + {0, 1}, j = 0..4, of its
 * (site, cat): the ten doubles it loads of an inner operand (five 16-byte
 * loads), the two accumulator chains of each 20-dot it computes (joined with
 * the other half by one __shfl_xor in the order (t0 + t1) + (t2 + t3)), AND
 * the ten x3[s] it accumulates from 0.0 over l = 0..19, rescales and stores.
 * The per-entry kernel gives a lane the states half * 10 + s instead; x3[s]
 * depends on s alone, so the bits are the same, and with one ownership for
 * operand and result a REG or LDS operand needs no exchange between lanes.
 * A tip child's u is the lookup ump[code][cat * 20 + l], the same for both
 * halves.  Rescale: ballot over the site's eight lanes, lane 0 of the group
 * adds wgt[site] to the entry's scalerInc.  No matrix instructions (§7l).
 *
 * A tile is the block's PGF_SITES sites.  Tile loop outside, entry loop
 * inside, persistent grid: blocks-per-CU x CUs blocks stride over the tiles
 * (examl_hip_prot_gamma_fused_grid_cap).  EV is staged once per block.  Per
 * (tile, entry) there are two barriers: one before the entry's table block
 * overwrites the previous one in LDS, one after.  Every thread reaches both:
 * the tile loop depends on blockIdx/gridDim only, the entry loop on
 * prog.count only, sites past n are predicated off as whole 8-lane groups
 * (so shuffles and ballots stay inside active lanes), and there is no
 * return/continue/break inside the loops.  The pool loads of MEM operands
 * and the tip codes are issued ahead of the barriers.
 *
 * The operand stack is sStk[slot][j][thread] (16 bytes each): a lane reads
 * and writes only its own ten doubles, so the stack needs no barrier.  With
 * PGF_D == 1 the planner takes an operand on chip only from the previous
 * entry (REG), and the stack takes no LDS at all.
 * ==========================================================================*/

#ifndef PGF_SITES
#define PGF_SITES 32 /* sites per tile; 8 lanes each */
#endif
#define PGF_BLOCK (8 * PGF_SITES)
#ifndef PGF_D
/* stack slots handed to fused_plan.  1: an operand comes on chip from the
 * previous entry only, more launches, no LDS for the stack, three blocks on
 * a CU by registers; 2 and 3 take 40 and 60 KiB more LDS, leave two and one
 * block on a CU and measured slower than the per-entry kernel (DESIGN §7m) */
#define PGF_D 1
#endif
#define PGF_CSTR 404                /* padded cat stride of a P half */
#define PGF_PLEN (4 * PGF_CSTR)     /* doubles of a padded P half */
#define PGF_HALF 1840               /* doubles per child: 23 x 80 ump */
#define PGF_TAB (2 * PGF_HALF)      /* doubles per entry */
#define PGF_STK (PGF_D > 1 ? PGF_D : 0) /* slots that take LDS */

static_assert(PGF_SITES == 16 || PGF_SITES == 32 || PGF_SITES == 64,
              "tile size");
static_assert(PGF_D >= 1 && PGF_D <= 16, "ctl holds 4-bit stack slots");
static_assert(PGF_PLEN <= PGF_HALF && PGF_PLEN % 2 == 0 && PGF_HALF % 2 == 0,
              "table halves are copied as 16-byte pairs");
static_assert((PGF_TAB + 400) * 8 + PGF_STK * PGF_BLOCK * 80 <= 160 * 1024,
              "LDS of one block");

/* is child h (0 left, 1 right) of an entry with this tipCase a tip? */
__device__ __forceinline__ bool pgf_tip(int tc, int h) {
  return h == 0 ? tc != EXAML_INNER_INNER : tc == EXAML_TIP_TIP;
}

/* one block per (entry of the run, child): the child's half of the entry's
 * table block */
template <bool FAST>
__global__ __launch_bounds__(NV_BLOCK) void k_prot_gamma_tables(
    const FusedProg prog, const double *__restrict__ pbuf,
    const double *__restrict__ tipVec, double *__restrict__ tab) {
  __shared__ double sP[PGF_PLEN], sTV[460];
  const int tid = threadIdx.x;
  const int e = blockIdx.x, h = blockIdx.y;
  const double *P = pbuf + (long)(prog.base + e) * 3200 + h * 1600;
  double *out = tab + (long)(prog.base + e) * PGF_TAB + h * PGF_HALF;
  for (int j = tid; j < PGF_PLEN; j += NV_BLOCK) {
    const int pc = j / PGF_CSTR, pr = j % PGF_CSTR;
    sP[j] = pr < 400 ? P[pc * 400 + pr] : 0.0;
  }
  for (int j = tid; j < 460; j += NV_BLOCK) sTV[j] = tipVec[j];
  __syncthreads();
  if (pgf_tip((int)(prog.ctl[e] & 3u), h)) {
    /* k_newview_prot_gamma's ump loop */
    for (int j = tid; j < 23 * 80; j += NV_BLOCK) {
      const int code = j / 80, k = j % 80;
      const int kc = k / 20, kl = k % 20;
      out[j] = dot20o<FAST>(&sTV[20 * code], &sP[kc * PGF_CSTR + kl * 20]);
    }
  } else {
    for (int j = tid; j < PGF_PLEN; j += NV_BLOCK) out[j] = sP[j];
  }
}

/* the lane's two accumulator chains of the 20-dot of x with the P row at pr
 * (its first own column), joined with the other half of the lane pair in
 * dot20o's order */
template <bool FAST>
__device__ __forceinline__ double pgf_dot(const double (&x)[10],
                                          const double *pr, int half) {
  double te = 0, to = 0;
#pragma unroll
  for (int j = 0; j < 5; j++) {
    const v2d p = *reinterpret_cast<const v2d *>(pr + 4 * j);
    if (FAST) {
      te = fma(x[2 * j], p.x, te);
      to = fma(x[2 * j + 1], p.y, to);
    } else {
      te += x[2 * j] * p.x;
      to += x[2 * j + 1] * p.y;
    }
  }
  const double mine = te + to;
  const double other = __shfl_xor(mine, 1);
  return half ? (other + mine) : (mine + other);
}

/* the lane's ten doubles of the 20-double (site, cat) row at p: columns
 * 4j + 2 * half + {0, 1}; p points at column 2 * half */
__device__ __forceinline__ void pgf_load(double (&x)[10], const double *p) {
#pragma unroll
  for (int j = 0; j < 5; j++) {
    const v2d v = *reinterpret_cast<const v2d *>(p + 4 * j);
    x[2 * j] = v.x;
    x[2 * j + 1] = v.y;
  }
}

template <bool FAST>
__global__ __launch_bounds__(PGF_BLOCK) void k_newview_prot_gamma_fused(
    const FusedProg prog, double *__restrict__ clv, long clvStride,
    const unsigned char *__restrict__ tips, long tipStride,
    const double *__restrict__ tab, const double *__restrict__ EV,
    const int *__restrict__ wgt, long n,
    unsigned int *__restrict__ scalerInc) {
  __shared__ __attribute__((aligned(16))) double sEV[400];
  __shared__ __attribute__((aligned(16))) double sT[PGF_TAB];
  __shared__ v2d sStk[PGF_STK ? PGF_STK : 1][PGF_STK ? 5 : 1]
                     [PGF_STK ? PGF_BLOCK : 1];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int cat = (tid >> 1) & 3, half = tid & 1;
  const int count = prog.count;
  const long tiles = (n + PGF_SITES - 1) / PGF_SITES;

  for (int i = tid; i < 400; i += PGF_BLOCK) sEV[i] = EV[i];
  double rr[10]; /* previous entry's result (REG) */
#pragma unroll
  for (int s = 0; s < 10; s++) rr[s] = 0.0;

  for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long site = t * PGF_SITES + (tid >> 3);
    const bool active = site < n; /* the whole 8-lane group alike */
    /* the lane's first column of its (site, cat) row in a pool slot */
    const long col = (site * 4 + cat) * 20 + 2 * half;

    for (int e = 0; e < count; e++) {
      const unsigned int ctl = prog.ctl[e];
      const int tc = (int)(ctl & 3u);
      const unsigned int k1 = (ctl >> 2) & 3u, k2 = (ctl >> 4) & 3u;

      /* ---- operands that come from memory, ahead of the barriers ---- */
      double xl[10], xr[10];
      int c1 = 0, c2 = 0;
      if (active) {
        if (tc != EXAML_INNER_INNER)
          c1 = tips[(long)prog.x1[e] * tipStride + site];
        else if (k1 == FSRC_MEM)
          pgf_load(xl, &clv[(long)prog.x1[e] * clvStride + col]);
        if (tc == EXAML_TIP_TIP)
          c2 = tips[(long)prog.x2[e] * tipStride + site];
        else if (k2 == FSRC_MEM)
          pgf_load(xr, &clv[(long)prog.x2[e] * clvStride + col]);
      }

      /* ---- the entry's table block into LDS ---- */
      __syncthreads(); /* the previous entry's readers are done (and sEV) */
      {
        const v2d *src = reinterpret_cast<const v2d *>(
            tab + (long)(prog.base + e) * PGF_TAB);
        v2d *dst = reinterpret_cast<v2d *>(sT);
        const int n0 = (pgf_tip(tc, 0) ? PGF_HALF : PGF_PLEN) / 2;
        const int n1 = (pgf_tip(tc, 1) ? PGF_HALF : PGF_PLEN) / 2;
        for (int i = tid; i < n0; i += PGF_BLOCK) dst[i] = src[i];
        for (int i = tid; i < n1; i += PGF_BLOCK)
          dst[PGF_HALF / 2 + i] = src[PGF_HALF / 2 + i];
      }
      __syncthreads();

      /* ---- entry e on the lane's (site, cat, half) ---- */
      if (active) {
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
            const v2d v = *reinterpret_cast<const v2d *>(ev + l * 20 + 4 * j);
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
          /* all 80 span entries below the threshold = all eight lanes of the
           * site vote small */
          bool small = true;
#pragma unroll
          for (int s = 0; s < 10; s++)
            small &= (fabs(acc[s]) < MINLIKELIHOOD);
          const unsigned long long m = __ballot(small);
          if (((m >> (lane & ~7)) & 0xFFULL) == 0xFFULL) {
#pragma unroll
            for (int s = 0; s < 10; s++) acc[s] *= TWOTOTHE256;
            if ((lane & 7) == 0)
              atomicAdd(scalerInc + prog.base + e, (unsigned int)wgt[site]);
          }
        }

        double *out = &clv[(long)prog.x3[e] * clvStride + col];
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

/* --- host side: glue behind examl_hip_newview_traversal_prot_gamma -------- */

static int prot_gamma_fused_depth(void) { return PGF_D; }

/* blocks of a launch: the blocks the device holds at once */
static int prot_gamma_fused_grid_cap(void) {
  static int cap = 0;
  if (cap > 0) return cap;
  int dev = 0, cus = 0, per_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                            dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(
          &per_cu, k_newview_prot_gamma_fused<false>, PGF_BLOCK, 0) !=
          hipSuccess ||
      cus < 1 || per_cu < 1) {
    (void)hipGetLastError();
    return 0;
  }
  return cap = cus * per_cu;
}

/* Device scratch of the entry tables, one slot per engine (keyed by its
 * device P buffer, like the pinned P staging), grown on demand.  A cached
 * graph holds the address, so growing clears the graph cache; hipFree waits
 * for the kernels that still read the old block. */
struct ProtTabSlot {
  const void *key;
  double *buf;
  size_t cap; /* entries */
};
static thread_local std::vector<ProtTabSlot> g_prot_tab_slots;

static double *prot_gamma_tab_get(const void *dev_pbuf, int numOps) {
  ProtTabSlot *slot = nullptr;
  for (auto &sl : g_prot_tab_slots)
    if (sl.key == dev_pbuf) {
      slot = &sl;
      break;
    }
  if (!slot) {
    g_prot_tab_slots.push_back({dev_pbuf, nullptr, 0});
    slot = &g_prot_tab_slots.back();
  }
  if ((size_t)numOps > slot->cap) {
    if (slot->buf) {
      (void)hipFree(slot->buf);
      examl_hip_graphs_clear();
    }
    slot->buf = nullptr;
    slot->cap = 0;
    const size_t want = (size_t)numOps * 2;
    if (hipMalloc((void **)&slot->buf, want * PGF_TAB * sizeof(double)) !=
        hipSuccess) {
      (void)hipGetLastError();
      slot->buf = nullptr;
      return nullptr;
    }
    slot->cap = want;
  }
  return slot->buf;
}

/* one run of >= 2 entries of the traversal c: its tables, then the run */
static void launch_prot_gamma_fused(const FusedProg &pg, const TravCall &c,
                                    double *tab) {
  const long tiles = (c.n + PGF_SITES - 1) / PGF_SITES;
  const int cap = prot_gamma_fused_grid_cap();
  const int grid = (int)(tiles < cap ? tiles : cap);
  with_flag(g_fast_math, [&](auto fast) {
    hipLaunchKernelGGL((k_prot_gamma_tables<decltype(fast)::value>),
                       dim3(pg.count, 2), dim3(NV_BLOCK), 0, c.stream, pg,
                       c.pbuf, c.tipVec, tab);
    hipLaunchKernelGGL((k_newview_prot_gamma_fused<decltype(fast)::value>),
                       dim3(grid), dim3(PGF_BLOCK), 0, c.stream, pg, c.clv,
                       c.clvStride, c.tips, c.tipStride, tab, c.EV, c.wgt,
                       c.n, c.inc);
  });
}

extern "C" int examl_hip_prot_gamma_fused_tile_sites(void) {
  return PGF_SITES;
}

extern "C" int examl_hip_prot_gamma_fused_depth(void) { return PGF_D; }

extern "C" int examl_hip_prot_gamma_fused_grid_cap(void) {
  return prot_gamma_fused_grid_cap();
}

extern "C" int examl_hip_prot_gamma_fused_launches(void) {
  return g_prot_gamma_fused_launches;
}
