"""Kernel parity where the other kernel-level tests never go: ragged widths,
waves in which some sites rescale and their neighbours do not, the
streaming-store (NT) instantiations, grid-stride wrap, the scaler-undo
term, and engine-level bit-exactness for protein CAT and LG4.

Expected values come from the CPU oracle (liboracle.so) at test time; the
rescale decisions are additionally known by construction
(tests/helpers.make_rescale_mix).  newview and sum are compared bit for
bit.  The reductions (evaluate, core) are compared with a longdouble
per-site reference (helpers.ld_lnl / ld_core) within
    |gpu - ref| <= 1e-12 * sum_i |w_i * term_i|   (lnL)
    |gpu - ref| <= 1e-11 * sum_i |w_i * term_i|   (each derivative)
— the suite's existing rtol values restated against the absolute sum, so
cancellation in the first derivative makes them neither vacuous nor flaky.
The CPU tests below show that the oracle alone meets these bounds.

Every output buffer carries 64 guard doubles behind its last element; a
tail overrun fails the test instead of corrupting memory.

Grid-stride wrap (more than MAX_GRID * 256 units): DNA GAMMA, DNA CAT and
the protein split-lane INNER_INNER newview are covered.  Protein TIP_TIP,
TIP_INNER, evaluate, sum and core wrap only above 524,288 sites (~336 MB
per CLV) and are left out.
"""

import ctypes
import functools
import math

import numpy as np
import pytest

import examl_amd as ea
import oracle as O
from tests import helpers as H
from tests.helpers import (DERIV_RTOL, EDGE_FAMILIES, LNL_RTOL,
                           RESCALING_CLASSES)

TIP_TIP, TIP_INNER, INNER_INNER = ea.TIP_TIP, ea.TIP_INNER, ea.INNER_INNER
TIPCASES = (TIP_TIP, TIP_INNER, INNER_INNER)
RAGGED = (1, 3, 63, 65, 333)
SEED = 1          # every class holds >= 10% of the 333 sites (asserted)
GUARD = 64
SENTINEL = -7.0e77
LOG_MINLIK = math.log(O.MINLIKELIHOOD)

# grid-stride wrap: one stride is MAX_GRID(8192) * 256 threads = 2,097,152
# units — 524,288 sites for DNA GAMMA (4 lanes/site), 262,144 for the
# protein split-lane II newview (8 lanes/site), 2,097,152 for DNA CAT.
WRAP_N = {"dna_gamma": 524288 + 1037, "dna_cat": 2097152 + 1037,
          "prot_gamma": 262144 + 77}
NT_N = {"dna_gamma": 65536 + 5, "dna_cat": 262144 + 5}


@functools.lru_cache(maxsize=None)
def mix(family, tc, n):
    """Shared, read-only rescale-mix case."""
    return H.make_rescale_mix(family, tc, n, SEED)


@functools.lru_cache(maxsize=3)   # each wrap-width case holds ~0.2-0.5 GB
def tiled(family, tc, n):
    """The n = 333 block tiled to n sites with ONE oracle newview at full
    n for the expectation.  333 = 3*3*37 shares no factor with the
    power-of-two grid stride and n is no multiple of 333 (the last tile is
    truncated), so the tile period never divides the stride: a thread's
    second loop iteration meets another tile phase than its first, and a
    stride error cannot land on an identical copy of the right data."""
    assert n % 333 != 0
    f = H.edge_family(family)
    c = H.tile_edge_case(mix(family, tc, 333), n)
    c.x3, c.inc = H.edge_newview(f, tc, c.x1, c.x2, c.tipX1, c.tipX2, n,
                                 c.wgt, c.cptr)
    if tc != TIP_TIP:
        assert c.inc == int(c.wgt[np.isin(c.classes,
                                          RESCALING_CLASSES)].sum())
    return c


def within(got, ref, abs_sum, rtol, what):
    err = abs(got - ref)
    print(f"{what}: got {got!r} ref {ref!r} err {err:.3e} "
          f"bound {rtol * abs_sum:.3e}")
    assert err <= rtol * abs_sum, (what, got, ref, err, rtol * abs_sum)


# ---------------------------------------------------------------------------
# CPU: the builder predicts the oracle, and the oracle meets the reduction
# bounds against the longdouble reference
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("tc", [TIP_INNER, INNER_INNER])
@pytest.mark.parametrize("family", EDGE_FAMILIES)
def test_rescale_mix_predicts_oracle(family, tc):
    f = H.edge_family(family)
    c = mix(family, tc, 333)
    x3, inc = H.edge_newview(f, tc, c.x1, c.x2, c.tipX1, c.tipX2, c.n,
                             c.wgt, c.cptr)
    assert np.array_equal(x3, c.x3)
    assert inc == c.inc == int(c.wgt[np.isin(c.classes,
                                             RESCALING_CLASSES)].sum())
    for k in H.edge_classes(family):
        share = float((c.classes == k).mean())
        assert share >= 0.10, (family, k, share)
    # classes 1/2 straddle the threshold within one binade of it
    mx = np.abs(x3_unscaled(c)).reshape(c.n, -1).max(axis=1)
    assert ((mx[c.classes == 1] >= 2.0 ** -257) &
            (mx[c.classes == 1] < 2.0 ** -256)).all()
    assert ((mx[c.classes == 2] >= 2.0 ** -256) &
            (mx[c.classes == 2] < 2.0 ** -255)).all()
    # no lucky zeros, nothing near the subnormal range
    assert np.abs(c.x2).min() > 2.0 ** -900


def x3_unscaled(c):
    """Expected x3 with the 2^256 rescale taken back out."""
    f = H.edge_family(c.family)
    up = np.isin(c.classes, RESCALING_CLASSES)
    x = c.x3.reshape(c.n, f.span).copy()
    x[up] = np.ldexp(x[up], -256)
    return x


@pytest.mark.parametrize("tc", [TIP_INNER, INNER_INNER])
@pytest.mark.parametrize("family", EDGE_FAMILIES)
def test_threshold_exact_predicts_oracle(family, tc):
    f, c = H.make_threshold_exact(family, tc)
    x3, inc = H.edge_newview(f, tc, c.x1, c.x2, c.tipX1, c.tipX2, c.n,
                             c.wgt, c.cptr)
    assert np.array_equal(x3, c.x3)
    assert inc == c.inc


def _oracle_reductions_meet_bounds(family, c):
    f = H.edge_family(family)
    for tip in (True, False):
        ref, ab = H.ld_lnl(f, c, tip)
        within(H.edge_evaluate(f, c, tip), ref, ab, LNL_RTOL,
               f"oracle lnL {family} tip={tip} n={c.n}")
    dtab = H.edge_core_dtables(f)
    for tc in TIPCASES:
        st = H.edge_sum(f, tc, c)
        (r1, a1), (r2, a2) = H.ld_core(f, c, st, dtab)
        d1, d2 = H.edge_core(f, c, st)
        within(d1, r1, a1, DERIV_RTOL, f"oracle d1 {family} tc={tc}")
        within(d2, r2, a2, DERIV_RTOL, f"oracle d2 {family} tc={tc}")


@pytest.mark.parametrize("family", EDGE_FAMILIES)
def test_oracle_reductions_meet_bounds(family):
    _oracle_reductions_meet_bounds(family, mix(family, INNER_INNER, 333))


def test_oracle_reductions_meet_bounds_at_wrap_width():
    _oracle_reductions_meet_bounds(
        "dna_gamma", tiled("dna_gamma", INNER_INNER, WRAP_N["dna_gamma"]))


# ---------------------------------------------------------------------------
# GPU plumbing
# ---------------------------------------------------------------------------

def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch, torch.device("cuda:0")


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def hp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Dev:
    """Device copies of one family block's model data."""

    def __init__(self, f):
        torch, dev = _torch()
        self.f, self.torch, self.dev = f, torch, dev
        self.EV = self.up(f.EV)
        self.tv = self.up(f.tipVector)
        self.P = self.up(np.concatenate([f.left, f.right]))
        self.diag = self.up(f.diag)
        self.part = torch.zeros(2 * 8192, dtype=torch.float64, device=dev)

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def guarded(self, n):
        return self.torch.full((n * self.f.span + GUARD,), SENTINEL,
                               dtype=self.torch.float64, device=self.dev)

    def split(self, d_out, n):
        """(payload, guard untouched?) of a guarded output buffer."""
        out = d_out.cpu().numpy()
        m = n * self.f.span
        return out[:m], bool((out[m:] == SENTINEL).all())

    def operands(self, c, tc):
        x1 = self.up(c.x1) if tc == INNER_INNER else None
        x2 = self.up(c.x2) if tc != TIP_TIP else None
        t1 = self.up(c.tipX1) if tc != INNER_INNER else None
        t2 = self.up(c.tipX2) if tc == TIP_TIP else None
        return x1, x2, t1, t2

    def newview(self, c, tc):
        """-> (x3, guard_ok, inc)"""
        f, L = self.f, ea.lib()
        x1, x2, t1, t2 = self.operands(c, tc)
        wgt = self.up(c.wgt)
        x3 = self.guarded(c.n)
        inc = self.torch.zeros(1, dtype=self.torch.int32, device=self.dev)
        if f.name == "dna_cat":
            ea.check(L.examl_hip_newview_dna_cat(
                tc, vp(self.EV), vp(self.up(c.cptr)), vp(x1), vp(x2),
                vp(x3), vp(self.tv), vp(t1), vp(t2), c.n, vp(self.P),
                f.num_cats, vp(wgt), vp(inc), None), "newview_cat")
        else:
            fn = (L.examl_hip_newview_dna_gamma if f.states == 4
                  else L.examl_hip_newview_prot_gamma)
            half = 4 * f.states * f.states
            ea.check(fn(tc, vp(x1), vp(x2), vp(x3), vp(self.EV),
                        vp(self.tv), vp(t1), vp(t2), c.n, vp(self.P),
                        ctypes.c_void_p(self.P.data_ptr() + half * 8),
                        vp(wgt), vp(inc), None), "newview")
        self.torch.cuda.synchronize()
        out, ok = self.split(x3, c.n)
        return out, ok, int(inc.item())

    def sum(self, c, tc):
        """-> (device sum buffer, sum table, guard_ok)"""
        f, L = self.f, ea.lib()
        x1, x2, t1, t2 = self.operands(c, tc)
        d_sum = self.guarded(c.n)
        fn = {"dna_gamma": L.examl_hip_sum_dna_gamma,
              "prot_gamma": L.examl_hip_sum_prot_gamma,
              "dna_cat": L.examl_hip_sum_dna_cat}[f.name]
        ea.check(fn(tc, vp(d_sum), vp(x1), vp(x2), vp(self.tv), vp(t1),
                    vp(t2), c.n, None), "sum")
        self.torch.cuda.synchronize()
        out, ok = self.split(d_sum, c.n)
        return d_sum, out, ok

    def evaluate(self, c, tip, gs=None, initial=0.0):
        f, L, torch = self.f, ea.lib(), self.torch
        x1 = None if tip else self.up(c.x1)
        t1 = self.up(c.tipX1) if tip else None
        x2, wgt = self.up(c.x2), self.up(c.wgt)
        lnl = torch.full((1,), initial, dtype=torch.float64,
                         device=self.dev)
        d_gs = (torch.tensor(gs, dtype=torch.int32, device=self.dev)
                if gs is not None else None)
        gp = vp(d_gs) if gs is not None else None
        gq = (ctypes.c_void_p(d_gs.data_ptr() + 4) if gs is not None
              else None)
        if f.name == "dna_cat":
            ea.check(L.examl_hip_evaluate_dna_cat(
                vp(self.up(c.cptr)), vp(wgt), vp(x1), vp(x2), vp(self.tv),
                vp(t1), c.n, vp(self.diag), f.num_cats, gp, gq,
                ctypes.c_double(LOG_MINLIK), vp(self.part), vp(lnl), None),
                "evaluate_cat")
        else:
            fn = (L.examl_hip_evaluate_dna_gamma if f.states == 4
                  else L.examl_hip_evaluate_prot_gamma)
            ea.check(fn(vp(wgt), vp(x1), vp(x2), vp(self.tv), vp(t1), c.n,
                        vp(self.diag), gp, gq, ctypes.c_double(LOG_MINLIK),
                        vp(self.part), vp(lnl), None), "evaluate")
        torch.cuda.synchronize()
        return float(lnl.item())

    def core(self, c, d_sum):
        f, L, torch = self.f, ea.lib(), self.torch
        wgt = self.up(c.wgt)
        out2 = torch.zeros(2, dtype=torch.float64, device=self.dev)
        dtab = torch.zeros(512, dtype=torch.float64, device=self.dev)
        if f.name == "dna_cat":
            ea.check(L.examl_hip_core_root_dna_cat(
                c.n, vp(d_sum), hp(f.EIGN), hp(f.rates), f.num_cats,
                ctypes.c_double(f.lz), vp(wgt), vp(self.up(c.cptr)),
                vp(dtab), vp(self.part), vp(out2), None), "core_cat")
        else:
            fn = (L.examl_hip_core_root_dna_gamma if f.states == 4
                  else L.examl_hip_core_root_prot_gamma)
            ea.check(fn(c.n, vp(d_sum), hp(f.EIGN), hp(f.rates),
                        ctypes.c_double(f.lz), vp(wgt), vp(dtab),
                        vp(self.part), vp(out2), None), "core")
        torch.cuda.synchronize()
        o = out2.cpu().numpy()
        return float(o[0]), float(o[1])


_DEV = {}


def dev_of(f, key=None):
    key = key or f.name
    if key not in _DEV:
        _DEV[key] = Dev(f)
    return _DEV[key]


def check_newview(d, c, tc):
    x3, guard_ok, inc = d.newview(c, tc)
    assert guard_ok, "newview wrote past the end of x3"
    assert inc == c.inc, (inc, c.inc)
    assert np.array_equal(x3, c.x3)


def check_sum(d, c, tc):
    d_sum, st, guard_ok = d.sum(c, tc)
    assert guard_ok, "sum wrote past the end of the sum table"
    assert np.array_equal(st, H.edge_sum(d.f, tc, c))
    return d_sum, st


def check_evaluate(d, c, tip):
    ref, ab = H.ld_lnl(d.f, c, tip)
    within(d.evaluate(c, tip), ref, ab, LNL_RTOL,
           f"lnL {d.f.name} tip={tip} n={c.n}")


def check_core(d, c, d_sum, st, what):
    (r1, a1), (r2, a2) = H.ld_core(d.f, c, st, H.edge_core_dtables(d.f))
    g1, g2 = d.core(c, d_sum)
    within(g1, r1, a1, DERIV_RTOL, f"d1 {what}")
    within(g2, r2, a2, DERIV_RTOL, f"d2 {what}")


# ---------------------------------------------------------------------------
# B1. ragged widths with mixed rescaling
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", RAGGED)
@pytest.mark.parametrize("tc", TIPCASES)
@pytest.mark.parametrize("family", EDGE_FAMILIES)
def test_newview_ragged_rescale_mix(family, tc, n):
    check_newview(dev_of(H.edge_family(family)), mix(family, tc, n), tc)


@pytest.mark.gpu
@pytest.mark.parametrize("tc", [TIP_INNER, INNER_INNER])
@pytest.mark.parametrize("family", EDGE_FAMILIES)
def test_newview_threshold_exact(family, tc):
    """Span maxima exactly ON 2^-256 must not rescale (strict <)."""
    f, c = H.make_threshold_exact(family, tc)
    check_newview(dev_of(f, key=family + "/identity"), c, tc)


@pytest.mark.gpu
@pytest.mark.parametrize("n", RAGGED)
@pytest.mark.parametrize("tc", TIPCASES)
@pytest.mark.parametrize("family", EDGE_FAMILIES)
def test_sum_and_core_ragged(family, tc, n):
    d = dev_of(H.edge_family(family))
    c = mix(family, INNER_INNER, n)
    d_sum, st = check_sum(d, c, tc)
    check_core(d, c, d_sum, st, f"{family} tc={tc} n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", RAGGED)
@pytest.mark.parametrize("tip", [True, False], ids=["tip", "inner"])
@pytest.mark.parametrize("family", EDGE_FAMILIES)
def test_evaluate_ragged(family, tip, n):
    check_evaluate(dev_of(H.edge_family(family)),
                   mix(family, INNER_INNER, n), tip)


# ---------------------------------------------------------------------------
# B2. scaler undo in k_reduce_lnl
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("tip", [True, False], ids=["tip", "inner"])
@pytest.mark.parametrize("family", EDGE_FAMILIES)
def test_evaluate_scaler_undo(family, tip):
    """gsP = 3, gsQ = 5 and a non-zero starting *dev_lnl (the entry point
    accumulates): initial + oracle lnL + 8 * log(2^-256)."""
    f = H.edge_family(family)
    c = mix(family, INNER_INNER, 333)
    initial = -1234.5
    got = dev_of(f).evaluate(c, tip, gs=[3, 5], initial=initial)
    expect = initial + H.edge_evaluate(f, c, tip) + 8 * LOG_MINLIK
    _, ab = H.ld_lnl(f, c, tip)
    within(got, expect, ab, LNL_RTOL, f"undo {family} tip={tip}")
    # and the undo term is really in there
    assert abs(got - (initial + H.edge_evaluate(f, c, tip))) > 1000


# ---------------------------------------------------------------------------
# B3. streaming-store (NT) instantiations
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("tc", TIPCASES)
@pytest.mark.parametrize("family", ["dna_gamma", "dna_cat"])
def test_newview_streaming_store(family, tc):
    n = NT_N[family]
    check_newview(dev_of(H.edge_family(family)), mix(family, tc, n), tc)


@pytest.mark.gpu
def test_traversal_executor_streaming_store():
    """The traversal executor picks NT on its own (n >= 65536): CLV slots
    and scalers of a 4-taxon tree against the oracle replay."""
    torch, dev = _torch()
    ntips, width = 4, NT_N["dna_gamma"]
    f = H.edge_family("dna_gamma")
    tips, wgt = H.make_synthetic(ntips, width, seed=12)
    tree = ea.PhyloTree.random(ntips, seed=3, rng_z=True)
    eng = ea.DnaGammaEngine(tips, wgt, f.model, device=dev)
    entries, root = tree.full_traversal()
    lnl = eng.full_lnl(tree).item()
    ref, clv_ref, scalers_ref = H.oracle_full_lnl(
        entries, root, tree, f.model, tips, wgt, return_state=True)
    clv = eng.d_clv.cpu().numpy()
    assert len(clv_ref) == ntips - 2
    for slot, x in clv_ref.items():
        assert np.array_equal(clv[slot], x), f"CLV slot {slot} differs"
    sc = eng.d_scalers.cpu().numpy()
    for node in range(ntips + 1, 2 * ntips - 1):
        assert sc[node] == scalers_ref[node]
    assert abs(lnl - ref) <= 1e-11 * abs(ref)


# ---------------------------------------------------------------------------
# B4. grid-stride wrap
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("family,tc", [
    ("dna_gamma", TIP_TIP), ("dna_gamma", TIP_INNER),
    ("dna_gamma", INNER_INNER), ("dna_cat", TIP_INNER),
    ("dna_cat", INNER_INNER), ("prot_gamma", INNER_INNER)])
def test_newview_grid_stride_wrap(family, tc):
    check_newview(dev_of(H.edge_family(family)),
                  tiled(family, tc, WRAP_N[family]), tc)


@pytest.mark.gpu
def test_sum_and_core_grid_stride_wrap():
    d = dev_of(H.edge_family("dna_gamma"))
    c = tiled("dna_gamma", INNER_INNER, WRAP_N["dna_gamma"])
    d_sum, st = check_sum(d, c, INNER_INNER)
    check_core(d, c, d_sum, st, "dna_gamma wrap")


@pytest.mark.gpu
@pytest.mark.parametrize("tip", [True, False], ids=["tip", "inner"])
@pytest.mark.parametrize("family", ["dna_gamma", "dna_cat"])
def test_evaluate_grid_stride_wrap(family, tip):
    check_evaluate(dev_of(H.edge_family(family)),
                   tiled(family, INNER_INNER, WRAP_N[family]), tip)


# ---------------------------------------------------------------------------
# C. engine-level bit-exactness for protein CAT and LG4
# ---------------------------------------------------------------------------

def _engine_pair(kind, ntips, width, seed):
    _, dev = _torch()
    if kind == "prot_cat":
        tips, wgt, model, cptr, rates = H.prot_cat_inputs(ntips, width,
                                                         seed)
        return (ea.ProtCatEngine(tips, wgt, model, cptr, rates, device=dev),
                H.OracleProtCatEngine(tips, wgt, model, cptr, rates))
    tips, wgt = H.random_tips(ntips, width, H.AA_CODES, seed)
    model = ea.Lg4Model.lg4x()
    return (ea.Lg4Engine(tips, wgt, model, device=dev),
            H.OracleLg4Engine(tips, wgt, model))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["random6", "deep"])
@pytest.mark.parametrize("kind", ["prot_cat", "lg4"])
def test_engine_bit_exact_vs_oracle(kind, shape):
    width = 77
    if shape == "random6":
        ntips = 6
        tree = ea.PhyloTree.random(ntips, seed=9, rng_z=True)
    else:
        ntips = H.DEEP_TIPS_PROT
        tree = H.deep_caterpillar(ntips)
    seed = 17 if kind == "prot_cat" else 23
    eng, orc = _engine_pair(kind, ntips, width, seed)
    entries, (p, q, z) = tree.full_traversal()
    eng.newview_traversal(entries)
    orc.newview_traversal(entries)
    if shape == "deep":
        assert orc.scalers.max() > 0, "test must exercise rescaling"
    span = eng.SPAN
    clv = eng.d_clv.cpu().numpy()
    assert len(orc.clv) == ntips - 2
    for slot, x in orc.clv.items():
        assert np.array_equal(clv[slot][:width * span], x), \
            f"{kind} CLV slot {slot} differs"
    sc = eng.d_scalers.cpu().numpy()
    for node in range(ntips + 1, 2 * ntips - 1):
        assert sc[node] == orc.scalers[node], node
    lnl = eng.evaluate_root(tree, p, q, z).item()
    ref = orc.evaluate_root(tree, p, q, z)
    assert math.isfinite(lnl) and abs(lnl - ref) <= 1e-11 * abs(ref)
    eng.sum_root(tree, p, q)
    orc.sum_root(tree, p, q)
    assert np.array_equal(eng.d_sum.cpu().numpy(), orc.sumtable)
