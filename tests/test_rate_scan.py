"""The -m PSR per-site rate search on the GPU (k_rate_scan_dna_cat through
DnaCatEngine.rate_scan and TreeSearch.optimize_rate_categories) against the
host path it replaces: examl_host_evaluate_partial_dna_cat (bit-exact
against the reference's evaluatePartialGTRCAT, tests/test_cat.py) and the
Python scan loop.

Per-site lnL: relative 1e-12, the bound tests/test_cat.py holds the DNA CAT
evaluate kernel to against the oracle; the only differences are the device's
exp and log.  Chosen rates: bit-equal.  The scan cases are seeded so that no
comparison the host makes is within 1e-8 of a tie or of eps (asserted on the
host values), eight orders above the lnL differences between the two sides.
"""

import ctypes
import functools

import numpy as np
import pytest

import examl_amd as ea
from examl_amd.search import TreeSearch
from examl_amd.synthetic import make_alignment
from tests.helpers import (OracleCatEngine, deep_caterpillar, make_synthetic,
                           random_tips)

RTOL = 1e-12
EPS = 0.00001
MODEL = ea.DnaGtrModel([0.3, 0.2, 0.26, 0.24], [1.2, 2.4, 0.7, 0.9, 3.1, 1.0],
                       1.0)
GLOBAL_BUDGET = 5 * 32 * 64   # bal64 needs 6 slots: its launch goes global


def balanced(ntips):
    """Tip 1 on top of a balanced rooted tree over tips 2..ntips."""
    t = ea.PhyloTree(ntips)
    inner = iter(range(ntips + 1, 2 * ntips - 1))

    def build(tips):
        if len(tips) == 1:
            return tips[0]
        a, b = build(tips[:len(tips) // 2]), build(tips[len(tips) // 2:])
        m = next(inner)
        t.add_edge(m, a, 0.9)
        t.add_edge(m, b, 0.9)
        return m
    t.add_edge(1, build(list(range(2, ntips + 1))), 0.9)
    return t


@functools.lru_cache(maxsize=None)
def tree_of(name):
    if name == "rand4":
        return ea.PhyloTree.random(4, seed=2, rng_z=True)
    if name == "rand12":
        return ea.PhyloTree.random(12, seed=4, rng_z=True)
    t = {"cat12": lambda: ea.PhyloTree.caterpillar(12),
         "bal16": lambda: balanced(16), "bal64": lambda: balanced(64)}[name]()
    rng = np.random.default_rng(len(name) + t.ntips)
    for a, b in t.edges():
        t.set_z(a, b, float(rng.uniform(0.2, 0.98)))
    return t


TREES = ("rand4", "rand12", "cat12", "bal16", "bal64")


def budget_of(name):
    return GLOBAL_BUDGET if name == "bal64" else -1


@functools.lru_cache(maxsize=None)
def data_of(ntips, width):
    tips, _ = make_synthetic(ntips, width, seed=width + ntips)
    wgt = np.random.default_rng(width).integers(1, 6, width).astype(np.int32)
    return tips, wgt


def host_eval_fn(tree, tips, wgt, model=MODEL):
    """site, rate -> examl_host_evaluate_partial_dna_cat over the full
    traversal at tip 1."""
    entries, (p, q, z) = tree.full_traversal()
    arr = (ea.TravEntry * len(entries))(*entries)
    fn = ea.lib().examl_host_evaluate_partial_dna_cat
    vp = ctypes.c_void_p
    fixed = [a.ctypes.data_as(vp) for a in
             (model.EIGN, model.EI, model.EV, model.tipVector, tips)]
    head = (ctypes.cast(arr, vp), len(entries), p, q, ctypes.c_double(z))
    tail = (*fixed, ctypes.c_long(tips.shape[1]), tree.ntips)

    def ev(i, ki):
        return fn(*head, ctypes.c_long(i), ctypes.c_double(ki), int(wgt[i]),
                  *tail)
    ev.keep = arr
    return ev


def host_scan(ev, patrat0, lo, up):
    """The scan loop of TreeSearch.optimize_rate_categories; also returns
    the smallest distance of a compared |delta lnL| from 0 and from eps."""
    patrat, lhs = patrat0.copy(), np.zeros(len(patrat0))
    margin = [np.inf]

    def better(v, best):
        d = abs(best - v)
        margin[0] = min(margin[0], d, abs(d - EPS))
        return v > best and d > EPS

    for i, r0 in enumerate(patrat0):
        l0 = ev(i, r0)
        best = {-1: (l0, r0), 1: (l0, r0)}
        for sign, step in ((-1, lo), (1, up)):
            k = 1
            while sign > 0 or r0 - k * step > 0.0001:
                rate = r0 + k * step if sign > 0 else r0 - k * step
                v = ev(i, rate)
                if not better(v, best[sign][0]):
                    break
                best[sign] = (v, rate)
                k += 1
        (left_lh, left_rate), (right_lh, right_rate) = best[-1], best[1]
        if right_lh > l0 and left_lh > l0:
            margin[0] = min(margin[0], abs(right_lh - left_lh))
        lhs[i] = l0
        if right_lh > l0 or left_lh > l0:
            patrat[i], lhs[i] = (right_rate, right_lh) \
                if right_lh > left_lh else (left_rate, left_lh)
    return patrat, lhs, margin[0]


def gpu_engine(tree, tips, wgt, cls=None):
    cls = cls or ea.DnaCatEngine
    return cls(tips, wgt, MODEL, np.zeros(tips.shape[1], dtype=np.int32),
               np.array([1.0]), device="cuda:0")


def check_lhs(got, ref):
    err = np.abs(got - ref) / np.abs(ref)
    print(f"largest relative lnL error {err.max():.3e} over {len(ref)} sites")
    assert (err <= RTOL).all(), (int(err.argmax()), err.max())


def kernel(tree, tips, wgt, patrat, lo, up, max_k, budget, home):
    entries, (p, q, z) = tree.full_traversal()
    out = gpu_engine(tree, tips, wgt).rate_scan(
        entries, p, q, z, patrat, lo, up, max_k=max_k, lds_budget=budget)
    assert ea.lib().examl_hip_rate_kernel_launches() == 1
    assert ea.lib().examl_hip_rate_scan_slot_home() == home
    return out


# one block handles more than one site past this many (grid-stride wrap)
WRAP_N = 64 * 4096 + 1037


@pytest.mark.gpu
@pytest.mark.parametrize("name,width", [(t, w) for t in TREES
                                        for w in (1, 63, 64, 65, 257)]
                         + [("rand4", WRAP_N)])
def test_evaluation_alone(name, width):
    assert WRAP_N > ea.lib().examl_hip_rate_scan_lanes()
    tree = tree_of(name)
    tips, wgt = data_of(tree.ntips, width)
    rates = np.random.default_rng(width + 1).uniform(0.05, 4.0, width)
    ev = host_eval_fn(tree, tips, wgt)
    ref = np.array([ev(i, rates[i]) for i in range(width)])
    patrat, lhs = kernel(tree, tips, wgt, rates, 0.5, 1.0, 0,
                         budget_of(name), int(name == "bal64"))
    assert np.array_equal(patrat, rates)
    check_lhs(lhs, ref)


@functools.lru_cache(maxsize=None)
def deep_case():
    tree = deep_caterpillar(300)
    tips, _ = random_tips(300, 65, (1, 2, 4, 8), seed=9)
    wgt = np.random.default_rng(9).integers(1, 6, 65).astype(np.int32)
    rates = np.random.default_rng(10).uniform(0.05, 4.0, 65)
    ev = host_eval_fn(tree, tips, wgt)
    return tree, tips, wgt, rates, np.array([ev(i, rates[i])
                                             for i in range(65)])


def test_deep_case_rescales_on_the_host():
    """Every site's host value crosses 2^-256 at least once on the way up,
    some more than once."""
    _, _, wgt, _, ref = deep_case()
    assert (ref / wgt < -256 * np.log(2.0)).all()
    assert (ref / wgt < -512 * np.log(2.0)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("budget,home", [(-1, 0), (0, 1)])
def test_rescaling(budget, home):
    tree, tips, wgt, rates, ref = deep_case()
    assert (ref / wgt < -256 * np.log(2.0)).all()
    _, lhs = kernel(tree, tips, wgt, rates, 0.5, 1.0, 0, budget, home)
    check_lhs(lhs, ref)


SCAN_CASES = [(t, w, s, i) for t in TREES for w in (65, 257)
              for s in (False, True) for i in (1, 3)]
# one data seed per case, in the order of SCAN_CASES, chosen so that the
# host loop meets no near tie (test_scan_cases_hold_no_near_tie)
SCAN_SEEDS = dict(zip(SCAN_CASES, [
    1, 2, 1, 10, 1, 66, 1, 48, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
    1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 1, 1, 1, 1, 1, 1, 1, 1]))


@functools.lru_cache(maxsize=None)
def scan_case(name, width, spread, inv):
    seed = SCAN_SEEDS[name, width, spread, inv]
    tree = tree_of(name)
    # bases only (an all-gap column has the same lnL at every rate, an exact
    # tie) and columns with signal: columns of random bases favour ever
    # higher rates, and a scan that creeps up a saturating curve at the fine
    # spacing passes eps in steps of a few 1e-7
    tips, _ = make_alignment(tree.ntips, width, seed=seed, ambiguity=0.0)
    rng = np.random.default_rng(seed)
    wgt = rng.integers(1, 6, width).astype(np.int32)
    start = rng.uniform(0.1, 3.0, width) if spread else np.ones(width)
    lo, up = (0.5, 1.0) if inv == 1 else (0.05 / inv, 0.1 / inv)
    return (tree, tips, wgt, start, lo, up,
            host_scan(host_eval_fn(tree, tips, wgt), start, lo, up))


@pytest.mark.parametrize("case", SCAN_CASES)
def test_scan_cases_hold_no_near_tie(case):
    margin = scan_case(*case)[6][2]
    print(f"smallest margin {margin:.3e}")
    assert margin > 1e-8


@pytest.mark.gpu
@pytest.mark.parametrize("case", SCAN_CASES)
def test_scan(case):
    tree, tips, wgt, start, lo, up, (ref_rat, ref_lhs, margin) = \
        scan_case(*case)
    assert margin > 1e-8
    patrat, lhs = kernel(tree, tips, wgt, start, lo, up, None,
                         budget_of(case[0]), int(case[0] == "bal64"))
    assert np.array_equal(patrat, ref_rat)
    check_lhs(lhs, ref_lhs)


def search_for(config, cls):
    widths = (130,) if config == "one" else (130, 70)
    tree = ea.PhyloTree.random(12, seed=3, rng_z=True)
    engines = [cls(*data_of(12, w), MODEL, np.zeros(w, dtype=np.int32),
                   np.array([1.0]), **({} if cls is OracleCatEngine
                                       else {"device": "cuda:0"}))
               for w in widths]
    return TreeSearch(tree, engines, rate_het="CAT",
                      per_gene_bl=config == "two-M")


@pytest.mark.gpu
@pytest.mark.parametrize("config,cls", [
    ("one", ea.DnaCatEngine), ("one", ea.SaveCatEngine),
    ("two", ea.DnaCatEngine), ("two-M", ea.DnaCatEngine)])
def test_through_tree_search(config, cls):
    got = {}
    try:
        for on in (1, 0):
            ea.lib().examl_hip_use_rate_kernel(on)
            ts = search_for(config, cls)
            ts.evaluate_generic(full=True)
            for _ in range(2):   # second round starts from spread rates
                ts.optimize_rate_categories(25)
                assert ts.rate_opt_path == ("kernel" if on else "host")
            got[on] = ([e.cptr.copy() for e in ts.engines],
                       [e.per_site_rates.copy() for e in ts.engines],
                       ts.likelihood)
    finally:
        ea.lib().examl_hip_use_rate_kernel(1)
    for a, b in zip(got[1][0] + got[1][1], got[0][0] + got[0][1]):
        assert np.array_equal(a, b)
    assert abs(got[1][2] - got[0][2]) < 1e-9


def E(tc, p, q, r):
    e = ea.TravEntry()
    e.tipCase, e.pNumber, e.qNumber, e.rNumber, e.qz, e.rz = tc, p, q, r, .9, .9
    return e


TT, TI, II = ea.TIP_TIP, ea.TIP_INNER, ea.INNER_INNER


@pytest.mark.parametrize("mxtips,ops,slots,L", [
    (3, [E(TT, 4, 2, 3)], [0], 1),
    (6, [E(TT, 7, 2, 3), E(TI, 8, 4, 7), E(TI, 9, 5, 8), E(TI, 10, 6, 9)],
     [0, 0, 0, 0], 1),
    (5, [E(TT, 6, 2, 3), E(TT, 7, 4, 5), E(II, 8, 6, 7)], [0, 1, 0], 2),
    (9, [E(TT, 10, 2, 3), E(TT, 11, 4, 5), E(II, 12, 10, 11),
         E(TT, 13, 6, 7), E(TT, 14, 8, 9), E(II, 15, 13, 14),
         E(II, 16, 12, 15)], [0, 1, 0, 1, 2, 1, 0], 3),
    (5, [E(TT, 6, 2, 3), E(II, 8, 6, 7)], None, None),   # 7 never produced
    (5, [E(TT, 6, 2, 3), E(TI, 7, 4, 6), E(TI, 8, 5, 6)], None, None),
])
def test_planner(mxtips, ops, slots, L):
    arr = (ea.TravEntry * len(ops))(*ops)
    out = (ctypes.c_int * len(ops))()
    n_slots = ctypes.c_int(-1)
    rc = ea.lib().examl_host_rate_scan_plan(
        ctypes.cast(arr, ctypes.c_void_p), len(ops), mxtips, out,
        ctypes.byref(n_slots))
    if slots is None:
        assert rc == -1
    else:
        assert (rc, list(out), n_slots.value) == (0, slots, L)


def test_oracle_engines_keep_the_host_loop():
    ts = search_for("one", OracleCatEngine)
    ts.evaluate_generic(full=True)
    ts.optimize_rate_categories(25)
    assert ts.rate_opt_path == "host"
