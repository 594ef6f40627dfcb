"""Evaluate, sum and core of partitioned DNA PSR over all partitions
(k_evaluate_dna_cat_mseg / k_sum_dna_cat_mseg / k_core_dna_cat_mseg behind
MultiDnaCatEngine) against each DnaCatEngine called alone, bit for bit, and
against the CPU oracle at the suite's tolerances (lnL 1e-11 relative, the
derivatives 1e-10 as tests/test_cat.py holds the per-partition core kernel).
Partitions have distinct models and category counts from (25, 1, 7)."""

import ctypes

import numpy as np
import pytest

import examl_amd as ea
from tests import helpers as H
from tests.test_cat_fused import categories
from tests.test_fused_traversal import SENTINEL
from tests.test_multi_cat_onchip import engines, specs_for

RAGGED = (255, 257, 0, 1, 700)


def cap():
    return ea.lib().examl_hip_multi_cat_root_grid_cap()


def root_units(widths, short=0):
    g = [min(-(-w // 256), cap()) for w in widths]
    n = sum(g) - short
    prefix = (ctypes.c_int * (len(widths) + 1))()
    part = (ctypes.c_int * max(n, 1))()
    rc = ea.lib().examl_hip_multi_cat_root_units(
        len(widths), (ctypes.c_long * len(widths))(*widths), prefix, part, n)
    return rc, list(prefix), list(part)[:n], g


@pytest.mark.parametrize("widths", [(1,), RAGGED, "wrap"])
def test_unit_table(widths):
    if widths == "wrap":
        widths = (cap() * 256 + 300, 1)
    rc, prefix, part, g = root_units(widths)
    assert rc == sum(g)
    assert prefix == [0] + list(np.cumsum(g))
    assert part == [p for p, k in enumerate(g) for _ in range(k)]
    assert root_units(widths, short=1)[0] == -1


def inner_edge(tree):
    return next((a, b) for a in tree.adj for b in tree.adj[a]
                if not tree.is_tip(a) and not tree.is_tip(b))


def vec(v, n):
    return np.broadcast_to(np.asarray(v, dtype=float), (n,))


def compare(tree, p, q, guards, multi, z, lzs, active=None):
    """Every root operation of `multi` against the engines called alone with
    their own z / lz, bit for bit; masked and empty partitions hold zeros
    and their sum buffers the sentinel.  -> (lnl [NP], [derivs [NP, 2]])"""
    import torch
    NP = len(guards)
    on = [g.eng.width > 0 and (active is None or bool(active[m]))
          for m, g in enumerate(guards)]
    lnl = multi.evaluate_root(tree, p, q, z, active=active).cpu().numpy()
    assert multi.root_kernels() >= 1
    for g in guards:
        g.eng.d_sum = torch.full((g.eng.width * 4,), SENTINEL,
                                 dtype=torch.float64, device="cuda:0")
    multi.sum_root(tree, p, q, active=active)
    assert multi.root_kernels() >= 1
    sums = [g.eng.d_sum.cpu().numpy() for g in guards]
    ders = [multi.core_derivs_vec(lz, active=active).cpu().numpy()
            for lz in lzs]
    assert multi.root_kernels() >= 1
    for m, g in enumerate(guards):
        if not on[m]:
            assert lnl[m] == 0 and all((d[m] == 0).all() for d in ders)
            assert (sums[m] == SENTINEL).all()
            continue
        e = g.eng
        assert lnl[m] == e.evaluate_root(tree, p, q,
                                         float(vec(z, NP)[m])).item()
        e.sum_root(tree, p, q)
        assert np.array_equal(sums[m], e.d_sum.cpu().numpy())
        for lz, d in zip(lzs, ders):
            own = e.core_derivs_async(float(vec(lz, NP)[m])).cpu().numpy()
            assert np.array_equal(d[m], own), (m, d[m], own)
    return lnl, ders


def traversed(widths, tree, **kw):
    parts = specs_for(widths, ntips=tree.ntips, **kw)
    guards, multi = engines(parts)
    multi.newview_traversal(tree.full_traversal()[0])
    return parts, guards, multi


@pytest.mark.gpu
@pytest.mark.parametrize("at_tip", [True, False])
@pytest.mark.parametrize("widths", [(1,), RAGGED])
def test_parity_with_engines_and_oracle(widths, at_tip):
    tree = ea.PhyloTree.random(12, seed=11, rng_z=True)
    parts, guards, multi = traversed(widths, tree)
    p, q = (1, next(iter(tree.adj[1]))) if at_tip else inner_edge(tree)
    z, lzs = tree.get_z(p, q), (np.log(0.3), np.log(0.9))
    lnl, ders = compare(tree, p, q, guards, multi, z, lzs)
    entries = tree.full_traversal()[0]
    for m, (tips, wgt, mdl, cptr, rates) in enumerate(parts):
        if tips.shape[1] == 0:
            continue
        tips = np.ascontiguousarray(tips)
        ref = H.oracle_cat_full_lnl(entries, (p, q, z), tree, mdl, tips, wgt,
                                    cptr, rates)
        print(f"partition {m}: lnL {lnl[m]!r} oracle {ref!r}")
        assert abs(lnl[m] - ref) <= 1e-11 * abs(ref)
        orc = H.OracleCatEngine(tips, wgt, mdl, cptr, rates)
        orc.newview_traversal(entries)
        orc.sum_root(tree, p, q)
        for lz, d in zip(lzs, ders):
            want = orc.core_derivs(float(lz))
            print(f"partition {m} lz {lz}: {d[m]!r} oracle {want!r}")
            assert np.allclose(d[m], want, rtol=1e-10, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("active", [(0, 1, 1), (0, 0, 0)])
def test_masked_partitions(active):
    tree = ea.PhyloTree.random(12, seed=31, rng_z=True)
    _, guards, multi = traversed((150, 300, 64), tree)
    p, q = inner_edge(tree)
    compare(tree, p, q, guards, multi, tree.get_z(p, q), (np.log(0.4),),
            active=active)


@pytest.mark.gpu
def test_per_partition_z_and_lz():
    tree = ea.PhyloTree.random(12, seed=31, rng_z=True)
    _, guards, multi = traversed((300, 259, 5), tree)
    p, q = inner_edge(tree)
    lnl, ders = compare(tree, p, q, guards, multi, (0.2, 0.5, 0.8),
                        (np.log((0.3, 0.6, 0.9)),))
    assert len(set(lnl)) == 3


@pytest.mark.gpu
def test_blocks_wrap_past_the_grid_cap():
    tree = ea.PhyloTree.random(4, seed=3, rng_z=True)
    _, guards, multi = traversed((cap() * 256 + 300, 1), tree, seed=12)
    p, q = inner_edge(tree)
    compare(tree, p, q, guards, multi, tree.get_z(p, q), (np.log(0.5),))


@pytest.mark.gpu
def test_set_site_rates_between_calls():
    tree = ea.PhyloTree.random(12, seed=5, rng_z=True)
    _, guards, multi = traversed((65, 3, 130), tree, seed=13)
    p, q = 1, next(iter(tree.adj[1]))
    z, lzs = tree.get_z(p, q), (np.log(0.5),)
    before, _ = compare(tree, p, q, guards, multi, z, lzs)
    assert guards[2].eng.num_cats == 7
    guards[2].eng.set_site_rates(*categories(130, 25, 5))
    multi.newview_traversal(tree.full_traversal()[0])
    after, _ = compare(tree, p, q, guards, multi, z, lzs)
    assert after[2] != before[2] and (after[:2] == before[:2]).all()


@pytest.mark.gpu
def test_tree_search_takes_the_all_partition_root_kernels():
    from examl_amd.search import TreeSearch
    parts = specs_for((150, 300, 64))
    got = {}
    try:
        for on in (1, 0):
            ea.lib().examl_hip_multi_use_fused(on)
            guards, _ = engines(parts)
            tree = ea.PhyloTree.random(12, seed=31, rng_z=True)
            ts = TreeSearch(tree, [g.eng for g in guards], rate_het="CAT")
            lnl = ts.evaluate_generic(full=True)
            assert (ts.fused_cat.root_kernels() >= 1) == bool(on)
            p, q = inner_edge(tree)
            znew = ts.makenewz_generic(p, q, tree.get_z(p, q), 16)
            assert (ts.fused_cat.root_kernels() >= 1) == bool(on)
            got[on] = (lnl, list(ts.per_partition_lnl), znew)
    finally:
        ea.lib().examl_hip_multi_use_fused(1)
    assert got[1] == got[0], (got[1], got[0])
    assert got[1][2] != tree.get_z(p, q)
