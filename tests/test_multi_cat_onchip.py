"""On-chip DNA PSR (CAT) traversal over all partitions
(k_newview_dna_cat_mseg_fused behind MultiDnaCatEngine) against the CPU
oracle replay per partition: ALL CLV slots and scaler counts bit for bit,
lnL within the suite's 1e-11 relative, guard doubles behind every pool
untouched, fused_launches() >= 1.  Partitions get distinct GTR models
(test_multi_onchip.mk_specs) and category counts from (1, 7, 25), so EV,
tipVector, catOff and the P pitch change between neighbouring tiles."""

import numpy as np
import pytest

import examl_amd as ea
from tests import helpers as H
from tests.test_cat_fused import GuardedCat, categories
from tests.test_fused_traversal import (SENTINEL, assert_state, check_plan,
                                        cherry_caterpillar, deep_stack_tree,
                                        fused_depth, model)
from tests.test_multi_onchip import grid_cap, mk_specs, tile_table

NCATS = (25, 1, 7)


def tile():
    return ea.lib().examl_hip_cat_fused_tile_sites()


def case_widths(name):
    T = tile()
    return {"one": (1,), "ragged": (T - 1, T + 1, 0, 1),
            "three": (3, 65, 2 * T + 5),
            "wrap": ((grid_cap() - 3) * T - 5, 1, 11 * T - 77)}[name]


@pytest.mark.parametrize("name", ["one", "ragged", "three", "wrap"])
def test_tile_table_at_the_cat_tile(name):
    widths, T = case_widths(name), tile()
    want = [(p, s) for p, w in enumerate(widths) for s in range(0, w, T)]
    rc, part, site = tile_table(widths, tile=T)
    assert rc == len(want) and list(zip(part, site)) == want
    assert tile_table(widths, cap=rc - 1, tile=T)[0] == -1


def with_cats(specs, seed=1):
    """(tips, wgt, model) -> (tips, wgt, model, cptr, rates); partition i has
    NCATS[i % 3] categories and its own rates."""
    out = []
    for i, (tips, wgt, mdl) in enumerate(specs):
        cptr, rates = categories(tips.shape[1], NCATS[i % 3], seed + i)
        out.append((tips, wgt, mdl, cptr, rates * (1 + 0.03 * i)))
    return out


def specs_for(widths, ntips=12, seed=5):
    # the generator has no zero-width case: make one site and cut it off
    specs = mk_specs([max(w, 1) for w in widths], ntips=ntips, seed=seed)
    return with_cats([(t[:, :w], g[:w], m)
                      for (t, g, m), w in zip(specs, widths)])


def engines(parts):
    """Guarded engines with the partitions' own models, and the multi
    engine over them."""
    guards = []
    for tips, wgt, mdl, cptr, rates in parts:
        g = GuardedCat(np.ascontiguousarray(tips), wgt, cptr, rates)
        g.eng.model = mdl
        g.eng.upload_model()
        guards.append(g)
    return guards, ea.MultiDnaCatEngine([g.eng for g in guards])


def per_partition(entries, qz, rz, m):
    return [ea.TravEntry(e.tipCase, e.pNumber, e.qNumber, e.rNumber,
                         e.x1Slot, e.x2Slot, e.x3Slot, qz[i, m], rz[i, m])
            for i, e in enumerate(entries)]


def run_full(tree, parts, active=None, qz=None, rz=None, zroot=None,
             min_launches=1):
    """One full traversal of all partitions against the oracle replay of
    each; -> the oracle's scaler counts per partition."""
    entries, (p, q, z) = tree.full_traversal()
    ntips = parts[0][0].shape[0] - 1
    guards, multi = engines(parts)
    idle = [t.shape[1] == 0 or (active is not None and not active[m])
            for m, (t, *_) in enumerate(parts)]
    for g, off in zip(guards, idle):
        if off:                     # a finalize that ran would overwrite it
            g.eng.d_scalers.fill_(7)
    multi.newview_traversal(entries, active=active, qz_ov=qz, rz_ov=rz)
    assert multi.fused_launches() >= min_launches
    scs = []
    for m, (g, (tips, wgt, mdl, cptr, rates)) in enumerate(zip(guards, parts)):
        clv, sc, guard_ok = g.state()
        assert guard_ok, "a kernel wrote past the end of a CLV pool"
        if idle[m]:
            assert (clv == SENTINEL).all() and (sc == 7).all(), m
            scs.append(None)
            continue
        zm = z if zroot is None else zroot[m]
        ent = entries if qz is None else per_partition(entries, qz, rz, m)
        ref, clv_ref, sc_ref = H.oracle_cat_full_lnl(
            ent, (p, q, zm), tree, mdl, np.ascontiguousarray(tips), wgt, cptr,
            rates, return_state=True)
        assert_state(g, clv_ref, sc_ref, ntips)
        lnl = g.eng.evaluate_root(tree, p, q, zm).item()
        print(f"partition {m}: lnL {lnl!r} oracle {ref!r}")
        assert abs(lnl - ref) <= 1e-11 * abs(ref)
        scs.append(sc_ref)
    return scs, entries


@pytest.mark.gpu
@pytest.mark.parametrize("ntips", [6, 12])
@pytest.mark.parametrize("name", ["one", "ragged", "three"])
def test_widths_and_category_counts(name, ntips):
    run_full(ea.PhyloTree.random(ntips, seed=11, rng_z=True),
             specs_for(case_widths(name), ntips=ntips))


@pytest.mark.gpu
def test_rescales_from_the_lds_stack_in_two_partitions():
    tree = cherry_caterpillar(70, H.DEEP_Z)
    tips, wgt = H.random_tips(tree.ntips, 37, H.DNA_BASES, seed=7)
    cptr, rates = categories(37)
    scs, entries = run_full(tree, [(tips, wgt, model(), cptr, rates),
                                   (tips, wgt + 2, model(), cptr, rates)])
    depth = check_plan(entries)["op_depth"]
    for sc in scs:
        assert [i for i, e in enumerate(entries)
                if e.tipCase == ea.INNER_INNER and depth[i] >= 2 and
                sc[e.pNumber] > sc[e.qNumber] + sc[e.rNumber]], \
            "no rescale happened at stack depth >= 2"
    assert not np.array_equal(scs[0], scs[1])


@pytest.mark.gpu
@pytest.mark.parametrize("active", [(0, 1, 1), (0, 0, 0)])
def test_masked_partitions_keep_sentinels_and_scalers(active):
    run_full(ea.PhyloTree.random(12, seed=31, rng_z=True),
             specs_for((150, tile() + 9, 64)), active=active)


@pytest.mark.gpu
def test_per_partition_branch_lengths():
    tree = ea.PhyloTree.random(12, seed=31, rng_z=True)
    entries, (_, _, z) = tree.full_traversal()
    rng = np.random.default_rng(9)
    f = rng.uniform(0.7, 1.3, (2, len(entries), 2))
    qz = np.clip(np.array([e.qz for e in entries])[:, None] * f[0], 1e-6,
                 0.999)
    rz = np.clip(np.array([e.rz for e in entries])[:, None] * f[1], 1e-6,
                 0.999)
    run_full(tree, specs_for((300, tile() + 3)), qz=qz, rz=rz,
             zroot=(min(z * 0.9, 0.999), min(z * 1.1, 0.999)))


@pytest.mark.gpu
def test_tree_deeper_than_the_stack_takes_several_launches():
    run_full(deep_stack_tree(fused_depth() + 1),
             specs_for((65, 200), ntips=50, seed=9), min_launches=2)


@pytest.mark.gpu
def test_graph_replays_partial_and_one_entry_lists_on_a_side_stream():
    """A sequence on one handle against stateful oracle engines, on a side
    stream (the executors never capture on the null stream): the full list
    captured and replayed, replayed after set_site_rates wrote new
    categories, captured anew after a new category tensor at a new address
    with another numCats on partition 1 and replayed again; then a partial
    and a one-entry list (too short for a graph), operands from the pool.
    Every pool is zeroed before every full-list call, so a replay that did
    not run, or ran with the old categories, cannot pass."""
    import torch
    ntips = 12
    tree = ea.PhyloTree.random(ntips, seed=5, rng_z=True)
    parts = specs_for((65, tile() + 1, 130), seed=13)
    guards, multi = engines(parts)
    orcs = [H.OracleCatEngine(np.ascontiguousarray(t), w, m, c, r)
            for t, w, m, c, r in parts]
    entries, (p, q, z) = tree.full_traversal()
    full = check_plan(entries)["launches"]
    assert len(entries) >= 8

    def run(lst, launches, zero=True):
        for g in guards if zero else ():
            g.buf[:g.m].zero_()
        multi.newview_traversal(lst)
        assert multi.fused_launches() == launches
        for g, o in zip(guards, orcs):
            o.newview_traversal(lst)
            assert_state(g, o.clv, o.scalers, ntips)
            ref = o.evaluate_root(tree, p, q, z)
            assert abs(g.eng.evaluate_root(tree, p, q, z).item() - ref) \
                <= 1e-11 * abs(ref)

    L = ea.lib()
    st = torch.cuda.Stream(device="cuda:0")
    st.wait_stream(torch.cuda.current_stream())
    try:
        L.examl_hip_graphs_clear()
        L.examl_hip_use_graphs(1)
        with torch.cuda.stream(st):
            run(entries, full)              # capture + launch
            run(entries, full)              # replay
            for seed in (2, 3):             # replays read the new categories
                for x in (guards[0].eng, orcs[0]):
                    x.set_site_rates(categories(65, 25, seed)[0], parts[0][4])
                run(entries, full)
            old = guards[1].eng.d_cptr      # stays alive: address not reused
            guards[1].eng.d_cptr = torch.empty_like(old)
            for x in (guards[1].eng, orcs[1]):
                x.set_site_rates(*categories(tile() + 1, 7, 5))
            assert old.data_ptr() != guards[1].eng.d_cptr.data_ptr()
            assert [e.num_cats for e in multi.engines] == [25, 7, 7]
            run(entries, full)              # new key: captured anew
            run(entries, full)              # and replayed
            last = entries[-1]
            run(entries[-3:], check_plan(entries[-3:])["launches"], zero=False)
            run([ea.TravEntry(last.tipCase, last.pNumber, last.qNumber,
                              last.rNumber, last.x1Slot, last.x2Slot,
                              last.x3Slot, 0.37, 0.21)], 1, zero=False)
        st.synchronize()
    finally:
        L.examl_hip_graphs_clear()


def snapshot(guards):
    out = []
    for g in guards:
        clv, sc, guard_ok = g.state()
        assert guard_ok
        out.append((clv.copy(), sc.copy()))
    return out


@pytest.mark.gpu
def test_grid_wrap_and_streaming_switch_on_against_off():
    """Tile counts cap - 3, 1 and 11: blocks 0..8 run a tile of partition 0
    and then one of partition 2; partition 0 is past the streaming rule.
    The per-partition engines are pinned to the oracle by test_cat_fused."""
    widths = case_widths("wrap")
    assert widths[0] >= 262144 and sum(widths) < 1_100_000
    parts = specs_for(widths, ntips=4, seed=12)
    tree = ea.PhyloTree.random(4, seed=3, rng_z=True)
    entries, _ = tree.full_traversal()
    got = {}
    try:
        for on in (1, 0):
            ea.lib().examl_hip_multi_use_fused(on)
            guards, multi = engines(parts)
            multi.newview_traversal(entries)
            assert (multi.fused_launches() >= 1) == bool(on)
            got[on] = snapshot(guards)
            del multi, guards
    finally:
        ea.lib().examl_hip_multi_use_fused(1)
    for (clv1, sc1), (clv0, sc0) in zip(got[1], got[0]):
        assert np.array_equal(clv1, clv0) and np.array_equal(sc1, sc0)
        assert not (clv1 == SENTINEL).any()


@pytest.mark.gpu
def test_tree_search_takes_the_on_chip_path():
    from examl_amd.search import TreeSearch
    parts = specs_for((150, tile() + 9, 64))
    got = {}
    try:
        for on in (1, 0):
            ea.lib().examl_hip_multi_use_fused(on)
            guards, _ = engines(parts)
            ts = TreeSearch(ea.PhyloTree.random(12, seed=31, rng_z=True),
                            [g.eng for g in guards], rate_het="CAT")
            lnl = ts.evaluate_generic(full=True)
            assert isinstance(ts.fused_cat, ea.MultiDnaCatEngine)
            assert (ts.fused_cat.fused_launches() > 0) == bool(on)
            got[on] = (lnl, snapshot(guards))
    finally:
        ea.lib().examl_hip_multi_use_fused(1)
    assert got[1][0] == got[0][0], (got[1][0], got[0][0])
    for (clv1, sc1), (clv0, sc0) in zip(got[1][1], got[0][1]):
        assert np.array_equal(clv1, clv0) and np.array_equal(sc1, sc0)


@pytest.mark.gpu
def test_too_many_categories_are_refused():
    parts = specs_for((65, 3))
    guards, multi = engines(parts)
    guards[1].eng.per_site_rates = np.linspace(0.1, 3.0, 26)
    guards[1].eng.num_cats = 26
    entries, _ = ea.PhyloTree.random(12, seed=31).full_traversal()
    with pytest.raises(RuntimeError, match="numCats"):
        multi.newview_traversal(entries)
    assert (guards[0].state()[0] == SENTINEL).all()
    assert multi.fused_launches() == 0
