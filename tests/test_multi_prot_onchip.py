"""On-chip multi-partition protein GAMMA traversal
(k_prot_gamma_tables_mseg + k_newview_prot_gamma_mseg_fused) against the
level path on the same handle.

Both paths read the same device P blocks and sum in the same order, so every
case demands IDENTICAL CLV pools, scaler arrays and per-partition lnL
(np.array_equal), untouched sentinels behind every pool, and the launch
counter: >= 1 with the path on, 0 with it off.  Helpers are those of
tests/test_multi_onchip.py and tests/test_fused_traversal.py."""

import os

import numpy as np
import pytest

import examl_amd as ea
from tests import helpers as H
from tests.test_fused_traversal import Guarded, check_plan, deep_stack_tree
from tests.test_multi_onchip import (assert_identical, call, rescaled,
                                     tile_table)

pytestmark = pytest.mark.gpu


def tile():
    return ea.lib().examl_hip_prot_gamma_fused_tile_sites()


def depth():
    return ea.lib().examl_hip_prot_gamma_fused_depth()


def grid_cap():
    return ea.lib().examl_hip_multi_prot_fused_grid_cap()


def mk_specs(widths, ntips=12, seed=5):
    """(tips, wgt, model) per partition, the distinct AA models of
    test_multi_fused._mk(states=20)."""
    rng = np.random.default_rng(seed)
    aa = np.load(os.path.join(os.path.dirname(ea.__file__), "data",
                              "aa_models.npz"))
    return [H.random_tips(ntips, w, H.AA_CODES, seed + i) +
            (ea.ProtGtrModel(aa["frequencies"][4 + i % 3],
                             aa["rates190"][4 + i % 3],
                             float(rng.uniform(0.4, 1.2))),)
            for i, w in enumerate(widths)]


def run_calls(specs, calls, switch, fast=0):
    """test_multi_onchip.run_calls for 20-state engines: fresh guarded
    engines and one handle, `switch` = examl_hip_multi_use_fused per call.
    -> per call ([clv pools], [scalers], lnL vector), and
    prot_fused_launches() after every traversal."""
    L = ea.lib()
    if isinstance(switch, int):
        switch = [switch] * len(calls)
    snaps, counts = [], []
    try:
        L.examl_hip_fast_math(fast)
        guards = [Guarded(t, w, m) for t, w, m in specs]
        multi = ea.MultiEngine([g.eng for g in guards])
        for c, on in zip(calls, switch):
            L.examl_hip_use_fused(1)
            L.examl_hip_multi_use_fused(on)
            multi.newview_traversal(c.entries, active=c.active, qz_ov=c.qz,
                                    rz_ov=c.rz)
            counts.append(multi.prot_fused_launches())
            assert multi.fused_launches() == 0    # the DNA kernel's counter
            lnl = multi.evaluate_root(c.tree, c.p, c.q,
                                      c.z).cpu().numpy().copy()
            states = [g.state() for g in guards]
            assert all(ok for _, _, ok in states), \
                "a kernel wrote past the end of a CLV pool"
            snaps.append(([s[0].copy() for s in states],
                          [s[1].copy() for s in states], lnl))
        del multi
    finally:
        L.examl_hip_fast_math(0)
        L.examl_hip_use_fused(1)
        L.examl_hip_multi_use_fused(1)
    return snaps, counts


def on_and_off(specs, calls, fast=0):
    on, n_on = run_calls(specs, calls, 1, fast)
    off, n_off = run_calls(specs, calls, 0, fast)
    print("on-chip launches per call:", n_on, "level path:", n_off)
    assert all(n >= 1 for n in n_on), n_on
    assert all(n == 0 for n in n_off), n_off
    for a, b in zip(on, off):
        assert_identical(a, b)
    return on, off, n_on


def bushy(seed=31):
    return ea.PhyloTree.random(12, seed=seed, rng_z=True)


@pytest.mark.parametrize("fast", [0, 1])
def test_ragged_widths_around_the_tile(fast):
    t = tile()
    widths = (1, t - 1, t, t + 1, 0, 2 * t + 6)
    specs = mk_specs(widths)
    c = call(bushy())
    on, _, _ = on_and_off(specs, [c], fast)
    for i, (tips, wgt, mdl) in enumerate(specs):
        got = on[0][2][i]
        if widths[i] == 0:
            assert got == 0.0
            continue
        orc = H.OracleEngine(tips, wgt, mdl)
        orc.newview_traversal(c.entries)
        ref = orc.evaluate_root(c.tree, c.p, c.q, c.z)
        print(f"partition {i} (width {widths[i]}): oracle {ref!r} "
              f"on-chip {got!r}")
        assert abs(got - ref) <= 1e-11 * abs(ref), (i, ref, got)


def test_deep_caterpillar_rescales():
    ntips, parts = H.fused_deep_inputs(20)
    on, off, _ = on_and_off(parts, [call(H.deep_caterpillar(ntips))])
    for side in (on, off):
        assert max(int(sc.max()) for sc in side[0][1]) > 0


def test_masked_partitions_stay_untouched():
    specs = mk_specs((40, tile() + 1, 17, 70))
    first = call(bushy())
    second = call(first.tree, entries=rescaled(first.entries, 0.8, 0.9),
                  root=(first.p, first.q, first.z), active=[1, 0, 1, 0])
    on, off, _ = on_and_off(specs, [first, second])
    for i in (1, 3):     # masked: byte-identical to before the second call
        assert np.array_equal(on[1][0][i], on[0][0][i])
        assert np.array_equal(on[1][1][i], on[0][1][i])
    for i in (0, 2):     # active: the second call did run
        assert not np.array_equal(on[1][0][i], on[0][0][i])


def test_per_partition_branch_lengths():
    specs = mk_specs((tile() + 3, 50))
    c = call(bushy())
    rng = np.random.default_rng(9)
    n = len(c.entries)
    qz = np.clip([[e.qz] * 2 for e in c.entries] *
                 rng.uniform(0.7, 1.3, (n, 2)), 1e-6, 0.999)
    rz = np.clip([[e.rz] * 2 for e in c.entries] *
                 rng.uniform(0.7, 1.3, (n, 2)), 1e-6, 0.999)
    zroot = np.clip([c.z * 0.9, c.z * 1.1], 1e-6, 0.999)
    on, _, _ = on_and_off(specs, [call(c.tree, qz=qz, rz=rz, zroot=zroot)])
    joint, _ = run_calls(specs, [c], 1)
    assert not np.array_equal(on[0][0][0], joint[0][0][0])


def test_tree_deeper_than_the_stack_takes_several_launches():
    tree = deep_stack_tree(depth() + 1)
    specs = mk_specs((tile() + 1, 9), ntips=tree.ntips, seed=9)
    _, _, n_on = on_and_off(specs, [call(tree)])
    assert n_on[0] >= 2


def test_one_entry_launch_runs_the_level_kernel():
    """A list the planner cuts into launches of 6, 3 and 1 entries.  The
    last one, the root-most INNER_INNER entry with its children named the
    other way round, goes through k_newview_prot_mseg inside the on-chip
    dispatch and reads both operands from the pool."""
    c = call(bushy(seed=8))
    e = c.entries[-1]
    assert e.tipCase == ea.INNER_INNER
    e.x1Slot, e.x2Slot = e.x2Slot, e.x1Slot
    e.qNumber, e.rNumber = e.rNumber, e.qNumber
    e.qz, e.rz = e.rz, e.qz
    sizes = list(np.bincount(check_plan(c.entries, depth())["plan"][0]))
    assert sizes == [6, 3, 1], sizes
    _, _, n_on = on_and_off(mk_specs((tile() + 1, 20, 33), seed=17), [c])
    assert n_on[0] == 2      # the one-entry launch is not an on-chip one


def test_grid_stride_wrap_restages_ev():
    """Tile counts cap - 3, 1 and 11: blocks 0..7 run a tile of partition 0
    and then one of partition 2 with another model."""
    t, cap = tile(), grid_cap()
    widths = ((cap - 3) * t - 5, 1, 11 * t - 7)
    rc, part, _ = tile_table(widths, tile=t)
    assert rc == cap + 9 and part[0] != part[cap]
    on_and_off(mk_specs(widths, ntips=4, seed=12),
               [call(ea.PhyloTree.random(4, seed=3, rng_z=True))])


def test_graph_replay_and_switching():
    specs = mk_specs((tile() + 1, 20, 33))
    base = call(bushy())
    calls = [call(base.tree, entries=rescaled(base.entries, f, 2 - f),
                  root=(base.p, base.q, base.z))
             for f in (1.0, 0.9, 0.8, 0.7, 0.95)]
    got, n = run_calls(specs, calls, [1, 1, 1, 0, 1])
    ref, n_ref = run_calls(specs, calls, 0)
    assert n[3] == 0 and all(k >= 1 for k in n[:3] + n[4:]), n
    assert n_ref == [0] * 5
    for a, b in zip(got, ref):
        assert_identical(a, b)
    assert not np.array_equal(got[0][0][0], got[1][0][0])
