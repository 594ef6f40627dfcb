"""On-chip protein GAMMA traversal (k_newview_prot_gamma_fused) against the
OracleEngine replay of the same entry list: ALL CLV slots and scaler counts
bit for bit, lnL within the suite's 1e-11 relative, guard doubles behind the
CLV pool untouched, and examl_hip_prot_gamma_fused_launches() telling that
the kernel really ran.  Trees and planner checks are those of
tests/test_fused_traversal.py."""

import numpy as np
import pytest

import examl_amd as ea
from tests import helpers as H
from tests.test_fused_traversal import (Guarded, assert_state, check_plan,
                                        cherry_caterpillar, deep_stack_tree,
                                        root_path_partial)

pytestmark = pytest.mark.gpu

ALL_CODES = tuple(range(1, 23))   # 20 amino acids, B/Z ambiguity, undetermined
# Rescaling, sized on the oracle alone at width 37 and z = DEEP_Z: the
# caterpillar first rescales at 56 tips; at 60 tips 5 nodes carry a count
# (largest 56).  cherry_caterpillar(28) (59 tips) rescales at 2 INNER_INNER
# entries whose chain operand sits below the cherry (26 levels: none): at
# plan depth 2 with a stack, read from the pool when planned with depth 1.
DEEP_TIPS, CHERRY_LEVELS, DEEP_WIDTH = 60, 28, 37


def L():
    return ea.lib()


def tile():
    return L().examl_hip_prot_gamma_fused_tile_sites()


def depth():
    return L().examl_hip_prot_gamma_fused_depth()


def model():
    return H.prot_cat_inputs(4, 4, 0)[2]


def run_full(tree, tips, wgt, min_launches=1):
    """Full traversal + root evaluate against the oracle replay."""
    entries, (p, q, z) = tree.full_traversal()
    g = Guarded(tips, wgt, model())
    lnl = g.eng.full_lnl(tree).item()
    assert L().examl_hip_prot_gamma_fused_launches() >= min_launches
    orc = H.OracleEngine(tips, wgt, model())
    orc.newview_traversal(entries)
    assert_state(g, orc.clv, orc.scalers, tips.shape[0] - 1)
    ref = orc.evaluate_root(tree, p, q, z)
    assert abs(lnl - ref) <= 1e-11 * abs(ref)
    return orc.scalers, entries


@pytest.mark.parametrize("ntips", [6, 12])
@pytest.mark.parametrize("width", [1, 3, 17, "tile-1", "tile+1"])
def test_ragged_widths(width, ntips):
    if isinstance(width, str):
        width = tile() + int(width[4:])
    tips, wgt = H.random_tips(ntips, width, ALL_CODES, seed=3 + ntips)
    run_full(ea.PhyloTree.random(ntips, seed=11, rng_z=True), tips, wgt)


def test_rescales_down_a_chain():
    """Operands from registers."""
    tips, wgt = H.random_tips(DEEP_TIPS, DEEP_WIDTH, H.AA_CODES, seed=5)
    sc, _ = run_full(H.deep_caterpillar(DEEP_TIPS), tips, wgt)
    assert sc.max() > 1 and (sc > 0).sum() > 1


def test_rescales_below_the_top_of_the_stack():
    """cherry_caterpillar: every chain entry takes the chain operand from
    below the cherry, at plan depth >= 2: from the LDS stack where the kernel
    has one (depth() >= 2), from the pool where it plans with depth 1."""
    tree = cherry_caterpillar(CHERRY_LEVELS, H.DEEP_Z)
    tips, wgt = H.random_tips(tree.ntips, DEEP_WIDTH, H.AA_CODES, seed=7)
    sc, entries = run_full(tree, tips, wgt)
    assert sc.max() > 1
    st = check_plan(entries, depth())
    at, s1 = st["op_depth"], st["plan"][1]
    assert [i for i, e in enumerate(entries)
            if e.tipCase == ea.INNER_INNER and
            sc[e.pNumber] > sc[e.qNumber] + sc[e.rNumber] and
            (at[i] >= 2 if depth() >= 2 else s1[i] == -1)], \
        "no rescale happened at an operand from below the top of the stack"


def test_tree_deeper_than_the_stack_runs_several_launches():
    tips, wgt = H.random_tips(50, 65, ALL_CODES, seed=9)
    run_full(deep_stack_tree(depth() + 1), tips, wgt, min_launches=2)


def test_partial_list_then_full_list_through_the_cached_graph():
    ntips, width = 12, 65
    tips, wgt = H.random_tips(ntips, width, ALL_CODES, seed=13)
    tree = ea.PhyloTree.random(ntips, seed=5, rng_z=True)
    g = Guarded(tips, wgt, model())
    orc = H.OracleEngine(tips, wgt, model())
    entries, _ = tree.full_traversal()
    for x in (g.eng, orc):
        x.newview_traversal(entries)
    # new branch lengths on one root path, then only its entries: operands
    # from outside the list come from the pool
    first = next(e for e in entries if e.tipCase == ea.TIP_TIP)
    for k, e in enumerate(root_path_partial(tree, first.pNumber)[0]):
        tree.set_z(e.pNumber, e.qNumber, 0.31 + 0.05 * k)
    part, _ = root_path_partial(tree, first.pNumber)
    assert len(part) >= 3 and check_plan(part, depth())["mem"] >= 1
    for x in (g.eng, orc):
        x.newview_traversal(part)
    assert L().examl_hip_prot_gamma_fused_launches() >= 1
    assert_state(g, orc.clv, orc.scalers, ntips)
    # the full list again: the graph captured above, with other P blocks
    entries, (p, q, z) = tree.full_traversal()
    for x in (g.eng, orc):
        x.newview_traversal(entries)
    assert L().examl_hip_prot_gamma_fused_launches() >= 1
    assert_state(g, orc.clv, orc.scalers, ntips)
    ref = orc.evaluate_root(tree, p, q, z)
    assert abs(g.eng.evaluate_root(tree, p, q, z).item() - ref) \
        <= 1e-11 * abs(ref)


@pytest.mark.parametrize("fast", [0, 1])
def test_switch_off_and_on_give_identical_arrays(fast):
    """The per-entry kernel is the reference here (the FMA build has no
    oracle): same arrays, same lnL."""
    tips, wgt = H.random_tips(50, 333, ALL_CODES, seed=17)
    tree = ea.PhyloTree.random(50, seed=7, rng_z=True)
    got = {}
    try:
        L().examl_hip_fast_math(fast)
        for on in (0, 1):
            L().examl_hip_use_fused(on)
            g = Guarded(tips, wgt, model())
            lnl = g.eng.full_lnl(tree).item()
            assert (L().examl_hip_prot_gamma_fused_launches() >= 1) == bool(on)
            clv, sc, guard_ok = g.state()
            assert guard_ok
            got[on] = (clv.copy(), sc.copy(), lnl)
    finally:
        L().examl_hip_use_fused(1)
        L().examl_hip_fast_math(0)
    assert np.array_equal(got[0][0], got[1][0])
    assert np.array_equal(got[0][1], got[1][1])
    assert got[0][2] == got[1][2]


def test_grid_wrap():
    """One grid stride plus a ragged last tile."""
    width = L().examl_hip_prot_gamma_fused_grid_cap() * tile() + 1037
    assert tile() * 8 < width < 100_000 and width % tile() != 0
    tips, wgt = H.random_tips(4, width, ALL_CODES, seed=12)
    run_full(ea.PhyloTree.random(4, seed=3, rng_z=True), tips, wgt)
