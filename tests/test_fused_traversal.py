"""Fused DNA GAMMA traversal: the host launch planner (CPU) and the fused
kernel against the oracle replay (GPU).

Planner tests re-simulate the operand stack in pure Python and check, for
every op, the invariant the kernel relies on: an operand is taken on chip
only if the same launch produced it and it is where stack order puts it;
an operand read from the CLV pool was never written by the same launch.

GPU tests compare ALL CLV slots and ALL scaler counts bit for bit with the
oracle, and lnL within the suite's 1e-11 relative tolerance.  The CLV pool
of every engine carries guard doubles behind its last slot.

Rescaling at stack depth >= 2: a DNA CLV loses about 2 bits per tree level,
so no 12-taxon tree reaches the 2^-256 threshold whatever its branch
lengths (the bushy 12-taxon case below runs, matches bit for bit, and is
asserted to reach depth >= 2, but its scalers stay 0).  The property itself
is pinned by `cherry_caterpillar`: a deep chain whose every level joins a
two-tip cherry, so each INNER_INNER op takes the chain operand from the
on-chip stack below the cherry, and rescales.
"""

import ctypes

import numpy as np
import pytest

import examl_amd as ea
from tests import helpers as H

TIP_TIP, TIP_INNER, INNER_INNER = ea.TIP_TIP, ea.TIP_INNER, ea.INNER_INNER
GUARD = 64
SENTINEL = -7.0e77
WIDTHS = (1, 3, 63, 65, 333)


# ---------------------------------------------------------------------------
# planner plumbing and the pure-Python stack simulation
# ---------------------------------------------------------------------------

def fused_depth():
    return ea.lib().examl_hip_fused_depth()


def plan(entries, depth=None):
    """-> (number of launches, launch_of_op, src1, src2)"""
    depth = depth or fused_depth()
    n = len(entries)
    arr = (ea.TravEntry * n)(*entries)
    lo, s1, s2 = ((ctypes.c_int * n)() for _ in range(3))
    nl = ea.lib().examl_hip_fused_plan(
        ctypes.cast(arr, ctypes.c_void_p), n, depth,
        ctypes.cast(lo, ctypes.c_void_p), ctypes.cast(s1, ctypes.c_void_p),
        ctypes.cast(s2, ctypes.c_void_p))
    return nl, list(lo), list(s1), list(s2)


def free_stack_depth(entries):
    """Peak depth of an unbounded operand stack, or None when the list is
    not in stack order."""
    stack, peak = [], 0
    for e in entries:
        if e.tipCase == TIP_INNER:
            if not stack or stack.pop() != e.x2Slot:
                return None
        elif e.tipCase == INNER_INNER:
            if len(stack) < 2 or stack.pop() != e.x2Slot or \
                    stack.pop() != e.x1Slot:
                return None
        stack.append(e.x3Slot)
        peak = max(peak, len(stack))
    return peak


def check_plan(entries, depth=None):
    """Validate a plan against an independent stack simulation.  Returns a
    dict of statistics (launches, peak depth, evictions, on-chip operands,
    the per-op depth at which each op ran)."""
    depth = depth or fused_depth()
    nl, launch, s1, s2 = plan(entries, depth)
    n = len(entries)
    assert nl >= 1
    # launches partition the list in order
    assert launch[0] == 0 and launch[-1] == nl - 1
    assert all(0 <= launch[i + 1] - launch[i] <= 1 for i in range(n - 1))
    max_ops = ea.lib().examl_hip_fused_max_ops()
    assert max(np.bincount(launch)) <= max_ops

    last_prod = {}          # clv slot -> op that produced it last
    stack = []              # live entries (position, clv slot, op)
    written = set()         # clv slots written by the current launch
    nxt = 0                 # next stack position
    stats = dict(launches=nl, peak=0, evictions=0, on_chip=0, mem=0,
                 op_depth=[])
    for i, e in enumerate(entries):
        if i == 0 or launch[i] != launch[i - 1]:
            stack, written, nxt = [], set(), 0
        stats["op_depth"].append(len(stack))
        # tip operands are never on chip
        if e.tipCase != INNER_INNER:
            assert s1[i] == -1
        if e.tipCase == TIP_TIP:
            assert s2[i] == -1
        inner = []
        if e.tipCase != TIP_TIP:
            inner.append((e.x2Slot, s2[i]))
        if e.tipCase == INNER_INNER:
            inner.append((e.x1Slot, s1[i]))
        for clv, src in inner:          # x2 first: it is on top
            if src == -1:
                # pool read: the launch must not have written it
                assert clv not in written, \
                    f"op {i} reads slot {clv} back through the pool"
                stats["mem"] += 1
            else:
                assert stack, f"op {i}: on-chip operand, empty stack"
                pos, sclv, sop = stack.pop()
                nxt = pos
                assert src == pos % depth
                assert sclv == clv and sop == last_prod[clv], \
                    f"op {i}: slot {src} does not hold CLV {clv}"
                stats["on_chip"] += 1
        stack.append((nxt, e.x3Slot, i))
        nxt += 1
        if len(stack) > depth:
            stack.pop(0)
            stats["evictions"] += 1
        stats["peak"] = max(stats["peak"], len(stack))
        written.add(e.x3Slot)
        last_prod[e.x3Slot] = i
    stats["plan"] = (launch, s1, s2)
    return stats


def inner_operands(entries):
    return sum((e.tipCase != TIP_TIP) + (e.tipCase == INNER_INNER)
               for e in entries)


def deep_stack_tree(min_depth):
    """First seeded random 50-taxon tree whose free stack depth reaches
    min_depth."""
    for seed in range(2000, 2400):
        t = ea.PhyloTree.random(50, seed=seed, rng_z=True)
        if free_stack_depth(t.full_traversal()[0]) >= min_depth:
            return t
    raise AssertionError("no deep-stack tree among the seeds")


def cherry_caterpillar(levels, z):
    """Tip 1 on top of a chain of `levels` nodes; every chain node joins the
    chain below it with a two-tip cherry, the last one joins two cherries.
    2*levels + 3 tips."""
    ntips = 2 * levels + 3
    t = ea.PhyloTree(ntips)
    nxt_tip, nxt_inner = 2, ntips + 1

    def cherry():
        nonlocal nxt_tip, nxt_inner
        h = nxt_inner
        nxt_inner += 1
        t.add_edge(h, nxt_tip, z)
        t.add_edge(h, nxt_tip + 1, z)
        nxt_tip += 2
        return h

    chain = []
    for _ in range(levels):
        chain.append(nxt_inner)
        nxt_inner += 1
    t.add_edge(1, chain[0], z)
    for k, c in enumerate(chain):
        below = chain[k + 1] if k + 1 < levels else cherry()
        t.add_edge(c, below, z)        # chain side first: it is q
        t.add_edge(c, cherry(), z)
    assert nxt_tip == ntips + 1 and nxt_inner == 2 * ntips - 1
    return t


def root_path_partial(tree, leaf_inner):
    """Entries (in traversal order) of the proper ancestors of inner node
    `leaf_inner` in the default full traversal."""
    entries, root = tree.full_traversal()
    parent = {}
    for e in entries:
        parent[e.qNumber] = e.pNumber
        parent[e.rNumber] = e.pNumber
    chain, v = set(), leaf_inner
    while v in parent:
        v = parent[v]
        chain.add(v)
    return [e for e in entries if e.pNumber in chain], root


# ---------------------------------------------------------------------------
# CPU: planner
# ---------------------------------------------------------------------------

def test_plan_bench_tree_is_one_launch_depth_3():
    entries, _ = ea.PhyloTree.random(50, seed=7).full_traversal()
    st = check_plan(entries)
    assert st["launches"] == 1
    assert st["peak"] == 3 == free_stack_depth(entries)
    assert st["evictions"] == 0 and st["mem"] == 0
    assert st["on_chip"] == inner_operands(entries)


def test_plan_200_random_trees():
    depth = fused_depth()
    for seed in range(200):
        entries, _ = ea.PhyloTree.random(50, seed=1000 + seed).full_traversal()
        st = check_plan(entries)
        free = free_stack_depth(entries)
        assert free is not None
        if free <= depth:
            assert st["launches"] == 1 and st["mem"] == 0
        else:
            assert st["launches"] > 1 or st["evictions"] > 0


def test_plan_caterpillar():
    entries, _ = ea.PhyloTree.caterpillar(50).full_traversal()
    st = check_plan(entries)
    assert st["launches"] == 1 and st["peak"] == 1 and st["mem"] == 0


@pytest.mark.parametrize("depth", [1, 2])
def test_plan_bench_tree_on_a_shallower_stack(depth):
    entries, _ = ea.PhyloTree.random(50, seed=7).full_traversal()
    assert free_stack_depth(entries) > depth
    st = check_plan(entries, depth)
    assert st["launches"] > 1 and st["evictions"] > 0


def test_plan_tree_deeper_than_the_kernel_stack():
    tree = deep_stack_tree(fused_depth() + 1)
    st = check_plan(tree.full_traversal()[0])
    assert st["launches"] > 1 and st["evictions"] > 0 and st["mem"] > 0


def test_plan_long_list_is_cut_at_the_argument_limit():
    entries, _ = ea.PhyloTree.caterpillar(500).full_traversal()
    st = check_plan(entries)
    max_ops = ea.lib().examl_hip_fused_max_ops()
    assert st["launches"] == -(-len(entries) // max_ops)


def test_plan_partial_list_reads_outside_operands_from_the_pool():
    tree = ea.PhyloTree.random(12, seed=5, rng_z=True)
    entries, _ = tree.full_traversal()
    first = next(e for e in entries if e.tipCase == TIP_TIP)
    part, _ = root_path_partial(tree, first.pNumber)
    assert len(part) >= 3
    st = check_plan(part)
    launch, s1, s2 = st["plan"]
    in_list = {e.x3Slot for e in part}
    for i, e in enumerate(part):
        if e.tipCase != TIP_TIP and e.x2Slot not in in_list:
            assert s2[i] == -1
        if e.tipCase == INNER_INNER and e.x1Slot not in in_list:
            assert s1[i] == -1
    assert st["launches"] == 1
    # the chain itself stays on chip
    assert st["on_chip"] == len(part) - 1


def test_plan_out_of_stack_order_list_is_still_valid():
    entries, _ = ea.PhyloTree.random(50, seed=7).full_traversal()
    k = next(i for i, e in enumerate(entries) if e.tipCase == INNER_INNER)
    e = entries[k]
    e.x1Slot, e.x2Slot = e.x2Slot, e.x1Slot
    e.qNumber, e.rNumber = e.rNumber, e.qNumber
    e.qz, e.rz = e.rz, e.qz
    assert free_stack_depth(entries) is None
    st = check_plan(entries)
    assert st["launches"] >= 2
    # a child used before the entry on top of it: [A, B, parent-of-A]
    a, b, c = ea.TravEntry(), ea.TravEntry(), ea.TravEntry()
    for x, (p, q, r, slot) in ((a, (7, 1, 2, 0)), (b, (8, 3, 4, 1))):
        x.tipCase, x.pNumber, x.qNumber, x.rNumber = TIP_TIP, p, q, r
        x.x1Slot, x.x2Slot, x.x3Slot, x.qz, x.rz = q, r, slot, 0.5, 0.5
    c.tipCase, c.pNumber, c.qNumber, c.rNumber = TIP_INNER, 9, 5, 7
    c.x1Slot, c.x2Slot, c.x3Slot, c.qz, c.rz = 5, 0, 2, 0.5, 0.5
    st = check_plan([a, b, c])
    assert st["launches"] == 2 and st["mem"] == 1


def test_plan_rejects_a_malformed_list():
    entries, _ = ea.PhyloTree.random(6, seed=1).full_traversal()
    entries[1].tipCase = 7
    assert plan(entries)[0] == -1


# ---------------------------------------------------------------------------
# GPU: fused kernel against the oracle
# ---------------------------------------------------------------------------

def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch, "cuda:0"


def model():
    return ea.DnaGtrModel([0.3, 0.2, 0.2, 0.3],
                          [1.1, 2.2, 0.7, 0.9, 3.1, 1.0], alpha=0.7)


class Guarded:
    """DnaGammaEngine whose CLV pool is followed by sentinel doubles."""

    def __init__(self, tips, wgt, mdl):
        torch, dev = _torch()
        self.torch = torch
        self.eng = ea.DnaGammaEngine(tips, wgt, mdl, device=dev)
        shape = self.eng.d_clv.shape
        self.m = shape[0] * shape[1]
        self.buf = torch.full((self.m + GUARD,), SENTINEL,
                              dtype=torch.float64, device=dev)
        self.eng.d_clv = self.buf[:self.m].view(shape)

    def state(self):
        """(clv [ninner, width*16], scalers, guard untouched?)"""
        out = self.buf.cpu().numpy()
        return (out[:self.m].reshape(self.eng.d_clv.shape),
                self.eng.d_scalers.cpu().numpy(),
                bool((out[self.m:] == SENTINEL).all()))


def assert_state(g, clv_ref, scalers_ref, ntips):
    clv, sc, guard_ok = g.state()
    assert guard_ok, "a kernel wrote past the end of the CLV pool"
    for slot, x in clv_ref.items():
        assert np.array_equal(clv[slot], x), f"CLV slot {slot} differs"
    for node in range(1, 2 * ntips - 1):
        assert sc[node] == scalers_ref[node], f"scaler of node {node}"


def run_full(tree, tips, wgt, mdl=None, want_launches=None):
    """Fused full traversal + root evaluate against the oracle replay."""
    mdl = mdl or model()
    ntips = tips.shape[0] - 1
    entries, root = tree.full_traversal()
    st = check_plan(entries)
    launch = st["plan"][0]
    assert max(np.bincount(launch)) >= 2, "the fused kernel would not run"
    if want_launches is not None:
        assert want_launches(st["launches"])
    g = Guarded(tips, wgt, mdl)
    lnl = g.eng.full_lnl(tree).item()
    ref, clv_ref, sc_ref = H.oracle_full_lnl(entries, root, tree, mdl, tips,
                                             wgt, return_state=True)
    assert len(clv_ref) == ntips - 2
    assert_state(g, clv_ref, sc_ref, ntips)
    assert abs(lnl - ref) <= 1e-11 * abs(ref)
    return st, sc_ref, entries


@pytest.mark.gpu
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("ntips", [6, 12])
def test_fused_ragged_widths(ntips, width):
    tips, wgt = H.make_synthetic(ntips, width, seed=3 + ntips)
    tree = ea.PhyloTree.random(ntips, seed=11, rng_z=True)
    run_full(tree, tips, wgt)


@pytest.mark.gpu
def test_fused_deep_caterpillar_rescales():
    # the last model of helpers.fused_deep_inputs: with it several of 37
    # random sites cross the threshold within 120 levels (checked on the
    # oracle; the flatter frequencies of model() never get there)
    ntips, parts = H.fused_deep_inputs(4)
    assert ntips == 120
    tips, wgt = H.random_tips(ntips, 37, H.DNA_BASES, seed=5)
    _, sc_ref, _ = run_full(H.deep_caterpillar(ntips), tips, wgt,
                            mdl=parts[3][2])
    assert sc_ref.max() > 0 and (sc_ref > 0).sum() > 1


@pytest.mark.gpu
def test_fused_bushy_12_short_z():
    tips, wgt = H.random_tips(12, 37, H.DNA_BASES, seed=6)
    tree = ea.PhyloTree.random(12, seed=4, z=H.DEEP_Z)
    st, _, _ = run_full(tree, tips, wgt)
    assert st["peak"] >= 2


@pytest.mark.gpu
def test_fused_rescales_at_stack_depth_2():
    tree = cherry_caterpillar(70, H.DEEP_Z)
    tips, wgt = H.random_tips(tree.ntips, 37, H.DNA_BASES, seed=7)
    st, sc_ref, entries = run_full(tree, tips, wgt)
    assert sc_ref.max() > 0
    # ops that rescaled (own increment > 0) while something else was
    # waiting below their operands, one operand coming from the LDS stack
    deep = [i for i, e in enumerate(entries)
            if e.tipCase == INNER_INNER and st["op_depth"][i] >= 2 and
            sc_ref[e.pNumber] > sc_ref[e.qNumber] + sc_ref[e.rNumber]]
    assert deep, "no rescale happened at stack depth >= 2"


@pytest.mark.gpu
def test_fused_tree_deeper_than_stack_runs_several_launches():
    tree = deep_stack_tree(fused_depth() + 1)
    tips, wgt = H.make_synthetic(50, 65, seed=9)
    run_full(tree, tips, wgt, want_launches=lambda nl: nl >= 2)


@pytest.mark.gpu
def test_fused_partial_traversal_reads_the_pool():
    ntips, width = 12, 65
    mdl = model()
    tips, wgt = H.make_synthetic(ntips, width, seed=13)
    tree = ea.PhyloTree.random(ntips, seed=5, rng_z=True)
    entries, root = tree.full_traversal()
    g = Guarded(tips, wgt, mdl)
    orc = H.OracleEngine(tips, wgt, mdl)
    g.eng.newview_traversal(entries)
    orc.newview_traversal(entries)
    # new branch lengths on one root path, then only its entries
    first = next(e for e in entries if e.tipCase == TIP_TIP)
    part, _ = root_path_partial(tree, first.pNumber)
    for k, e in enumerate(part):
        tree.set_z(e.pNumber, e.qNumber, 0.31 + 0.05 * k)
    part, _ = root_path_partial(tree, first.pNumber)
    st = check_plan(part)
    assert len(part) >= 3 and st["launches"] == 1 and st["mem"] >= 1
    g.eng.newview_traversal(part)
    orc.newview_traversal(part)
    assert_state(g, orc.clv, orc.scalers, ntips)
    p, q, z = root
    lnl = g.eng.evaluate_root(tree, p, q, z).item()
    ref = orc.evaluate_root(tree, p, q, z)
    assert abs(lnl - ref) <= 1e-11 * abs(ref)


@pytest.mark.gpu
def test_fused_on_and_off_give_identical_arrays():
    ntips, width = 50, 333
    tips, wgt = H.make_synthetic(ntips, width, seed=17)
    tree = ea.PhyloTree.random(ntips, seed=7, rng_z=True)
    got = {}
    try:
        for on in (0, 1):
            ea.lib().examl_hip_use_fused(on)
            g = Guarded(tips, wgt, model())
            lnl = g.eng.full_lnl(tree).item()
            clv, sc, guard_ok = g.state()
            assert guard_ok
            got[on] = (clv.copy(), sc.copy(), lnl)
    finally:
        ea.lib().examl_hip_use_fused(1)
    assert np.array_equal(got[0][0], got[1][0])
    assert np.array_equal(got[0][1], got[1][1])
    assert got[0][2] == got[1][2]


@pytest.mark.gpu
def test_fused_tile_wrap():
    """One grid stride of the fused kernel plus a partial last tile."""
    L = ea.lib()
    tile = L.examl_hip_fused_tile_sites()
    width = L.examl_hip_fused_grid_cap() * tile + 1037
    assert width <= 526000 and width % tile != 0
    tips, wgt = H.make_synthetic(4, width, seed=12)
    tree = ea.PhyloTree.random(4, seed=3, rng_z=True)
    run_full(tree, tips, wgt, want_launches=lambda nl: nl == 1)
