"""On-chip multi-partition DNA GAMMA traversal (k_newview_dna_mseg_fused):
the tile-table builder (CPU) and the kernel against the level path (GPU).

The on-chip path and the level path share the device P blocks, so the GPU
cases demand IDENTICAL results (np.array_equal) on every partition's CLV
pool, every scaler array and the per-partition lnL vector.  Every engine's
CLV pool is followed by sentinel doubles that must stay untouched, and every
case reads the launch counter: >= 1 with the path on, 0 with it off.
"""

import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import examl_amd as ea
from tests import helpers as H
from tests.test_fused_traversal import (Guarded, check_plan,
                                        cherry_caterpillar, deep_stack_tree,
                                        fused_depth, model,
                                        root_path_partial)
from tests.test_multi_fused import _mk

INNER_INNER = ea.INNER_INNER
MULTI_FUSED_DEFAULT = 1      # the library's default of the switch


# ---------------------------------------------------------------------------
# CPU: tile table
# ---------------------------------------------------------------------------

def tile_sites():
    return ea.lib().examl_hip_fused_tile_sites()


def grid_cap():
    return ea.lib().examl_hip_fused_grid_cap()


def tile_table(widths, cap=None, tile=None):
    """-> (return value, part_of_tile, site0_of_tile)"""
    tile = tile or tile_sites()
    want = sum(-(-w // tile) for w in widths)
    cap = want if cap is None else cap
    n = len(widths)
    w = (ctypes.c_long * max(n, 1))(*widths)
    part = (ctypes.c_int * max(cap, 1))()
    site = (ctypes.c_long * max(cap, 1))()
    rc = ea.lib().examl_hip_multi_tile_table(
        ctypes.cast(w, ctypes.c_void_p), n, tile,
        ctypes.cast(part, ctypes.c_void_p),
        ctypes.cast(site, ctypes.c_void_p), cap)
    return rc, list(part)[:max(rc, 0)], list(site)[:max(rc, 0)]


def check_tile_table(widths):
    tile = tile_sites()
    want_part, want_site = [], []
    for p, w in enumerate(widths):
        for s in range(0, w, tile):
            want_part.append(p)
            want_site.append(s)
    rc, part, site = tile_table(widths)
    assert rc == len(want_part)
    assert part == want_part and site == want_site
    # tiles of a partition are consecutive, in partition order
    assert all(part[i] <= part[i + 1] for i in range(rc - 1))
    assert all(s % tile == 0 for s in site)
    for p, w in enumerate(widths):
        mine = [i for i in range(rc) if part[i] == p]
        if w == 0:
            assert not mine, "a zero-width partition owns a tile"
            continue
        assert mine == list(range(mine[0], mine[0] + -(-w // tile)))
        assert [site[i] for i in mine] == list(range(0, w, tile))
        ragged = w - site[mine[-1]] < tile
        assert ragged == (w % tile != 0)
    if rc > 0:
        assert tile_table(widths, cap=rc - 1)[0] == -1
    return rc


@pytest.mark.parametrize("widths", [(1,), (128, 128), (127, 129, 0, 1),
                                    (0, 0, 5)])
def test_tile_table_small_lists(widths):
    check_tile_table(widths)


def test_tile_table_50_random_lists():
    rng = np.random.default_rng(2024)
    tile = tile_sites()
    for _ in range(50):
        n = int(rng.integers(1, 20))
        pick = rng.integers(0, 4, n)
        widths = [int(x) for x in np.where(
            pick == 0, rng.integers(0, 3, n),
            np.where(pick == 1, tile * rng.integers(1, 4, n) +
                     rng.integers(-1, 2, n), rng.integers(0, 5000, n)))]
        check_tile_table(widths)


def test_tile_table_just_past_the_grid_cap():
    tile, cap = tile_sites(), grid_cap()
    widths = ((cap - 3) * tile - 5, 1, 11 * tile - 77)
    assert check_tile_table(widths) == cap + 9


def test_tile_table_rejects_malformed_arguments():
    assert tile_table((5, -1), cap=4)[0] == -1
    assert tile_table((5,), cap=4, tile=-1)[0] == -1


# ---------------------------------------------------------------------------
# GPU: on-chip path against the level path
# ---------------------------------------------------------------------------

def mk_specs(widths, ntips=12, seed=5, tips_fn=None):
    """(tips, wgt, model) per partition with the distinct random GTR models
    of test_multi_fused._mk."""
    rng = np.random.default_rng(seed)
    specs = []
    for i, w in enumerate(widths):
        tips, wgt = (tips_fn or H.make_synthetic)(ntips, w, seed=seed + i)
        freqs = rng.uniform(0.1, 0.4, 4)
        freqs /= freqs.sum()
        rates = list(rng.uniform(0.3, 3.0, 5)) + [1.0]
        specs.append((tips, wgt, ea.DnaGtrModel(
            list(freqs), rates, alpha=float(rng.uniform(0.2, 1.5)))))
    return specs


def call(tree, entries=None, root=None, active=None, qz=None, rz=None,
         zroot=None):
    if entries is None:
        entries, root = tree.full_traversal()
    p, q, z = root
    return SimpleNamespace(tree=tree, entries=entries, p=p, q=q,
                           z=z if zroot is None else zroot, active=active,
                           qz=qz, rz=rz)


def rescaled(entries, fq, fr):
    return [ea.TravEntry(e.tipCase, e.pNumber, e.qNumber, e.rNumber,
                         e.x1Slot, e.x2Slot, e.x3Slot, min(e.qz * fq, 0.99),
                         min(e.rz * fr, 0.99)) for e in entries]


def run_calls(specs, calls, switch):
    """Fresh guarded engines and one handle; `switch` is the value of
    examl_hip_multi_use_fused for every call, or one value per call.
    -> per call: ([clv pool per partition], [scalers per partition],
    lnL vector), and the launch counter after every traversal."""
    L = ea.lib()
    if isinstance(switch, int):
        switch = [switch] * len(calls)
    snaps, counts = [], []
    try:
        guards = [Guarded(t, w, m) for t, w, m in specs]
        multi = ea.MultiDnaEngine([g.eng for g in guards])
        for c, on in zip(calls, switch):
            L.examl_hip_use_fused(1)
            L.examl_hip_multi_use_fused(on)
            multi.newview_traversal(c.entries, active=c.active, qz_ov=c.qz,
                                    rz_ov=c.rz)
            counts.append(multi.fused_launches())
            lnl = multi.evaluate_root(c.tree, c.p, c.q,
                                      c.z).cpu().numpy().copy()
            clvs, scs = [], []
            for g in guards:
                clv, sc, guard_ok = g.state()
                assert guard_ok, "a kernel wrote past the end of a CLV pool"
                clvs.append(clv.copy())
                scs.append(sc.copy())
            snaps.append((clvs, scs, lnl))
        del multi
    finally:
        L.examl_hip_use_fused(1)
        L.examl_hip_multi_use_fused(MULTI_FUSED_DEFAULT)
    return snaps, counts


def assert_identical(a, b, parts=None):
    clv_a, sc_a, lnl_a = a
    clv_b, sc_b, lnl_b = b
    for i in (range(len(clv_a)) if parts is None else parts):
        assert np.array_equal(clv_a[i], clv_b[i]), f"CLV pool {i} differs"
        assert np.array_equal(sc_a[i], sc_b[i]), f"scalers {i} differ"
        assert lnl_a[i] == lnl_b[i], (i, lnl_a[i], lnl_b[i])


def on_and_off(specs, calls):
    """Both sides of a case; asserts the counters and identical states."""
    on, n_on = run_calls(specs, calls, 1)
    off, n_off = run_calls(specs, calls, 0)
    print("on-chip launches per call:", n_on, "level path:", n_off)
    assert all(n >= 1 for n in n_on), n_on
    assert all(n == 0 for n in n_off), n_off
    for a, b in zip(on, off):
        assert_identical(a, b)
    return on, off, n_on


@pytest.mark.gpu
def test_onchip_ragged_widths_around_the_tile():
    widths = (1, 3, 127, 128, 129, 333)
    specs = mk_specs(widths)
    tree = ea.PhyloTree.random(12, seed=31, rng_z=True)
    c = call(tree)
    on, _, _ = on_and_off(specs, [c])
    for i, (tips, wgt, mdl) in enumerate(specs):
        eng = ea.DnaGammaEngine(tips, wgt, mdl, device="cuda:0")
        eng.newview_traversal(c.entries)
        single = eng.evaluate_root(tree, c.p, c.q, c.z).item()
        got = on[0][2][i]
        print(f"partition {i} (width {widths[i]}): single {single!r} "
              f"on-chip {got!r}")
        assert abs(got - single) <= 1e-11 * abs(single), (i, single, got)


@pytest.mark.gpu
def test_onchip_deep_caterpillar_rescales():
    ntips, parts = H.fused_deep_inputs(4)
    on, off, _ = on_and_off(parts, [call(H.deep_caterpillar(ntips))])
    for side in (on, off):
        assert max(int(sc.max()) for sc in side[0][1]) > 0


@pytest.mark.gpu
def test_onchip_rescales_with_an_lds_stack_operand():
    tree = cherry_caterpillar(70, H.DEEP_Z)
    # partition 0 is the alignment and model of
    # test_fused_rescales_at_stack_depth_2, which rescales
    mdls = (model(), H.fused_deep_inputs(4)[1][3][2])
    specs = [H.random_tips(tree.ntips, w, H.DNA_BASES, seed=7 + i) + (m,)
             for i, (w, m) in enumerate(zip((37, 130), mdls))]
    c = call(tree)
    on, off, _ = on_and_off(specs, [c])
    st = check_plan(c.entries)
    deep = []
    for sc in on[0][1]:
        assert sc.max() > 0
        deep += [i for i, e in enumerate(c.entries)
                 if e.tipCase == INNER_INNER and st["op_depth"][i] >= 2 and
                 sc[e.pNumber] > sc[e.qNumber] + sc[e.rNumber]]
    assert deep, "no rescale happened at stack depth >= 2"


@pytest.mark.gpu
def test_onchip_masked_partitions_stay_untouched():
    specs = mk_specs((150, 129, 64, 300))
    tree = ea.PhyloTree.random(12, seed=31, rng_z=True)
    first = call(tree)
    second = call(tree, entries=rescaled(first.entries, 0.8, 0.9),
                  root=(first.p, first.q, first.z), active=[1, 0, 1, 0])
    on, off, _ = on_and_off(specs, [first, second])
    # masked: byte-identical to before the second call
    for i in (1, 3):
        assert np.array_equal(on[1][0][i], on[0][0][i])
        assert np.array_equal(on[1][1][i], on[0][1][i])
    # active: what the level path gives, and the second call did run
    assert_identical(on[1], off[1], parts=(0, 2))
    for i in (0, 2):
        assert not np.array_equal(on[1][0][i], on[0][0][i])


@pytest.mark.gpu
def test_onchip_per_partition_branch_lengths():
    specs = mk_specs((300, 515))
    tree = ea.PhyloTree.random(12, seed=31, rng_z=True)
    entries, (p, q, z) = tree.full_traversal()
    rng = np.random.default_rng(9)
    qz = np.empty((len(entries), 2))
    rz = np.empty((len(entries), 2))
    for i, e in enumerate(entries):
        for m in range(2):
            qz[i, m] = min(max(e.qz * rng.uniform(0.7, 1.3), 1e-6), 0.999)
            rz[i, m] = min(max(e.rz * rng.uniform(0.7, 1.3), 1e-6), 0.999)
    zroot = np.array([min(max(z * 0.9, 1e-6), 0.999),
                      min(max(z * 1.1, 1e-6), 0.999)])
    on, _, _ = on_and_off(specs, [call(tree, qz=qz, rz=rz, zroot=zroot)])
    # the overrides reached the kernel: partition 0 differs from a joint run
    joint, _ = run_calls(specs, [call(tree)], 1)
    assert not np.array_equal(on[0][0][0], joint[0][0][0])


@pytest.mark.gpu
def test_onchip_tree_deeper_than_the_stack_takes_several_launches():
    tree = deep_stack_tree(fused_depth() + 1)
    specs = mk_specs((65, 200), ntips=50, seed=9)
    _, _, n_on = on_and_off(specs, [call(tree)])
    assert n_on[0] >= 2


def _swapped_children(entries, k):
    """The same computation with the children of INNER_INNER entry k named
    the other way round: no longer in stack order."""
    e = entries[k]
    e.x1Slot, e.x2Slot = e.x2Slot, e.x1Slot
    e.qNumber, e.rNumber = e.rNumber, e.qNumber
    e.qz, e.rz = e.rz, e.qz


@pytest.mark.gpu
def test_onchip_one_entry_launch_runs_the_level_kernel():
    """A list the planner cuts into a 9-entry launch and a one-entry
    launch: the second goes through k_newview_dna_mseg inside the on-chip
    dispatch and reads both operands from the pool."""
    tree = ea.PhyloTree.random(12, seed=4, rng_z=True)
    c = call(tree)
    _swapped_children(c.entries, 9)
    assert c.entries[9].tipCase == INNER_INNER
    st = check_plan(c.entries)
    sizes = list(np.bincount(st["plan"][0]))
    assert sizes == [9, 1], sizes
    _, _, n_on = on_and_off(mk_specs((65, 200, 129), seed=17), [c])
    assert n_on[0] == 1      # one multi-entry launch; the single is not one


@pytest.mark.gpu
def test_onchip_partial_list_reads_the_pool():
    specs = mk_specs((65, 200), seed=13)
    tree = ea.PhyloTree.random(12, seed=5, rng_z=True)
    full = call(tree)
    start = next(e for e in full.entries if e.tipCase == ea.TIP_TIP)
    part, _ = root_path_partial(tree, start.pNumber)
    for k, e in enumerate(part):
        tree.set_z(e.pNumber, e.qNumber, 0.31 + 0.05 * k)
    part, root = root_path_partial(tree, start.pNumber)
    st = check_plan(part)
    assert len(part) >= 3 and st["launches"] == 1 and st["mem"] >= 1
    _, _, n_on = on_and_off(specs, [full, call(tree, entries=part,
                                               root=root)])
    assert n_on[1] == 1


@pytest.mark.gpu
def test_onchip_graph_replay_and_switching():
    specs = mk_specs((65, 200, 129))
    tree = ea.PhyloTree.random(12, seed=31, rng_z=True)
    base = call(tree)
    calls = [call(tree, entries=rescaled(base.entries, f, 2 - f),
                  root=(base.p, base.q, base.z))
             for f in (1.0, 0.9, 0.8, 0.7, 0.95)]
    got, n = run_calls(specs, calls, [1, 1, 1, 0, 1])
    ref, n_ref = run_calls(specs, calls, 0)
    print("launch counter per call:", n)
    assert n[3] == 0 and all(k >= 1 for k in n[:3] + n[4:]), n
    assert n_ref == [0] * 5
    for a, b in zip(got, ref):
        assert_identical(a, b)
    # the branch lengths did change what the replays computed
    assert not np.array_equal(got[0][0][0], got[1][0][0])


@pytest.mark.gpu
def test_onchip_grid_stride_wrap_across_partitions():
    """Tile counts cap - 3, 1 and 11: blocks 0..8 run a tile of partition 0
    and then one of partition 2, the one-site partition sits between."""
    tile, cap = tile_sites(), grid_cap()
    widths = ((cap - 3) * tile - 5, 1, 11 * tile - 77)
    assert sum(widths) <= 530000
    rc, part, _ = tile_table(widths)
    assert rc == cap + 9 and part[0] != part[cap]
    specs = mk_specs(widths, ntips=4, seed=12)
    on_and_off(specs, [call(ea.PhyloTree.random(4, seed=3, rng_z=True))])


@pytest.mark.gpu
def test_onchip_launch_larger_than_the_cache_streams_narrow_partitions():
    """A launch that stores more than FUSED_STREAM_BYTES (256 MB) streams
    every partition's stores, also those under the 65536-site rule: the
    smallest such shape is one 48-entry launch over 44,001 sites."""
    widths = (30000, 14001)
    tree = ea.PhyloTree.random(50, seed=7)     # the bench tree: one launch
    c = call(tree)
    assert check_plan(c.entries)["launches"] == 1
    assert max(widths) < 65536
    assert len(c.entries) * sum(widths) * 128 > (256 << 20)
    on_and_off(mk_specs(widths, ntips=50, seed=21), [c])


@pytest.mark.gpu
def test_onchip_switch_leaves_protein_handles_alone():
    L = ea.lib()
    lnl = {}
    try:
        for on in (1, 0):
            L.examl_hip_use_fused(1)
            L.examl_hip_multi_use_fused(on)
            _, multi, tree = _mk(states=20)
            lnl[on] = multi.full_lnl(tree).cpu().numpy().copy()
            assert multi.fused_launches() == 0
    finally:
        L.examl_hip_use_fused(1)
        L.examl_hip_multi_use_fused(MULTI_FUSED_DEFAULT)
    assert np.array_equal(lnl[0], lnl[1])
