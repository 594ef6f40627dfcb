"""hipGraph capture and replay of the traversal executors against direct
launches.

Engines run on the null stream by default, where the executors never
capture; every test here runs on a side stream, so the first call captures,
instantiates and launches a graph and the second replays it."""

import numpy as np
import pytest
import torch

import examl_amd as ea
from tests import helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NTIPS, WIDTH = 12, 77      # 10 entries >= the graph threshold of 8


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _tree():
    return ea.PhyloTree.random(NTIPS, seed=23, rng_z=True)


def _cat_arrays(seed):
    f = H.edge_family("dna_cat")
    rng = np.random.default_rng(seed)
    return (rng.integers(0, f.num_cats, WIDTH).astype(np.int32),
            np.array(f.rates))


def _family(name):
    """-> (engine, {slot: oracle CLV} or None) of one executor family."""
    if name in ("dna_gamma", "dna_gamma_unfused", "dna_cat"):
        tips, wgt = H.random_tips(NTIPS, WIDTH, H.DNA_BASES, 7)
    else:
        tips, wgt = H.random_tips(NTIPS, WIDTH, H.AA_CODES, 7)
    entries, root = _tree().full_traversal()
    if name in ("dna_gamma", "dna_gamma_unfused"):
        model = H.edge_family("dna_gamma").model
        _, ref, _ = H.oracle_full_lnl(entries, root, _tree(), model, tips,
                                      wgt, return_state=True)
        return ea.DnaGammaEngine(tips, wgt, model, device=DEV), ref
    if name == "prot_gamma":
        model = H.edge_family("prot_gamma").model
        return ea.DnaGammaEngine(tips, wgt, model, device=DEV), None
    if name == "dna_cat":
        cptr, rates = _cat_arrays(11)
        return ea.DnaCatEngine(tips, wgt, H.edge_family("dna_cat").model,
                               cptr, rates, device=DEV), None
    if name == "prot_cat":
        tips, wgt, model, cptr, rates = H.prot_cat_inputs(NTIPS, WIDTH, 7)
        orc = H.OracleProtCatEngine(tips, wgt, model, cptr, rates)
        orc.newview_traversal(entries)
        return ea.ProtCatEngine(tips, wgt, model, cptr, rates,
                                device=DEV), orc.clv
    assert name == "lg4"
    model = ea.Lg4Model.lg4x()
    orc = H.OracleLg4Engine(tips, wgt, model)
    orc.newview_traversal(entries)
    return ea.Lg4Engine(tips, wgt, model, device=DEV), orc.clv


def _state(engines):
    return ([e.d_clv.cpu().numpy().copy() for e in engines],
            [e.d_scalers.cpu().numpy().copy() for e in engines])


def replay_and_direct(run, engines, fused=1, multi_fused=1):
    """`run()` enqueues one traversal on the current stream.  -> the
    (CLV pools, scalers) of a graph replay and of a direct run."""
    L = ea.lib()
    st = torch.cuda.Stream(device=DEV)
    st.wait_stream(torch.cuda.current_stream(DEV))
    try:
        L.examl_hip_graphs_clear()
        L.examl_hip_use_graphs(1)
        L.examl_hip_use_fused(fused)
        L.examl_hip_multi_use_fused(multi_fused)
        with torch.cuda.stream(st):
            run()                          # capture + launch
            for e in engines:
                e.d_clv.zero_()
            run()                          # replay
        st.synchronize()
        replay = _state(engines)
        L.examl_hip_use_graphs(0)
        with torch.cuda.stream(st):
            for e in engines:
                e.d_clv.zero_()
                e.d_scalers.zero_()
            run()
        st.synchronize()
        direct = _state(engines)
    finally:
        L.examl_hip_use_graphs(1)
        L.examl_hip_use_fused(1)
        L.examl_hip_multi_use_fused(1)
        L.examl_hip_graphs_clear()
    return replay, direct


def assert_same(replay, direct):
    for i, (a, b) in enumerate(zip(replay[0], direct[0])):
        assert np.array_equal(_bits(a), _bits(b)), f"CLV pool {i} differs"
    for i, (a, b) in enumerate(zip(replay[1], direct[1])):
        assert np.array_equal(a, b), f"scalers {i} differ"


@pytest.mark.parametrize("name", ["dna_gamma", "dna_gamma_unfused",
                                  "prot_gamma", "dna_cat", "prot_cat",
                                  "lg4"])
def test_graph_replay_matches_direct(name):
    eng, ref = _family(name)
    entries, _ = _tree().full_traversal()
    assert len(entries) >= 8           # the executors' graph threshold
    replay, direct = replay_and_direct(
        lambda: eng.newview_traversal(entries), [eng],
        fused=0 if name == "dna_gamma_unfused" else 1)
    assert_same(replay, direct)
    if ref is not None:
        for slot, x in ref.items():
            assert np.array_equal(_bits(replay[0][0][slot]), _bits(x)), slot


def test_graph_replay_crosses_chunks():
    """198 entries: past the 180-entry finalize chunk and the 192-entry
    fused program."""
    ntips, width = 200, 24
    tree = H.deep_caterpillar(ntips)
    entries, root = tree.full_traversal()
    assert len(entries) == 198
    tips, wgt = H.random_tips(ntips, width, H.DNA_BASES, 3)
    model = H.edge_family("dna_gamma").model
    eng = ea.DnaGammaEngine(tips, wgt, model, device=DEV)
    replay, direct = replay_and_direct(
        lambda: eng.newview_traversal(entries), [eng])
    assert_same(replay, direct)
    _, _, sc_ref = H.oracle_full_lnl(entries, root, tree, model, tips, wgt,
                                     return_state=True)
    sc = replay[1][0]
    assert sc.max() > 0                # the finalize recursion did add up
    assert np.array_equal(sc.astype(np.int64), sc_ref)


def test_cat_graph_key_follows_cptr():
    """A new rate-category tensor at a new address must not replay the graph
    that bound the old one."""
    tips, wgt = H.random_tips(NTIPS, WIDTH, H.DNA_BASES, 7)
    cptr_a, rates = _cat_arrays(11)
    cptr_b, _ = _cat_arrays(12)
    assert (cptr_a != cptr_b).any()
    eng = ea.DnaCatEngine(tips, wgt, H.edge_family("dna_cat").model, cptr_a,
                          rates, device=DEV)
    entries, _ = _tree().full_traversal()
    d_cptr_a = eng.d_cptr              # stays alive: its address is not reused
    L = ea.lib()
    st = torch.cuda.Stream(device=DEV)
    st.wait_stream(torch.cuda.current_stream(DEV))
    try:
        L.examl_hip_graphs_clear()
        L.examl_hip_use_graphs(1)
        with torch.cuda.stream(st):
            eng.newview_traversal(entries)
            eng.d_cptr = torch.from_numpy(cptr_b).to(DEV)
            eng.d_clv.zero_()
            eng.newview_traversal(entries)
        st.synchronize()
        got = _state([eng])
        L.examl_hip_use_graphs(0)
        with torch.cuda.stream(st):
            eng.d_clv.zero_()
            eng.d_scalers.zero_()
            eng.newview_traversal(entries)
        st.synchronize()
        want = _state([eng])
    finally:
        L.examl_hip_use_graphs(1)
        L.examl_hip_use_fused(1)
        L.examl_hip_graphs_clear()
    assert d_cptr_a.data_ptr() != eng.d_cptr.data_ptr()
    assert_same(got, want)


@pytest.mark.parametrize("multi_fused", [1, 0])
def test_multi_graph_replay_matches_direct(multi_fused):
    from tests.test_multi_onchip import mk_specs
    specs = mk_specs((37, 131, 1), ntips=NTIPS)
    engines = [ea.DnaGammaEngine(t, w, m, device=DEV) for t, w, m in specs]
    multi = ea.MultiDnaEngine(engines)
    entries, _ = _tree().full_traversal()
    launches = []

    def run():
        multi.newview_traversal(entries)
        launches.append(multi.fused_launches())

    replay, direct = replay_and_direct(run, engines, multi_fused=multi_fused)
    del multi
    assert all((n >= 1) == bool(multi_fused) for n in launches), launches
    assert_same(replay, direct)
