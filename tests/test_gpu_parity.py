"""GPU parity tests: the HIP kernels against the committed reference golden
vectors (bit-exact for newview/sum; 1e-12 relative for the log/reduction
paths) and the full device pipeline against the CPU oracle."""

import ctypes
import math
import os

import numpy as np
import pytest

import examl_amd as ea
from tests.helpers import (load_golden_parts, make_synthetic, oracle_full_lnl,
                           oracle_makenewz)

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def kern(golden_dir):
    return load_golden_parts(golden_dir, "kernels_dna_gamma")


@pytest.fixture(scope="module")
def model(golden_dir):
    d = np.load(os.path.join(golden_dir, "model_dna.npz"))
    return ea.DnaGtrModel(d["m1_freqs"], d["m1_rates6"], float(d["m1_alpha"]))


def _to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("tag", ["norm", "tiny", "tiny2"])
@pytest.mark.parametrize("tc", [ea.TIP_TIP, ea.TIP_INNER, ea.INNER_INNER])
def test_newview_kernel_bit_exact_vs_golden(kern, model, dev, tag, tc):
    n = len(kern[f"{tag}_wgt"])
    d_x1 = _to_dev(kern[f"{tag}_x1"], dev)
    d_x2 = _to_dev(kern[f"{tag}_x2"], dev)
    d_x3 = torch.zeros(n * 16, dtype=torch.float64, device=dev)
    d_P = _to_dev(np.concatenate([kern["left"], kern["right"]]), dev)
    d_EV = _to_dev(model.EV, dev)
    d_tv = _to_dev(model.tipVector, dev)
    d_t1 = _to_dev(kern[f"{tag}_tipX1"], dev)
    d_t2 = _to_dev(kern[f"{tag}_tipX2"], dev)
    d_wgt = _to_dev(kern[f"{tag}_wgt"], dev)
    d_inc = torch.zeros(1, dtype=torch.int32, device=dev)
    null = ctypes.c_void_p(0)
    x1p = vp(d_x1) if tc == ea.INNER_INNER else null
    x2p = vp(d_x2) if tc != ea.TIP_TIP else null
    t1p = vp(d_t1) if tc != ea.INNER_INNER else null
    t2p = vp(d_t2) if tc == ea.TIP_TIP else null
    ea.check(ea.lib().examl_hip_newview_dna_gamma(
        tc, x1p, x2p, vp(d_x3), vp(d_EV), vp(d_tv), t1p, t2p,
        ctypes.c_long(n), vp(d_P),
        ctypes.c_void_p(d_P.data_ptr() + 64 * 8), vp(d_wgt), vp(d_inc),
        ctypes.c_void_p(0)), "newview")
    torch.cuda.synchronize()
    x3 = d_x3.cpu().numpy()
    assert int(d_inc.item()) == int(kern[f"{tag}_newview_tc{tc}_inc"])
    assert np.array_equal(x3, kern[f"{tag}_newview_tc{tc}_x3"])


def test_evaluate_kernel_vs_golden(kern, model, dev):
    n = len(kern["norm_wgt"])
    d_x1 = _to_dev(kern["norm_x1"], dev)
    d_x2 = _to_dev(kern["norm_x2"], dev)
    d_tv = _to_dev(model.tipVector, dev)
    d_t1 = _to_dev(kern["norm_tipX1"], dev)
    d_wgt = _to_dev(kern["norm_wgt"], dev)
    d_diag = _to_dev(kern["diag"], dev)
    d_lnl = torch.zeros(1, dtype=torch.float64, device=dev)
    d_part = torch.zeros(8192, dtype=torch.float64, device=dev)
    ea.check(ea.lib().examl_hip_evaluate_dna_gamma(
        vp(d_wgt), vp(d_x1), vp(d_x2), vp(d_tv), ctypes.c_void_p(0),
        ctypes.c_long(n), vp(d_diag), ctypes.c_void_p(0), ctypes.c_void_p(0),
        ctypes.c_double(0.0), vp(d_part), vp(d_lnl), ctypes.c_void_p(0)),
        "evaluate")
    torch.cuda.synchronize()
    assert np.isclose(d_lnl.item(), float(kern["eval_II"]), rtol=1e-12)
    d_lnl.zero_()
    ea.check(ea.lib().examl_hip_evaluate_dna_gamma(
        vp(d_wgt), ctypes.c_void_p(0), vp(d_x2), vp(d_tv), vp(d_t1),
        ctypes.c_long(n), vp(d_diag), ctypes.c_void_p(0), ctypes.c_void_p(0),
        ctypes.c_double(0.0), vp(d_part), vp(d_lnl), ctypes.c_void_p(0)),
        "evaluate")
    torch.cuda.synchronize()
    assert np.isclose(d_lnl.item(), float(kern["eval_TIP"]), rtol=1e-12)


@pytest.mark.parametrize("tc", [ea.TIP_TIP, ea.TIP_INNER, ea.INNER_INNER])
def test_sum_and_core_kernels_vs_golden(kern, model, dev, tc):
    n = len(kern["norm_wgt"])
    d_x1 = _to_dev(kern["norm_x1"], dev)
    d_x2 = _to_dev(kern["norm_x2"], dev)
    d_tv = _to_dev(model.tipVector, dev)
    d_t1 = _to_dev(kern["norm_tipX1"], dev)
    d_t2 = _to_dev(kern["norm_tipX2"], dev)
    d_sum = torch.zeros(n * 16, dtype=torch.float64, device=dev)
    null = ctypes.c_void_p(0)
    x1p = vp(d_x1) if tc == ea.INNER_INNER else null
    x2p = vp(d_x2) if tc != ea.TIP_TIP else null
    t1p = vp(d_t1) if tc != ea.INNER_INNER else null
    t2p = vp(d_t2) if tc == ea.TIP_TIP else null
    ea.check(ea.lib().examl_hip_sum_dna_gamma(
        tc, vp(d_sum), x1p, x2p, vp(d_tv), t1p, t2p, ctypes.c_long(n),
        ctypes.c_void_p(0)), "sum")
    torch.cuda.synchronize()
    assert np.array_equal(d_sum.cpu().numpy(), kern[f"sum_tc{tc}"])

    d_wgt = _to_dev(kern["norm_wgt"], dev)
    d_dtab = torch.zeros(48, dtype=torch.float64, device=dev)
    d_out2 = torch.zeros(2, dtype=torch.float64, device=dev)
    d_part = torch.zeros(2 * 8192, dtype=torch.float64, device=dev)
    ea.check(ea.lib().examl_hip_core_root_dna_gamma(
        ctypes.c_long(n), vp(d_sum),
        model.EIGN.ctypes.data_as(ctypes.c_void_p),
        model.gammaRates.ctypes.data_as(ctypes.c_void_p),
        ctypes.c_double(float(kern["lz_core"])), vp(d_wgt), vp(d_dtab),
        vp(d_part), vp(d_out2), ctypes.c_void_p(0)), "core")
    torch.cuda.synchronize()
    out = d_out2.cpu().numpy()
    assert np.isclose(out[0], float(kern[f"core_tc{tc}_d1"]), rtol=1e-11)
    assert np.isclose(out[1], float(kern[f"core_tc{tc}_d2"]), rtol=1e-11)


def test_full_pipeline_vs_oracle(dev):
    ntips, width = 24, 8192
    tips, wgt = make_synthetic(ntips, width, seed=123)
    model = ea.DnaGtrModel([0.31, 0.19, 0.22, 0.28],
                           [1.5, 2.9, 0.6, 1.2, 3.3, 1.0], alpha=0.42)
    tree = ea.PhyloTree.random(ntips, seed=77, rng_z=True)
    eng = ea.DnaGammaEngine(tips, wgt, model, device=dev)
    entries, root = tree.full_traversal()
    lnl = eng.full_lnl(tree).item()
    ref, clv_ref, scalers_ref = oracle_full_lnl(entries, root, tree, model,
                                                tips, wgt, return_state=True)
    assert math.isfinite(lnl) and lnl < 0
    assert abs(lnl - ref) / abs(ref) < 1e-11
    # CLVs bit-exact, recursive scalers exact
    clv = eng.d_clv.cpu().numpy()
    for slot, x in clv_ref.items():
        assert np.array_equal(clv[slot], x), f"CLV slot {slot} differs"
    sc = eng.d_scalers.cpu().numpy()
    for node in range(ntips + 1, 2 * ntips - 1):
        assert sc[node] == scalers_ref[node]


def test_full_pipeline_scaling_depth(dev):
    """Deep caterpillar-ish tree with long branches -> guaranteed 2^-256
    rescales; lnL must still match the oracle."""
    ntips, width = 500, 128
    tips, wgt = make_synthetic(ntips, width, seed=99)
    model = ea.DnaGtrModel.jukes_cantor(alpha=0.3)
    # 498-op traversal: also exercises the chunked scaler finalize
    tree = ea.PhyloTree.caterpillar(ntips, z=0.5)
    eng = ea.DnaGammaEngine(tips, wgt, model, device=dev)
    entries, root = tree.full_traversal()
    lnl = eng.full_lnl(tree).item()
    ref, _, scalers_ref = oracle_full_lnl(entries, root, tree, model, tips,
                                          wgt, return_state=True)
    assert scalers_ref.max() > 0, "test must exercise rescaling"
    assert abs(lnl - ref) / abs(ref) < 1e-11


def test_rerooting_invariance_on_gpu(dev):
    ntips, width = 16, 4096
    tips, wgt = make_synthetic(ntips, width, seed=31)
    model = ea.DnaGtrModel([0.26, 0.24, 0.27, 0.23],
                           [0.9, 2.2, 1.1, 0.8, 2.7, 1.0], alpha=0.8)
    tree = ea.PhyloTree.random(ntips, seed=13, rng_z=True)
    eng = ea.DnaGammaEngine(tips, wgt, model, device=dev)
    edges = tree.edges()
    vals = [eng.full_lnl(tree, root_edge=e).item()
            for e in (edges[0], edges[len(edges) // 2], edges[-1])]
    assert np.allclose(vals, vals[0], rtol=1e-9)


def test_makenewz_vs_oracle(dev):
    ntips, width = 20, 4096
    tips, wgt = make_synthetic(ntips, width, seed=55)
    model = ea.DnaGtrModel([0.29, 0.21, 0.26, 0.24],
                           [1.2, 3.1, 0.5, 0.8, 2.9, 1.0], alpha=0.6)
    tree = ea.PhyloTree.random(ntips, seed=21, rng_z=True)
    eng = ea.DnaGammaEngine(tips, wgt, model, device=dev)
    entries, root = tree.full_traversal()
    p, q, z0 = root
    eng.newview_traversal(entries)
    z_gpu = eng.makenewz(tree, p, q, z0)
    z_ref = oracle_makenewz(entries, root, tree, model, tips, wgt, z0)
    assert abs(z_gpu - z_ref) < 1e-9
    # optimized branch must not decrease the likelihood (_DEBUG_UPDATE
    # invariant, searchAlgo.c:135-185)
    before = eng.evaluate_root(tree, p, q, z0).item()
    after = eng.evaluate_root(tree, p, q, z_gpu).item()
    assert after >= before - 0.01


def test_lnl_bitwise_deterministic(dev):
    """The two-pass fixed-order reductions make lnL and the NR derivatives
    bit-reproducible across repeated evaluations and engine instances (the
    reference's determinism rationale, makenewzGenericSpecial.c:1242)."""
    ntips, width = 20, 100000
    tips, wgt = make_synthetic(ntips, width, seed=8)
    model = ea.DnaGtrModel([0.3, 0.2, 0.25, 0.25],
                           [1.1, 2.4, 0.8, 0.9, 3.0, 1.0], alpha=0.7)
    tree = ea.PhyloTree.random(ntips, seed=2, rng_z=True)
    vals = []
    derivs = []
    for _ in range(2):
        eng = ea.DnaGammaEngine(tips, wgt, model, device=dev)
        entries, (p, q, z) = tree.full_traversal()
        eng.newview_traversal(entries)
        vals.append(eng.evaluate_root(tree, p, q, z).item())
        vals.append(eng.evaluate_root(tree, p, q, z).item())
        eng.sum_root(tree, p, q)
        derivs.append(eng.core_derivs(float(np.log(z))))
    assert vals[0] == vals[1] == vals[2] == vals[3]
    assert derivs[0] == derivs[1]


def test_partitioned_multistream_lnl(dev):
    """Config-3 shape: the alignment split into partitions, each evaluated
    on its own HIP stream; the summed per-partition lnL must equal the
    single-partition evaluation (shard linearity on device)."""
    ntips, width, P = 20, 64000, 8
    tips, wgt = make_synthetic(ntips, width, seed=44)
    model = ea.DnaGtrModel([0.3, 0.2, 0.25, 0.25],
                           [1.0, 2.2, 0.9, 1.1, 2.8, 1.0], alpha=0.5)
    tree = ea.PhyloTree.random(ntips, seed=6, rng_z=True)
    full = ea.DnaGammaEngine(tips, wgt, model, device=dev)
    ref = full.full_lnl(tree).item()
    pw = width // P
    engines = [ea.DnaGammaEngine(np.ascontiguousarray(tips[:, i*pw:(i+1)*pw]),
                                 wgt[i*pw:(i+1)*pw], model, device=dev)
               for i in range(P)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(P)]
    entries, (p, q, z) = tree.full_traversal()
    cur = torch.cuda.current_stream(dev)
    for e_, st in zip(engines, streams):
        st.wait_stream(cur)
        with torch.cuda.stream(st):
            e_.newview_traversal(entries)
            e_.evaluate_root(tree, p, q, z)
    for st in streams:
        cur.wait_stream(st)
    total = float(torch.cat([e_.d_lnl for e_ in engines]).sum().item())
    assert abs(total - ref) / abs(ref) < 1e-12
