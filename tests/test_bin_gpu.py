"""Binary (two-state) GTRGAMMA on the device.

  - the L0 kernels against tests/golden/bin_kernels.npz (the reference's own
    compiled kernels): newview and sum bit for bit, scaler increments
    included, in the ordinary, all-rescaling and mixed regimes; evaluate and
    core to 1e-11 relative;
  - newview at ragged widths against tests/bin_ref.py, bit for bit: around
    the 64-site block, on both sides of the streaming-store threshold and
    just past the grid cap, with half the sites rescaling;
  - the engine: full_lnl, a 500-tip caterpillar whose rescaling recurses
    through the scaler finalize, makenewz, graph replay against direct
    launches;
  - `python -m examl_amd -f E` on the pure binary and the mixed DNA+BIN
    fixtures against the reference examl-AVX lnL.
"""

import ctypes
import os

import numpy as np
import pytest

import examl_amd as ea
from examl_amd import INNER_INNER, TIP_INNER, TIP_TIP
from tests import bin_ref
from tests import helpers as H

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LNL_E_BIN = -1234.713639      # reference examl-AVX, tests/golden/gen_bin.py
LNL_E_MIX = -2626.066536

NULL = ctypes.c_void_p(0)


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def npv(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gk(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "bin_kernels.npz")))


def _to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def gpu_newview(dev, tc, x1, x2, EV, tv, t1, t2, n, P, wgt):
    """One examl_hip_newview_bin_gamma launch; returns (x3, inc)."""
    d_x1 = _to_dev(x1, dev) if tc == INNER_INNER else None
    d_x2 = _to_dev(x2, dev) if tc != TIP_TIP else None
    d_t1 = _to_dev(t1, dev) if tc != INNER_INNER else None
    d_t2 = _to_dev(t2, dev) if tc == TIP_TIP else None
    # poisoned output: every double must be written
    d_x3 = torch.full((n * 8,), float("nan"), dtype=torch.float64,
                      device=dev)
    d_P = _to_dev(P, dev)
    d_EV, d_tv, d_wgt = _to_dev(EV, dev), _to_dev(tv, dev), _to_dev(wgt, dev)
    d_inc = torch.zeros(1, dtype=torch.int32, device=dev)
    ea.check(ea.lib().examl_hip_newview_bin_gamma(
        tc, vp(d_x1) if d_x1 is not None else NULL,
        vp(d_x2) if d_x2 is not None else NULL, vp(d_x3), vp(d_EV), vp(d_tv),
        vp(d_t1) if d_t1 is not None else NULL,
        vp(d_t2) if d_t2 is not None else NULL, ctypes.c_long(n), vp(d_P),
        ctypes.c_void_p(d_P.data_ptr() + 16 * 8), vp(d_wgt), vp(d_inc),
        NULL), "newview_bin")
    torch.cuda.synchronize()
    return d_x3.cpu().numpy(), int(d_inc.item())


# ---- L0 kernels against the reference's vectors ---------------------------

@pytest.mark.parametrize("tag", ["norm", "tiny", "mix"])
@pytest.mark.parametrize("tc", [TIP_TIP, TIP_INNER, INNER_INNER])
def test_newview_bin_bit_exact_vs_golden(gk, dev, tag, tc):
    n = len(gk["wgt"])
    P = np.concatenate([gk["m1_left"], gk["m1_right"]])
    x3, inc = gpu_newview(dev, tc, gk.get(f"{tag}_tc{tc}_x1"),
                          gk.get(f"{tag}_tc{tc}_x2"), gk["m1_EV"],
                          gk["m1_tipVector"], gk["tipX1"], gk["tipX2"], n, P,
                          gk["wgt"])
    assert inc == int(gk[f"{tag}_tc{tc}_inc"])
    assert np.array_equal(_bits(x3), _bits(gk[f"{tag}_tc{tc}_x3"]))


def test_evaluate_bin_vs_golden(gk, dev):
    n = len(gk["wgt"])
    d_x1 = _to_dev(gk["norm_tc2_x1"], dev)
    d_x2 = _to_dev(gk["norm_tc2_x2"], dev)
    d_tv = _to_dev(gk["m1_tipVector"], dev)
    d_t1 = _to_dev(gk["tipX1"], dev)
    d_wgt = _to_dev(gk["wgt"], dev)
    d_diag = _to_dev(gk["diag"], dev)
    d_part = torch.zeros(8192, dtype=torch.float64, device=dev)
    for x1p, t1p, key in ((vp(d_x1), NULL, "eval_II"),
                          (NULL, vp(d_t1), "eval_TIP")):
        d_lnl = torch.zeros(1, dtype=torch.float64, device=dev)
        ea.check(ea.lib().examl_hip_evaluate_bin_gamma(
            vp(d_wgt), x1p, vp(d_x2), vp(d_tv), t1p, ctypes.c_long(n),
            vp(d_diag), NULL, NULL, ctypes.c_double(0.0), vp(d_part),
            vp(d_lnl), NULL), "evaluate_bin")
        torch.cuda.synchronize()
        got, want = d_lnl.item(), float(gk[key])
        print(key, got, want, abs(got - want) / abs(want))
        assert abs(got - want) <= 1e-11 * abs(want)


@pytest.mark.parametrize("tc", [TIP_TIP, TIP_INNER, INNER_INNER])
def test_sum_and_core_bin_vs_golden(gk, dev, tc):
    n = len(gk["wgt"])
    x1 = gk.get(f"norm_tc{tc}_x1")
    x2 = gk.get(f"norm_tc{tc}_x2")
    d_x1 = _to_dev(x1, dev) if x1 is not None else None
    d_x2 = _to_dev(x2, dev) if x2 is not None else None
    d_tv = _to_dev(gk["m1_tipVector"], dev)
    d_t1, d_t2 = _to_dev(gk["tipX1"], dev), _to_dev(gk["tipX2"], dev)
    d_sum = torch.full((n * 8,), float("nan"), dtype=torch.float64,
                       device=dev)
    ea.check(ea.lib().examl_hip_sum_bin_gamma(
        tc, vp(d_sum), vp(d_x1) if d_x1 is not None else NULL,
        vp(d_x2) if d_x2 is not None else NULL, vp(d_tv),
        vp(d_t1) if tc != INNER_INNER else NULL,
        vp(d_t2) if tc == TIP_TIP else NULL, ctypes.c_long(n), NULL),
        "sum_bin")
    torch.cuda.synchronize()
    assert np.array_equal(_bits(d_sum.cpu().numpy()),
                          _bits(gk[f"sum_tc{tc}"]))

    d_wgt = _to_dev(gk["wgt"], dev)
    d_dtab = torch.zeros(24, dtype=torch.float64, device=dev)
    d_out2 = torch.zeros(2, dtype=torch.float64, device=dev)
    d_part = torch.zeros(2 * 8192, dtype=torch.float64, device=dev)
    ea.check(ea.lib().examl_hip_core_root_bin_gamma(
        ctypes.c_long(n), vp(d_sum), npv(gk["m1_EIGN"]),
        npv(gk["m1_gammaRates"]), ctypes.c_double(float(gk["lz_core"])),
        vp(d_wgt), vp(d_dtab), vp(d_part), vp(d_out2), NULL), "core_bin")
    torch.cuda.synchronize()
    out = d_out2.cpu().numpy()
    for got, key in ((out[0], "d1"), (out[1], "d2")):
        want = float(gk[f"core_tc{tc}_{key}"])
        print(tc, key, got, want, abs(got - want) / abs(want))
        assert abs(got - want) <= 1e-11 * abs(want)
    # the L0 entry on the uploaded tables gives the same two numbers
    d_out2b = torch.zeros(2, dtype=torch.float64, device=dev)
    ea.check(ea.lib().examl_hip_core_bin_gamma(
        ctypes.c_long(n), vp(d_sum), vp(_to_dev(gk["dtab_core"], dev)),
        vp(d_wgt), vp(d_part), vp(d_out2b), NULL), "core_bin L0")
    torch.cuda.synchronize()
    assert np.array_equal(_bits(d_out2b.cpu().numpy()), _bits(out))


# ---- widths ----------------------------------------------------------------

NT_SITES = 131072               # examl_hip_bin_nt_threshold()
GRID_WRAP = 524288 + 37         # n*4 > 8192*256: the grid-stride loop wraps
WIDTHS = [1, 3, 63, 64, 65, 257, 1000, NT_SITES - 1, NT_SITES, GRID_WRAP]

_inputs = {}


def width_inputs(n):
    """Random operands for width n (shared by the three tipCases): tips with
    codes 1..3, CLVs of which every other site is tiny, so scaler increments
    are non-zero wherever the width has two sites."""
    if n not in _inputs:
        rng = np.random.default_rng(1000 + n)
        x1 = rng.uniform(0.01, 1.0, (n, 8))
        x2 = rng.uniform(0.01, 1.0, (n, 8))
        x1[1::2] *= 1e-90
        x2[1::2] *= 1e-90
        t1 = rng.integers(1, 4, n).astype(np.uint8)
        t2 = rng.integers(1, 4, n).astype(np.uint8)
        wgt = rng.integers(1, 5, n).astype(np.int32)
        _inputs.clear()            # keep one width's arrays alive at a time
        _inputs[n] = (x1.reshape(-1), x2.reshape(-1), t1, t2, wgt)
    return _inputs[n]


@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("tc", [TIP_TIP, TIP_INNER, INNER_INNER])
def test_newview_bin_widths_bit_exact(gk, dev, n, tc):
    assert ea.lib().examl_hip_bin_nt_threshold() == NT_SITES
    x1, x2, t1, t2, wgt = width_inputs(n)
    P = np.concatenate([gk["m1_left"], gk["m1_right"]])
    EV, tv = gk["m1_EV"], gk["m1_tipVector"]
    want, want_inc = bin_ref.newview(
        tc, x1 if tc == INNER_INNER else None,
        x2 if tc != TIP_TIP else None, EV, tv,
        t1 if tc != INNER_INNER else None, t2 if tc == TIP_TIP else None,
        n, P[:16], P[16:], wgt)
    got, inc = gpu_newview(dev, tc, x1, x2, EV, tv, t1, t2, n, P, wgt)
    assert inc == want_inc
    if tc != TIP_TIP and n >= 2:
        assert inc > 0
    assert np.array_equal(_bits(got), _bits(want))


# ---- engine level ------------------------------------------------------------

def _bin_case(ntips, width, seed, freqs=(0.41, 0.59), alpha=0.6,
              codes=(1, 2, 3)):
    tips, wgt = H.random_tips(ntips, width, codes, seed)
    return tips, wgt, ea.BinGtrModel(list(freqs), alpha)


def test_engine_full_lnl_and_makenewz_vs_numpy(dev):
    tips, wgt, model = _bin_case(12, 333, seed=3)
    tree = ea.PhyloTree.random(12, seed=11, rng_z=True)
    eng = ea.DnaGammaEngine(tips, wgt, model, device=dev)
    assert eng.SPAN == 8 and eng._sfx == "bin"
    ref = bin_ref.BinRefEngine(tips, wgt, model)
    got = eng.full_lnl(tree).item()
    want = ref.full_lnl(tree)
    print("full_lnl", got, want, abs(got - want) / abs(want))
    assert abs(got - want) <= 1e-11 * abs(want)
    # every CLV of the traversal is bit-identical to the numpy engine's
    clv = eng.d_clv.cpu().numpy()
    for slot, x in ref.clv.items():
        assert np.array_equal(_bits(clv[slot]), _bits(x)), slot
    _, (p, q, z) = tree.full_traversal()
    z_gpu = eng.makenewz(tree, p, q, z)
    z_ref = ref.makenewz(tree, p, q, z)
    print("makenewz", z_gpu, z_ref)
    assert abs(z_gpu - z_ref) <= 1e-9 * abs(z_ref)
    assert ea.ZMIN <= z_gpu <= ea.ZMAX and z_gpu != z


def test_engine_deep_caterpillar_rescales(dev):
    """500 tips at a small width: CLV magnitudes fall below 2^-256 more than
    once along the chain, so per-node scaler counts accumulate through the
    finalize kernel."""
    ntips = 500
    # determined tips only: an undetermined tip does not shrink the CLV
    tips, wgt, model = _bin_case(ntips, 24, seed=9, codes=(1, 2))
    tree = H.deep_caterpillar(ntips)
    eng = ea.DnaGammaEngine(tips, wgt, model, device=dev)
    ref = bin_ref.BinRefEngine(tips, wgt, model)
    got = eng.full_lnl(tree).item()
    want = ref.full_lnl(tree)
    sc = eng.d_scalers.cpu().numpy().astype(np.int64)
    assert np.array_equal(sc, ref.scalers)
    # some sites rescale twice on the way down: the counts of the two
    # events reach the root only through the recursive finalize
    assert sc.max() > int(wgt.sum())
    print("caterpillar", got, want, abs(got - want) / abs(want), sc.max())
    assert abs(got - want) <= 1e-11 * abs(want)


def test_engine_graph_replay_matches_direct_launches(dev):
    tips, wgt, model = _bin_case(24, 200, seed=5)
    tree = ea.PhyloTree.random(24, seed=2, rng_z=True)
    entries, _ = tree.full_traversal()
    assert len(entries) >= 8          # the executor's graph threshold
    eng = ea.DnaGammaEngine(tips, wgt, model, device=dev)
    L = ea.lib()
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    try:
        with torch.cuda.stream(st):
            eng.newview_traversal(entries)   # capture + launch
            eng.d_clv.zero_()
            eng.newview_traversal(entries)   # replay
        st.synchronize()
        clv_graph = eng.d_clv.cpu().numpy().copy()
        sc_graph = eng.d_scalers.cpu().numpy().copy()
        L.examl_hip_use_graphs(0)
        with torch.cuda.stream(st):
            eng.d_clv.zero_()
            eng.d_scalers.zero_()
            eng.newview_traversal(entries)
        st.synchronize()
    finally:
        L.examl_hip_use_graphs(1)
        L.examl_hip_graphs_clear()
    assert np.array_equal(_bits(eng.d_clv.cpu().numpy()), _bits(clv_graph))
    assert np.array_equal(eng.d_scalers.cpu().numpy(), sc_graph)
    ref = bin_ref.BinRefEngine(tips, wgt, model)
    ref.newview_traversal(entries)
    for slot, x in ref.clv.items():
        assert np.array_equal(_bits(clv_graph[slot]), _bits(x)), slot


# ---- end to end on the device ------------------------------------------------

@pytest.mark.parametrize("fixture,want", [("12bin.binary", LNL_E_BIN),
                                          ("12mix.binary", LNL_E_MIX)])
def test_cli_f_E_binary_gpu(golden_dir, tmp_path, fixture, want):
    from examl_amd.__main__ import main
    rc = main(["-s", os.path.join(golden_dir, fixture),
               "-t", os.path.join(golden_dir, "12.tree"),
               "-n", "B", "-f", "E", "-w", str(tmp_path)])
    assert rc == 0
    info = open(os.path.join(tmp_path, "ExaML_info.B")).read()
    assert "DataType: BINARY/MORPHOLOGICAL" in info
    line = [ln for ln in info.splitlines()
            if ln.startswith("Likelihood tree 0:")][0]
    lnl = float(line.split(":")[1])
    print(fixture, lnl, want, abs(lnl - want) / abs(want))
    assert abs(lnl - want) <= 1e-6 * abs(want)
