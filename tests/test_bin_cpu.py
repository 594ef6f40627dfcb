"""Binary (two-state, BINARY/MORPHOLOGICAL) partitions, CPU side.

  - tests/bin_ref.py (the numpy restatement of the four reference kernels)
    is pinned against tests/golden/bin_kernels.npz, the reference's own
    compiled kernels: newview CLVs, scaler increments and sum tables bit
    for bit, evaluate and core to 1e-12 relative;
  - the product's host model math (examl_host_init_gtr_bin, make_p and
    calc_diagptable at states = 2, examl_host_core_dtables_bin) is bit-exact
    against the same goldens; it loads and runs without a GPU;
  - search and command line run end to end with only the engine factory
    swapped for CPU engines, against the reference examl-AVX goldens listed
    in tests/golden/gen_bin.py.
"""

import ctypes
import os

import numpy as np
import pytest

import examl_amd as ea
from examl_amd import INNER_INNER, TIP_INNER, TIP_TIP
from tests import bin_ref

# reference examl-AVX results (tests/golden/gen_bin.py)
LNL_E_BIN = -1234.713639
LNL_E_MIX = -2626.066536
LNL_E_MIX_M = -2504.119971
LNL_D_BIN = -1065.065040


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def gk(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "bin_kernels.npz")))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _nv_args(gk, tag, tc):
    x1 = gk.get(f"{tag}_tc{tc}_x1")
    x2 = gk.get(f"{tag}_tc{tc}_x2")
    t1 = gk["tipX1"] if tc != INNER_INNER else None
    t2 = gk["tipX2"] if tc == TIP_TIP else None
    return x1, x2, t1, t2


# ---- the numpy restatement against the reference's kernels ----------------

@pytest.mark.parametrize("tag", ["norm", "tiny", "mix"])
@pytest.mark.parametrize("tc", [TIP_TIP, TIP_INNER, INNER_INNER])
def test_bin_ref_newview_bit_exact(gk, tag, tc):
    x1, x2, t1, t2 = _nv_args(gk, tag, tc)
    n = len(gk["wgt"])
    x3, inc = bin_ref.newview(tc, x1, x2, gk["m1_EV"], gk["m1_tipVector"],
                              t1, t2, n, gk["m1_left"], gk["m1_right"],
                              gk["wgt"])
    assert np.array_equal(_bits(x3), _bits(gk[f"{tag}_tc{tc}_x3"]))
    assert inc == int(gk[f"{tag}_tc{tc}_inc"])


def test_bin_golden_regimes(gk):
    """The fixture holds what the issue asks for: nothing rescales in norm,
    everything in tiny, both in mix; mix site 1 has exactly one output above
    2^-256 and site 3 exactly one output EQUAL to 2^-256, and the reference
    rescaled neither."""
    thr = 2.0 ** -256
    for tc in (TIP_INNER, INNER_INNER):
        assert not gk[f"norm_tc{tc}_scaled"].any()
        assert gk[f"tiny_tc{tc}_scaled"].all()
        sc = gk[f"mix_tc{tc}_scaled"]
        assert 0 < sc.sum() < len(sc)
        x3 = np.abs(gk[f"mix_tc{tc}_x3"].reshape(-1, 8))
        assert not sc[1] and (x3[1] >= thr).sum() == 1 \
            and (x3[1] == thr).sum() == 0
        assert not sc[3] and (x3[3] >= thr).sum() == 1 \
            and (x3[3] == thr).sum() == 1
        assert int(gk[f"mix_tc{tc}_inc"]) == int(gk["wgt"][sc].sum())
    assert int(gk["mix_tc0_inc"]) == 0


@pytest.mark.parametrize("tc", [TIP_TIP, TIP_INNER, INNER_INNER])
def test_bin_ref_sum_bit_exact_core_close(gk, tc):
    x1, x2, t1, t2 = _nv_args(gk, "norm", tc)
    n = len(gk["wgt"])
    st = bin_ref.sumtable(tc, x1, x2, gk["m1_tipVector"], t1, t2, n)
    assert np.array_equal(_bits(st), _bits(gk[f"sum_tc{tc}"]))
    dtab = bin_ref.core_dtables(gk["m1_EIGN"], gk["m1_gammaRates"],
                                float(gk["lz_core"]))
    d1, d2 = bin_ref.core(n, st, dtab, gk["wgt"])
    for got, key in ((d1, "d1"), (d2, "d2")):
        want = float(gk[f"core_tc{tc}_{key}"])
        assert abs(got - want) <= 1e-12 * abs(want), (key, got, want)


def test_bin_ref_evaluate_close(gk):
    n = len(gk["wgt"])
    x1, x2 = gk["norm_tc2_x1"], gk["norm_tc2_x2"]
    for tip, key in ((None, "eval_II"), (gk["tipX1"], "eval_TIP")):
        got = bin_ref.evaluate(gk["wgt"], None if tip is not None else x1,
                               x2, gk["m1_tipVector"], tip, n, gk["diag"])
        want = float(gk[key])
        assert abs(got - want) <= 1e-12 * abs(want), (key, got, want)


# ---- product host math (no GPU) -------------------------------------------

@pytest.mark.parametrize("name", ["m0", "m1"])
def test_host_init_gtr_bin_bit_exact(gk, name):
    m = ea.BinGtrModel(gk[f"{name}_freqs"], float(gk[f"{name}_alpha"]))
    assert m.states == 2 and m.n_codes == 4 and list(m.rates1) == [1.0]
    for k in ("EIGN", "EV", "EI", "tipVector", "gammaRates"):
        assert np.array_equal(_bits(getattr(m, k)), _bits(gk[f"{name}_{k}"])), k
    # undetermined (code 3) is the sum of both states' rows, capped at
    # MAX_TIP_EV (axml.h:88) like every tipVector entry; code 0 is empty
    tv = m.tipVector.reshape(4, 2)
    assert not tv[0].any()
    assert np.array_equal(tv[3], np.minimum(tv[1] + tv[2], 0.999999999))
    # set_alpha / reinit keep working like DnaGtrModel's
    m.set_alpha(0.9)
    m.set_alpha(float(gk[f"{name}_alpha"]))
    m.reinit()
    assert np.array_equal(_bits(m.gammaRates), _bits(gk[f"{name}_gammaRates"]))
    assert np.array_equal(_bits(m.EV), _bits(gk[f"{name}_EV"]))


@pytest.mark.parametrize("name", ["m0", "m1"])
def test_host_make_p_states2_bit_exact(gk, name):
    """left[cat*4 + row*2 + col], 16 doubles per side; m0 also takes the
    zmin clamp (z = 1e-20 was clamped before the log)."""
    left, right = np.zeros(16), np.zeros(16)
    lq, lr = gk[f"{name}_p_logz"]
    ea.lib().examl_host_make_p(
        float(lq), float(lr), _vp(gk[f"{name}_gammaRates"]),
        _vp(gk[f"{name}_EI"]), _vp(gk[f"{name}_EIGN"]), 4, _vp(left),
        _vp(right), 2)
    assert np.array_equal(_bits(left), _bits(gk[f"{name}_left"]))
    assert np.array_equal(_bits(right), _bits(gk[f"{name}_right"]))


def test_host_diag_and_dtables_bin_bit_exact(gk):
    diag = np.zeros(8)
    ea.lib().examl_host_calc_diagptable(
        float(gk["z_root"]), 2, 4, _vp(gk["m1_gammaRates"]),
        _vp(gk["m1_EIGN"]), _vp(diag))
    assert np.array_equal(_bits(diag), _bits(gk["diag"]))
    dtab = bin_ref.core_dtables(gk["m1_EIGN"], gk["m1_gammaRates"],
                                float(gk["lz_core"]))
    assert np.array_equal(_bits(dtab), _bits(gk["dtab_core"]))


def test_bin_symbols_exported():
    L = ea.lib()
    for name in ("newview", "evaluate", "sum", "core"):
        assert hasattr(L, f"examl_hip_{name}_bin_gamma")
    for name in ("newview_traversal", "evaluate_root", "sum_root",
                 "core_root"):
        assert hasattr(L, f"examl_hip_{name}_bin_gamma")
    assert L.examl_hip_bin_nt_threshold() == 131072


# ---- search and command line ------------------------------------------------

def _cpu_build_engines(parts, opts, device):
    """Test-only stand-in for the GPU engine factory: the CPU oracle engine
    for DNA partitions, the numpy engine for binary ones."""
    from tests.helpers import OracleEngine
    engines, auto_flags, empirical = [], [], []
    for p in parts:
        auto_flags.append(False)
        empirical.append(p.frequencies)
        if p.states == 2:
            m = ea.BinGtrModel(p.frequencies, 1.0, use_median=opts["a"])
            engines.append(bin_ref.BinRefEngine(p.tips, p.wgt, m))
        else:
            assert p.states == 4
            m = ea.DnaGtrModel(p.frequencies, [1.0] * 6, 1.0,
                               use_median=opts["a"])
            engines.append(OracleEngine(p.tips, p.wgt, m))
    return engines, auto_flags, empirical


def _info_value(path, prefix):
    for ln in open(path).read().splitlines():
        if ln.startswith(prefix):
            return float(ln.split(":")[1])
    raise AssertionError(f"no {prefix!r} line in {path}")


@pytest.mark.parametrize("fixture,extra,want", [
    ("12bin.binary", [], LNL_E_BIN),
    ("12mix.binary", [], LNL_E_MIX),
    ("12mix.binary", ["-M"], LNL_E_MIX_M),
])
def test_cli_f_E_binary_cpu(golden_dir, tmp_path, monkeypatch, fixture,
                            extra, want):
    import examl_amd.__main__ as cli
    monkeypatch.setattr(cli, "_build_engines", _cpu_build_engines)
    rc = cli.main(["-s", os.path.join(golden_dir, fixture),
                   "-t", os.path.join(golden_dir, "12.tree"),
                   "-n", "E", "-f", "E", "-w", str(tmp_path)] + extra,
                  device="cpu")
    assert rc == 0
    info = os.path.join(tmp_path, "ExaML_info.E")
    lnl = _info_value(info, "Likelihood tree 0:")
    assert abs(lnl - want) <= 1e-6 * abs(want), (lnl, want)
    assert "DataType: BINARY/MORPHOLOGICAL" in open(info).read()


def test_cli_f_d_binary_cpu(golden_dir, tmp_path, monkeypatch):
    """-f d on the pure binary alignment: the reference's final lnL and
    topology, and per-cycle checkpoints that read back with the model
    arrays that were written."""
    import examl_amd.__main__ as cli
    import examl_amd.checkpoint as ckpt
    from examl_amd.examl_io import parse_newick_topology, read_byte_file
    from examl_amd.spr import RfConvergence, SprTree
    monkeypatch.setattr(cli, "_build_engines", _cpu_build_engines)
    written = []
    real_write = ckpt.write_checkpoint

    def recording_write(path, tree, models, *a, **kw):
        written.append((path, [{k: np.array(v, copy=True)
                                for k, v in m.items()} for m in models]))
        return real_write(path, tree, models, *a, **kw)

    monkeypatch.setattr(ckpt, "write_checkpoint", recording_write)
    rc = cli.main(["-s", os.path.join(golden_dir, "12bin.binary"),
                   "-t", os.path.join(golden_dir, "12.tree"),
                   "-n", "D", "-f", "d", "-w", str(tmp_path)], device="cpu")
    assert rc == 0
    lnl = _info_value(os.path.join(tmp_path, "ExaML_info.D"),
                      "Likelihood of best tree:")
    assert abs(lnl - LNL_D_BIN) <= 1e-6 * abs(LNL_D_BIN), lnl

    taxa, _ = read_byte_file(os.path.join(golden_dir, "12bin.binary"))

    def bips(path):
        with open(path) as f:
            t = parse_newick_topology(f.read(), taxa, read_bl=True)
        return {frozenset(b)
                for b in RfConvergence(SprTree.from_phylo(t))._bipartitions()}

    assert bips(os.path.join(tmp_path, "ExaML_result.D")) == \
        bips(os.path.join(golden_dir, "12bin.result.tree"))

    assert written, "-f d wrote no checkpoint for binary data"
    path, models = written[-1]
    ck = ckpt.read_checkpoint(path, 12, [2])
    assert len(ck.models) == 1
    for k in ("EIGN", "EV", "EI", "frequencies", "tipVector", "substRates",
              "gammaRates"):
        assert np.array_equal(_bits(ck.models[0][k]), _bits(models[0][k])), k
    assert ck.models[0]["alpha"] == float(models[0]["alpha"])
    assert ck.models[0]["EV"].shape == (4,)
    assert ck.models[0]["tipVector"].shape == (8,)
    assert ck.models[0]["substRates"].shape == (1,)


def test_cli_binary_other_modes_cpu(golden_dir, tmp_path, monkeypatch):
    """-f e, -a and -f q on the mixed DNA+BIN input, -f o on the pure
    binary one."""
    import examl_amd.__main__ as cli
    monkeypatch.setattr(cli, "_build_engines", _cpu_build_engines)
    base = ["-s", os.path.join(golden_dir, "12mix.binary"),
            "-t", os.path.join(golden_dir, "12.tree"), "-w", str(tmp_path)]
    assert cli.main(base + ["-n", "e", "-f", "e"], device="cpu") == 0
    fast = _info_value(os.path.join(tmp_path, "ExaML_info.e"),
                       "Likelihood tree 0:")
    # the fast mode optimizes less thoroughly than -f E, never better
    assert LNL_E_MIX - 5.0 < fast <= LNL_E_MIX + 1e-3
    assert cli.main(base + ["-n", "a", "-f", "e", "-a"], device="cpu") == 0
    med = _info_value(os.path.join(tmp_path, "ExaML_info.a"),
                      "Likelihood tree 0:")
    assert np.isfinite(med) and med != fast  # median gamma rates differ
    assert cli.main(base + ["-n", "q", "-f", "q", "-r", "12", "-p", "3"],
                    device="cpu") == 0
    qlines = [ln for ln in open(os.path.join(tmp_path, "ExaML_quartets.q"))
              if "|" in ln]
    assert len(qlines) == 3 * 12  # three topologies per quartet
    assert all(float(ln.split(":")[1]) < 0.0 for ln in qlines)
    # -f o (no lnL cutoff) on the pure binary input
    assert cli.main(["-s", os.path.join(golden_dir, "12bin.binary"),
                     "-t", os.path.join(golden_dir, "12.tree"),
                     "-w", str(tmp_path), "-n", "o", "-f", "o"],
                    device="cpu") == 0
    best = _info_value(os.path.join(tmp_path, "ExaML_info.o"),
                       "Likelihood of best tree:")
    assert best >= LNL_E_BIN - 1e-3  # the search never ends below its start


@pytest.mark.parametrize("extra,word", [
    (["-m", "PSR"], "-m PSR"), (["-S"], "-S"), (["-R", "nofile"], "-R")])
def test_cli_binary_refuses_unsupported(golden_dir, tmp_path, monkeypatch,
                                        extra, word):
    import examl_amd.__main__ as cli
    monkeypatch.setattr(cli, "_build_engines", _cpu_build_engines)
    with pytest.raises(SystemExit) as e:
        cli.main(["-s", os.path.join(golden_dir, "12mix.binary"),
                  "-t", os.path.join(golden_dir, "12.tree"),
                  "-n", "X", "-f", "E", "-w", str(tmp_path)] + extra,
                 device="cpu")
    msg = e.value.code
    assert isinstance(msg, str) and "\n" not in msg
    assert "binary" in msg and word in msg


def test_build_engines_routes_binary(golden_dir, monkeypatch):
    """The product factory hands a BIN partition to BinGtrModel +
    DnaGammaEngine (not to the protein branch)."""
    import examl_amd.__main__ as cli
    from examl_amd.examl_io import read_byte_file
    made = []

    class FakeEngine:
        def __init__(self, tips, wgt, model, device=None):
            made.append(model)

    monkeypatch.setattr(ea, "DnaGammaEngine", FakeEngine)
    _, parts = read_byte_file(os.path.join(golden_dir, "12mix.binary"))
    opts = cli._parse_args(["-s", "x", "-n", "y", "-t", "z"])
    engines, auto, _ = cli._build_engines(parts, opts, "cpu")
    assert [type(m).__name__ for m in made] == ["DnaGtrModel", "BinGtrModel"]
    assert auto == [False, False]
    assert np.array_equal(made[1].frequencies, parts[1].frequencies)


def test_tree_search_keeps_binary_out_of_multi_engine(golden_dir,
                                                      monkeypatch):
    """Two dense-GAMMA binary engines on a GPU pass every other condition of
    the fused-partition gate; the state-count condition must keep them on
    the per-partition loop (MultiEngine knows 4 and 20 states only)."""
    import torch

    import examl_amd.engine as engine_mod
    from examl_amd.examl_io import read_byte_file, read_newick_trees
    from examl_amd.search import TreeSearch
    calls = []

    class RecordingMulti:
        def __init__(self, engines):
            calls.append(engines)

    monkeypatch.setattr(engine_mod, "MultiEngine", RecordingMulti)

    class DnaGammaEngine(bin_ref.BinRefEngine):  # the gate looks at the name
        device = torch.device("cuda")

    taxa, parts = read_byte_file(os.path.join(golden_dir, "12bin.binary"))
    p = parts[0]
    engines = [DnaGammaEngine(p.tips, p.wgt,
                              ea.BinGtrModel(p.frequencies, 1.0))
               for _ in range(2)]
    tree = read_newick_trees(os.path.join(golden_dir, "12.tree"), taxa)[0]
    ts = TreeSearch(tree, engines)
    assert ts.fused is None and not calls
    # the same stand-ins with 4 states do reach MultiEngine
    for e in engines:
        e.states = 4
    ts = TreeSearch(tree, engines)
    assert len(calls) == 1 and ts.fused is not None


def test_opt_base_freqs_binary_pass(golden_dir):
    """optBaseFreqs' third pass (optimizeModel.c:1568-1594): with the flag
    set (parser model BINX) the two binary frequencies are optimized and the
    likelihood does not drop; without it they stay as they are."""
    from examl_amd.examl_io import read_byte_file, read_newick_trees
    from examl_amd.search import TreeSearch
    taxa, parts = read_byte_file(os.path.join(golden_dir, "12bin.binary"))
    p = parts[0]
    out = {}
    for flag in (False, True):
        m = ea.BinGtrModel([0.5, 0.5], 1.0)
        eng = bin_ref.BinRefEngine(p.tips, p.wgt, m)
        tree = read_newick_trees(os.path.join(golden_dir, "12.tree"), taxa)[0]
        ts = TreeSearch(tree, [eng], opt_freq_flags=[flag])
        before = ts.evaluate_generic(full=True)
        ts.opt_base_freqs(0.1)
        ts.opt_rates_generic(0.1)  # no rate to optimize: a no-op
        after = ts.evaluate_generic(full=True)
        out[flag] = (before, after, m.frequencies.copy())
    assert out[False][1] == out[False][0]
    assert np.array_equal(out[False][2], [0.5, 0.5])
    assert out[True][1] > out[True][0]
    assert abs(out[True][2].sum() - 1.0) < 1e-12
    assert out[True][2][0] > 0.5  # the data hold more 0s than 1s
