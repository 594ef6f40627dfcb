"""How the binary (two-state) golden fixtures were generated (not run in CI).

Needs the reference artifacts that `make -C oracle` builds where the
reference sources are present (oracle/_ref/libref.so, parse-examl,
examl-AVX):

    python tests/golden/gen_bin.py            # everything
    python tests/golden/gen_bin.py kernels    # bin_kernels.npz only
    python tests/golden/gen_bin.py e2e        # alignments + reference runs

Kernel vectors (bin_kernels.npz)
  The reference's own compiled kernels, called through ctypes on 16-byte
  aligned buffers: newviewGTRGAMMA_BINARY, evaluateGTRGAMMA_BINARY,
  sumGAMMA_BINARY, coreGTRGAMMA_BINARY, plus initGeneric (n = 2, bit vector
  0..3), makeP, calcDiagptable and makeGammaCats for the model inputs.
  newview runs in all three tipCases on three magnitude regimes, N = 96
  sites each:
    norm  ordinary magnitudes, nothing rescales;
    tiny  inner operands * 1e-90, every site rescales (TIP_INNER and
          INNER_INNER; TIP_TIP never rescales);
    mix   even sites ordinary, odd sites tiny, plus two built sites:
          site 1: 7 of its 8 outputs below 2^-256 and one above -> must not
                  rescale;
          site 3: one output exactly 2^-256, the other 7 below -> must not
                  rescale (the compare is strict).
          The built operands are found by a search over the numpy
          restatement (tests/bin_ref.py) and then CHECKED on the reference's
          output; the generator also asserts that the reference rescales
          some sites of the mix and leaves others.

End-to-end fixtures
  Alignment: 12 taxa T01..T12, a random-walk 0/1 matrix (root row mutated at
  15% per join of a random join order, numpy default_rng(2024)), 300
  columns, 3% of the cells replaced by '?' and 2% by '-'.
    12bin.binary  parse-examl -s 12bin.phy -m BIN -n 12bin
    12mix.binary  parse-examl -s 12mix.phy -q mix.part -m DNA -n 12mix
                  12mix.phy = 200 random-walk DNA columns (default_rng(2025))
                  followed by the first 200 binary columns;
                  mix.part: "DNA, p1 = 1-200" / "BIN, p2 = 201-400"
  Starting tree: the existing 12.tree.

  Goldens (reference examl-AVX -m GAMMA on these inputs):
    -f E     12bin.binary      -1234.713639
    -f E     12mix.binary      -2626.066536
    -f E -M  12mix.binary      -2504.119971
    -f d     12bin.binary      -1065.065040   (+ 12bin.result.tree)
"""

import ctypes
import math
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, ROOT)
REF = os.path.join(ROOT, "oracle", "_ref")

from tests import bin_ref  # noqa: E402

TIP_TIP, TIP_INNER, INNER_INNER = 0, 1, 2
THR = 2.0 ** -256
N = 96


def aligned(n, dtype=np.float64, alignment=64):
    dtype = np.dtype(dtype)
    buf = np.zeros(n * dtype.itemsize + alignment, dtype=np.uint8)
    off = (-buf.ctypes.data) % alignment
    return buf[off:off + n * dtype.itemsize].view(dtype)


def al(a):
    out = aligned(len(a))
    out[:] = a
    return out


def dp(a):
    assert a.dtype == np.float64 and a.ctypes.data % 16 == 0
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def up(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte))


# ---- the reference's functions -------------------------------------------

def ref_init(ref, freqs):
    vv = np.arange(4, dtype=np.uint32)
    EIGN, EV, EI, tv = aligned(2), aligned(4), aligned(4), aligned(8)
    f = al(np.asarray(freqs, dtype=np.float64))
    r = al(np.array([1.0]))
    ref.initGeneric(ctypes.c_int(2),
                    vv.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)),
                    ctypes.c_int(4), dp(EIGN), dp(EV), dp(EI), dp(f), dp(r),
                    dp(tv), ctypes.c_int(0))
    return EIGN, EV, EI, tv


def ref_gamma(ref, alpha):
    g = aligned(4)
    ref.makeGammaCats(ctypes.c_double(alpha), dp(g), ctypes.c_int(4),
                      ctypes.c_int(0))
    return g


def ref_make_p(ref, z1, z2, g, EI, EIGN):
    P = aligned(32)
    left, right = P[:16], P[16:]
    ref.makeP(ctypes.c_double(z1), ctypes.c_double(z2), dp(g), dp(EI),
              dp(EIGN), ctypes.c_int(4), dp(left), dp(right), ctypes.c_int(0),
              ctypes.c_int(4), ctypes.c_int(2))
    return left, right


def ref_diag(ref, z, g, EIGN):
    d = aligned(8)
    ref.calcDiagptable(ctypes.c_double(z), ctypes.c_int(2), ctypes.c_int(4),
                       dp(g), dp(EIGN), dp(d))
    return d


def ref_newview(ref, tc, x1, x2, EV, tv, t1, t2, n, left, right, wgt):
    x3 = aligned(n * 8)
    inc = ctypes.c_int(0)
    null_d = ctypes.POINTER(ctypes.c_double)()
    null_u = ctypes.POINTER(ctypes.c_ubyte)()
    ref.newviewGTRGAMMA_BINARY(
        ctypes.c_int(tc), dp(x1) if x1 is not None else null_d,
        dp(x2) if x2 is not None else null_d, dp(x3), dp(EV), dp(tv),
        ctypes.POINTER(ctypes.c_int)(),
        up(t1) if t1 is not None else null_u,
        up(t2) if t2 is not None else null_u, ctypes.c_int(n), dp(left),
        dp(right), ip(wgt), ctypes.byref(inc), ctypes.c_int(1))
    return x3, inc.value


def ref_evaluate(ref, wgt, x1, x2, tv, t1, n, diag):
    ref.evaluateGTRGAMMA_BINARY.restype = ctypes.c_double
    null_d = ctypes.POINTER(ctypes.c_double)()
    null_u = ctypes.POINTER(ctypes.c_ubyte)()
    null_i = ctypes.POINTER(ctypes.c_int)()
    return ref.evaluateGTRGAMMA_BINARY(
        null_i, null_i, ip(wgt), dp(x1) if x1 is not None else null_d,
        dp(x2), dp(tv), up(t1) if t1 is not None else null_u,
        ctypes.c_int(n), dp(diag), ctypes.c_int(1))


def ref_sum(ref, tc, x1, x2, tv, t1, t2, n):
    st = aligned(n * 8)
    null_d = ctypes.POINTER(ctypes.c_double)()
    null_u = ctypes.POINTER(ctypes.c_ubyte)()
    ref.sumGAMMA_BINARY(
        ctypes.c_int(tc), dp(st), dp(x1) if x1 is not None else null_d,
        dp(x2) if x2 is not None else null_d, dp(tv),
        up(t1) if t1 is not None else null_u,
        up(t2) if t2 is not None else null_u, ctypes.c_int(n))
    return st


def ref_core(ref, n, st, EIGN, g, lz, wgt):
    d1, d2 = ctypes.c_double(0), ctypes.c_double(0)
    ref.coreGTRGAMMA_BINARY(ctypes.c_int(n), dp(st), ctypes.byref(d1),
                            ctypes.byref(d2), dp(EIGN), dp(g),
                            ctypes.c_double(lz), ip(wgt))
    return d1.value, d2.value


# ---- built sites of the mix regime ----------------------------------------

def _site_out(tc, x1s, x2s, code, EV, tv, left, right):
    """The 8 outputs of one site BEFORE any rescaling, by the arithmetic of
    tests/bin_ref.newview (the rescale decision needs the raw values)."""
    t1 = np.array([code], dtype=np.uint8)
    L = left.reshape(4, 2, 2)
    R = right.reshape(4, 2, 2)
    a = (x1s.reshape(4, 2) if tc == INNER_INNER
         else np.broadcast_to(tv.reshape(4, 2)[t1[0]], (4, 2)))
    b = x2s.reshape(4, 2)
    x3 = np.zeros((4, 2))
    for l in range(2):
        alv = a[:, 0] * L[:, l, 0] + a[:, 1] * L[:, l, 1]
        arv = b[:, 0] * R[:, l, 0] + b[:, 1] * R[:, l, 1]
        x3 = x3 + (alv * arv)[:, None] * EV.reshape(2, 2)[l][None, :]
    return x3.reshape(8)


def build_site(tc, code, EV, tv, left, right, want_exact, rng):
    """Operands (x1[8], x2[8]) of a site whose cat-2 pair holds the one
    output at (want_exact) or above 2^-256 while the other 7 stay below."""
    for _try in range(200):
        x1s = rng.uniform(0.2, 1.0, 8)
        x2s = rng.uniform(0.2, 1.0, 8) * 1e-90
        if tc == INNER_INNER:
            x1s = x1s * 1e-90
        # cat 2: operands (u, 0) and (v, 0), v carries the magnitude
        x1s[4:6] = (1.0, 0.0)
        x2s[4:6] = (1.0, 0.0)
        unit = _site_out(tc, x1s, x2s, code, EV, tv, left, right)[4:6]
        j = int(np.argmax(np.abs(unit)))
        if abs(unit[1 - j]) >= 0.95 * abs(unit[j]):
            continue
        v0 = (THR if want_exact else 1.04 * THR) / abs(unit[j])
        cands = [v0]
        if want_exact:
            # walk the neighbouring doubles on both sides of v0
            lo = v0
            for _ in range(2000):
                lo = np.nextafter(lo, 0.0)
            cands = [lo]
            for _ in range(4000):
                cands.append(np.nextafter(cands[-1], 1.0))
        for v in cands:
            x2s[4] = v
            out = _site_out(tc, x1s, x2s, code, EV, tv, left, right)
            big = np.abs(out) >= THR
            if big.sum() != 1 or not big[4 + j]:
                continue
            if want_exact and abs(out[4 + j]) != THR:
                continue
            return x1s, x2s
    raise AssertionError("no operand found for the built site")


def gen_kernels():
    ref = ctypes.CDLL(os.path.join(REF, "libref.so"))
    rng = np.random.default_rng(20261021)
    out = {}

    # --- eigen blocks for two frequency vectors, P blocks ------------------
    models = {"m0": ([0.5, 0.5], 1.0), "m1": ([0.37, 0.63], 0.47)}
    for name, (freqs, alpha) in models.items():
        EIGN, EV, EI, tv = ref_init(ref, freqs)
        g = ref_gamma(ref, alpha)
        out[f"{name}_freqs"] = np.array(freqs)
        out[f"{name}_alpha"] = np.float64(alpha)
        for k, v in (("EIGN", EIGN), ("EV", EV), ("EI", EI),
                     ("tipVector", tv), ("gammaRates", g)):
            out[f"{name}_{k}"] = v.copy()
        zq, zr = (0.81, 0.13) if name == "m1" else (0.9, 1e-20)
        lq = np.log(max(zq, 1e-15))
        lr = np.log(max(zr, 1e-15))
        left, right = ref_make_p(ref, lq, lr, g, EI, EIGN)
        out[f"{name}_p_z"] = np.array([zq, zr])
        out[f"{name}_p_logz"] = np.array([lq, lr])
        out[f"{name}_left"] = left.copy()
        out[f"{name}_right"] = right.copy()

    EIGN, EV, EI, tv = (al(out["m1_EIGN"]), al(out["m1_EV"]),
                        al(out["m1_EI"]), al(out["m1_tipVector"]))
    g = al(out["m1_gammaRates"])
    P = al(np.concatenate([out["m1_left"], out["m1_right"]]))
    left, right = P[:16], P[16:]

    n = N
    wgt = np.ascontiguousarray(rng.integers(1, 5, n), dtype=np.int32)
    tipX1 = np.ascontiguousarray(rng.integers(1, 4, n), dtype=np.uint8)
    tipX2 = np.ascontiguousarray(rng.integers(1, 4, n), dtype=np.uint8)
    out["wgt"], out["tipX1"], out["tipX2"] = wgt, tipX1, tipX2

    base1 = rng.uniform(0.01, 1.0, n * 8)
    base2 = rng.uniform(0.01, 1.0, n * 8)
    odd = np.repeat(np.arange(n) % 2 == 1, 8)
    for tag in ("norm", "tiny", "mix"):
        for tc in (TIP_TIP, TIP_INNER, INNER_INNER):
            if tag == "norm":
                x1, x2 = base1.copy(), base2.copy()
            elif tag == "tiny":
                x1, x2 = base1 * 1e-90, base2 * 1e-90
            else:
                x1 = np.where(odd, base1 * 1e-90, base1)
                x2 = np.where(odd, base2 * 1e-90, base2)
                if tc != TIP_TIP:
                    for site, exact in ((1, False), (3, True)):
                        s1, s2 = build_site(tc, int(tipX1[site]), EV, tv,
                                            left, right, exact, rng)
                        x1[site * 8:site * 8 + 8] = s1
                        x2[site * 8:site * 8 + 8] = s2
            x1, x2 = al(x1), al(x2)
            a1 = x1 if tc == INNER_INNER else None
            a2 = x2 if tc != TIP_TIP else None
            t1 = tipX1 if tc != INNER_INNER else None
            t2 = tipX2 if tc == TIP_TIP else None
            x3, inc = ref_newview(ref, tc, a1, a2, EV, tv, t1, t2, n, left,
                                  right, wgt)
            if a1 is not None:
                out[f"{tag}_tc{tc}_x1"] = x1.copy()
            if a2 is not None:
                out[f"{tag}_tc{tc}_x2"] = x2.copy()
            out[f"{tag}_tc{tc}_x3"] = x3.copy()
            out[f"{tag}_tc{tc}_inc"] = np.int64(inc)
            # the numpy restatement agrees with the reference bit for bit
            y3, yinc = bin_ref.newview(tc, a1, a2, EV, tv, t1, t2, n, left,
                                       right, wgt)
            assert np.array_equal(y3, x3) and yinc == inc, (tag, tc)
            if tc == TIP_TIP:
                assert inc == 0
                continue
            # which sites did the reference rescale?  A rescaled site has
            # raw outputs all < 2^-256; recover the raw values from numpy
            raw = np.stack([
                _site_out(tc, x1[i * 8:i * 8 + 8], x2[i * 8:i * 8 + 8],
                          int(tipX1[i]), EV, tv, left, right)
                for i in range(n)])
            scaled = (raw != x3.reshape(n, 8)).any(axis=1)
            assert inc == int(wgt[scaled].sum())
            out[f"{tag}_tc{tc}_scaled"] = scaled
            if tag == "norm":
                assert scaled.sum() == 0
            elif tag == "tiny":
                assert scaled.all()
            else:
                assert 0 < scaled.sum() < n, "mix must do both"
                # site 1: seven below, one above; site 3: one exactly equal
                for site, exact in ((1, False), (3, True)):
                    r = np.abs(raw[site])
                    assert (r >= THR).sum() == 1 and not scaled[site]
                    assert ((r == THR).sum() == 1) == exact
                    assert np.array_equal(raw[site], x3.reshape(n, 8)[site])

    # --- evaluate / sum / core on the ordinary inputs ----------------------
    x1, x2 = al(base1), al(base2)
    z_root = 0.77
    diag = ref_diag(ref, z_root, g, EIGN)
    out["z_root"] = np.float64(z_root)
    out["diag"] = diag.copy()
    out["eval_II"] = np.float64(
        ref_evaluate(ref, wgt, x1, x2, tv, None, n, diag))
    out["eval_TIP"] = np.float64(
        ref_evaluate(ref, wgt, None, x2, tv, tipX1, n, diag))
    lz = float(np.log(0.61))
    out["lz_core"] = np.float64(lz)
    for tc in (TIP_TIP, TIP_INNER, INNER_INNER):
        a1 = x1 if tc == INNER_INNER else None
        a2 = x2 if tc != TIP_TIP else None
        t1 = tipX1 if tc != INNER_INNER else None
        t2 = tipX2 if tc == TIP_TIP else None
        st = ref_sum(ref, tc, a1, a2, tv, t1, t2, n)
        out[f"sum_tc{tc}"] = st.copy()
        d1, d2 = ref_core(ref, n, st, EIGN, g, lz, wgt)
        out[f"core_tc{tc}_d1"] = np.float64(d1)
        out[f"core_tc{tc}_d2"] = np.float64(d2)
    # the d-tables as coreGTRGAMMA_BINARY's prologue builds them
    # (makenewzGenericSpecial.c:1484-1496), in numpy float64
    # in Python floats: the same IEEE products, and libm's exp
    dt = np.zeros(24)
    e1 = float(EIGN[1])
    for i in range(4):
        ki = float(g[i])
        dt[2 * i] = 1.0
        dt[2 * i + 1] = math.exp(e1 * ki * lz)
        dt[8 + 2 * i + 1] = e1 * ki
        dt[16 + 2 * i + 1] = e1 * e1 * (ki * ki)
    out["dtab_core"] = dt
    np.savez_compressed(os.path.join(HERE, "bin_kernels.npz"), **out)
    print("bin_kernels.npz:", len(out), "arrays")


# ---- end-to-end fixtures ---------------------------------------------------

def random_walk(ntaxa, ncols, nstates, seed, rate=0.15):
    rng = np.random.default_rng(seed)
    rows = [rng.integers(0, nstates, ncols)]
    while len(rows) < ntaxa:
        parent = rows[rng.integers(0, len(rows))]
        child = parent.copy()
        hit = rng.random(ncols) < rate
        child[hit] = rng.integers(0, nstates, int(hit.sum()))
        rows.append(child)
    return np.array(rows), rng


def write_phy(path, rows):
    with open(path, "w") as f:
        f.write(f"{len(rows)} {len(rows[0])}\n")
        for i, r in enumerate(rows):
            f.write(f"T{i + 1:02d} {r}\n")


def run_ref(td, args):
    r = subprocess.run([os.path.join(REF, "examl-AVX")] + args, cwd=td,
                       capture_output=True, text=True, check=True)
    return r.stdout


def gen_e2e():
    mat, rng = random_walk(12, 300, 2, 2024)
    chars = np.array(["0", "1"])[mat]
    miss = rng.random(mat.shape)
    chars[miss < 0.03] = "?"
    chars[(miss >= 0.03) & (miss < 0.05)] = "-"
    bin_rows = ["".join(r) for r in chars]
    dna, _ = random_walk(12, 200, 4, 2025)
    dna_rows = ["".join(r) for r in np.array(list("ACGT"))[dna]]
    mix_rows = [d + b[:200] for d, b in zip(dna_rows, bin_rows)]

    with tempfile.TemporaryDirectory() as td:
        write_phy(os.path.join(td, "12bin.phy"), bin_rows)
        write_phy(os.path.join(td, "12mix.phy"), mix_rows)
        with open(os.path.join(td, "mix.part"), "w") as f:
            f.write("DNA, p1 = 1-200\nBIN, p2 = 201-400\n")
        parse = os.path.join(REF, "parse-examl")
        subprocess.run([parse, "-s", "12bin.phy", "-m", "BIN", "-n", "12bin"],
                       cwd=td, check=True, capture_output=True)
        subprocess.run([parse, "-s", "12mix.phy", "-q", "mix.part", "-m",
                        "DNA", "-n", "12mix"], cwd=td, check=True,
                       capture_output=True)
        for f in ("12bin.binary", "12mix.binary"):
            shutil.copy(os.path.join(td, f), os.path.join(HERE, f))
        shutil.copy(os.path.join(HERE, "12.tree"), td)
        for tag, args in (
                ("E bin", ["-s", "12bin.binary", "-f", "E"]),
                ("E mix", ["-s", "12mix.binary", "-f", "E"]),
                ("E -M mix", ["-s", "12mix.binary", "-f", "E", "-M"]),
                ("d bin", ["-s", "12bin.binary", "-f", "d"])):
            name = tag.replace(" ", "").replace("-", "")
            log = run_ref(td, args + ["-t", "12.tree", "-m", "GAMMA", "-n",
                                      name])
            info = open(os.path.join(td, f"ExaML_info.{name}")).read()
            for ln in (log + info).splitlines():
                if ("Likelihood tree 0" in ln or "Likelihood of best" in ln
                        or "DataType" in ln):
                    print(tag, "|", ln.strip())
            if tag == "d bin":
                shutil.copy(os.path.join(td, f"ExaML_result.{name}"),
                            os.path.join(HERE, "12bin.result.tree"))


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what in ("all", "kernels"):
        gen_kernels()
    if what in ("all", "e2e"):
        gen_e2e()
