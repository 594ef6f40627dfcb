"""Shared test helpers: synthetic data and the ORACLE-side executor that
replays a product traversal on the CPU restatement (the checker for GPU
parity and host-logic tests)."""

import functools
import glob
import math
import os
import types

import numpy as np

import oracle as O
from examl_amd import INNER_INNER, TIP_INNER, TIP_TIP


def load_golden_parts(golden_dir, stem):
    """Merge the arrays of tests/golden/<stem>.<k>.npz (a fixture set that
    oracle/gen_golden.py stores in parts to keep every file small)."""
    paths = sorted(glob.glob(os.path.join(golden_dir, stem + ".*.npz")))
    assert paths, f"no golden parts for {stem} in {golden_dir}"
    out = {}
    for path in paths:
        with np.load(path) as d:
            for k in d.files:
                assert k not in out, f"{k} stored twice in {stem}"
                out[k] = d[k]
    return out


def make_synthetic(ntips, width, seed=42):
    """Seeded synthetic alignment (delegates to the product generator)."""
    from examl_amd.synthetic import make_alignment
    return make_alignment(ntips, width, seed=seed)


def _model_arrays(model):
    """Aligned copies of a DnaGtrModel's vectors for the oracle's AVX-path
    reference calls."""
    def al(a):
        out = O.aligned(a.shape)
        out[:] = a
        return out
    return (al(model.EIGN), al(model.EV), al(model.EI), al(model.tipVector),
            al(model.gammaRates))


def oracle_full_lnl(entries, root, tree, model, tips, wgt,
                    return_state=False):
    """Replay the product's traversal entries through the CPU oracle
    (newview per entry + recursive scalers + evaluate at the root),
    restating evaluateGeneric end to end.  model.states picks DNA/protein."""
    EIGN, EV, EI, tipVector, g = _model_arrays(model)
    st = model.states
    nv = O.newview_dna_gamma if st == 4 else O.newview_prot_gamma
    ev = O.evaluate_dna_gamma if st == 4 else O.evaluate_prot_gamma
    width = tips.shape[1]
    ntips = tips.shape[0] - 1
    clv = {}
    scalers = np.zeros(2 * ntips, dtype=np.int64)
    wgt = np.ascontiguousarray(wgt, dtype=np.int32)

    for e in entries:
        qz = math.log(e.qz) if e.qz > O.ZMIN else math.log(O.ZMIN)
        rz = math.log(e.rz) if e.rz > O.ZMIN else math.log(O.ZMIN)
        left, right = O.make_p(qz, rz, g, EI, EIGN, 4, st)
        if e.tipCase == TIP_TIP:
            x3, inc = nv(
                TIP_TIP, None, None, EV, tipVector,
                np.ascontiguousarray(tips[e.x1Slot]),
                np.ascontiguousarray(tips[e.x2Slot]), width, left, right, wgt)
        elif e.tipCase == TIP_INNER:
            x3, inc = nv(
                TIP_INNER, None, clv[e.x2Slot], EV, tipVector,
                np.ascontiguousarray(tips[e.x1Slot]), None, width, left,
                right, wgt)
        else:
            x3, inc = nv(
                INNER_INNER, clv[e.x1Slot], clv[e.x2Slot], EV, tipVector,
                None, None, width, left, right, wgt)
        clv[e.x3Slot] = x3
        scalers[e.pNumber] = scalers[e.qNumber] + scalers[e.rNumber] + inc

    p, q, z = root
    diag = O.calc_diagptable(z, st, 4, g, EIGN)
    p_tip, q_tip = tree.is_tip(p), tree.is_tip(q)
    if q_tip:
        lnl = ev(wgt, None, clv[tree.clv_slot(p)],
                 tipVector, np.ascontiguousarray(tips[q]), width, diag)
    elif p_tip:
        lnl = ev(wgt, None, clv[tree.clv_slot(q)],
                 tipVector, np.ascontiguousarray(tips[p]), width, diag)
    else:
        lnl = ev(wgt, clv[tree.clv_slot(p)],
                 clv[tree.clv_slot(q)], tipVector, None, width, diag)
    lnl += float(scalers[p] + scalers[q]) * math.log(O.MINLIKELIHOOD)
    if return_state:
        return lnl, clv, scalers
    return lnl


def make_synthetic_aa(ntips, width, seed=42):
    """Seeded synthetic protein alignment (codes 1..22)."""
    rng = np.random.default_rng(seed)
    tips = np.zeros((ntips + 1, width), dtype=np.uint8)
    base = rng.integers(1, 21, width).astype(np.uint8)
    for t in range(1, ntips + 1):
        row = base.copy()
        mut = rng.random(width) < 0.15
        row[mut] = rng.integers(1, 21, int(mut.sum())).astype(np.uint8)
        amb = rng.random(width) < 0.01
        row[amb] = rng.integers(1, 23, int(amb.sum())).astype(np.uint8)
        tips[t] = row
    wgt = np.ones(width, dtype=np.int32)
    return tips, wgt


class OracleEngine:
    """CPU engine with the SAME interface as DnaGammaEngine, executing the
    oracle kernels — lets examl_amd.search.TreeSearch run end to end on the
    CPU restatement (the checker for the GPU search path, and the vehicle
    for the testData/49 -f E parity anchor)."""

    def __init__(self, tips, wgt, model):
        self.model = model
        self.ntips = tips.shape[0] - 1
        self.width = tips.shape[1]
        self.tips = tips
        self.wgt = np.ascontiguousarray(wgt, dtype=np.int32)
        self.host_tips = np.ascontiguousarray(tips)
        self.host_wgt = self.wgt
        self.clv = {}
        self.scalers = np.zeros(2 * self.ntips, dtype=np.int64)
        self.sumtable = None
        self._nv = O.newview_dna_gamma if model.states == 4 \
            else O.newview_prot_gamma
        self._ev = O.evaluate_dna_gamma if model.states == 4 \
            else O.evaluate_prot_gamma
        self._sum = O.sum_dna_gamma if model.states == 4 else O.sum_prot_gamma
        self._core = O.core_dna_gamma if model.states == 4 \
            else O.core_prot_gamma

    def upload_model(self):
        pass  # oracle reads model arrays directly per call

    def _arrays(self):
        return _model_arrays(self.model)

    def newview_traversal(self, entries):
        EIGN, EV, EI, tipVector, g = self._arrays()
        st = self.model.states
        for e in entries:
            qz = math.log(e.qz) if e.qz > O.ZMIN else math.log(O.ZMIN)
            rz = math.log(e.rz) if e.rz > O.ZMIN else math.log(O.ZMIN)
            left, right = O.make_p(qz, rz, g, EI, EIGN, 4, st)
            if e.tipCase == TIP_TIP:
                x3, inc = self._nv(
                    TIP_TIP, None, None, EV, tipVector,
                    np.ascontiguousarray(self.tips[e.x1Slot]),
                    np.ascontiguousarray(self.tips[e.x2Slot]), self.width,
                    left, right, self.wgt)
            elif e.tipCase == TIP_INNER:
                x3, inc = self._nv(
                    TIP_INNER, None, self.clv[e.x2Slot], EV, tipVector,
                    np.ascontiguousarray(self.tips[e.x1Slot]), None,
                    self.width, left, right, self.wgt)
            else:
                x3, inc = self._nv(
                    INNER_INNER, self.clv[e.x1Slot], self.clv[e.x2Slot], EV,
                    tipVector, None, None, self.width, left, right, self.wgt)
            self.clv[e.x3Slot] = x3
            self.scalers[e.pNumber] = (self.scalers[e.qNumber] +
                                       self.scalers[e.rNumber] + inc)

    def evaluate_root(self, tree, p, q, z):
        EIGN, EV, EI, tipVector, g = self._arrays()
        st = self.model.states
        diag = O.calc_diagptable(z, st, 4, g, EIGN)
        p_tip, q_tip = tree.is_tip(p), tree.is_tip(q)
        if q_tip:
            lnl = self._ev(self.wgt, None, self.clv[tree.clv_slot(p)],
                           tipVector, np.ascontiguousarray(self.tips[q]),
                           self.width, diag)
        elif p_tip:
            lnl = self._ev(self.wgt, None, self.clv[tree.clv_slot(q)],
                           tipVector, np.ascontiguousarray(self.tips[p]),
                           self.width, diag)
        else:
            lnl = self._ev(self.wgt, self.clv[tree.clv_slot(p)],
                           self.clv[tree.clv_slot(q)], tipVector, None,
                           self.width, diag)
        lnl += float(self.scalers[p] + self.scalers[q]) * \
            math.log(O.MINLIKELIHOOD)
        return lnl

    def sum_root(self, tree, p, q):
        EIGN, EV, EI, tipVector, g = self._arrays()
        p_tip, q_tip = tree.is_tip(p), tree.is_tip(q)
        if p_tip and q_tip:
            self.sumtable = self._sum(
                TIP_TIP, None, None, tipVector,
                np.ascontiguousarray(self.tips[p]),
                np.ascontiguousarray(self.tips[q]), self.width)
        elif q_tip:
            self.sumtable = self._sum(
                TIP_INNER, None, self.clv[tree.clv_slot(p)], tipVector,
                np.ascontiguousarray(self.tips[q]), None, self.width)
        elif p_tip:
            self.sumtable = self._sum(
                TIP_INNER, None, self.clv[tree.clv_slot(q)], tipVector,
                np.ascontiguousarray(self.tips[p]), None, self.width)
        else:
            self.sumtable = self._sum(
                INNER_INNER, self.clv[tree.clv_slot(p)],
                self.clv[tree.clv_slot(q)], tipVector, None, None,
                self.width)

    def core_derivs(self, lz):
        EIGN, EV, EI, tipVector, g = self._arrays()
        return self._core(self.width, self.sumtable, EIGN, g, lz, self.wgt)

    def core_derivs_async(self, lz):
        return self.core_derivs(lz)


class OracleCatEngine(OracleEngine):
    """CPU CAT (PSR) engine with the DnaCatEngine interface — lets
    TreeSearch(rate_het="CAT") run fully on the oracle kernels (the checker
    for the GPU PSR path and the vehicle for the 49 -f E -m PSR anchor)."""

    def __init__(self, tips, wgt, model, cptr, per_site_rates):
        super().__init__(tips, wgt, model)
        self.cptr = np.ascontiguousarray(cptr, dtype=np.int32)
        self.per_site_rates = np.ascontiguousarray(per_site_rates,
                                                   dtype=np.float64)
        self.num_cats = len(self.per_site_rates)

    def set_site_rates(self, cptr, per_site_rates):
        self.cptr = np.ascontiguousarray(cptr, dtype=np.int32)
        self.per_site_rates = np.ascontiguousarray(per_site_rates,
                                                   dtype=np.float64)
        self.num_cats = len(self.per_site_rates)

    def _rptr(self):
        r = O.aligned(self.num_cats)
        r[:] = self.per_site_rates
        return r

    def newview_traversal(self, entries):
        EIGN, EV, EI, tipVector, _ = self._arrays()
        rptr = self._rptr()
        for e in entries:
            qz = math.log(e.qz) if e.qz > O.ZMIN else math.log(O.ZMIN)
            rz = math.log(e.rz) if e.rz > O.ZMIN else math.log(O.ZMIN)
            left, right = O.make_p(qz, rz, rptr, EI, EIGN, self.num_cats, 4)
            if e.tipCase == TIP_TIP:
                x3, inc = O.newview_dna_cat(
                    TIP_TIP, EV, self.cptr, None, None, tipVector,
                    np.ascontiguousarray(self.tips[e.x1Slot]),
                    np.ascontiguousarray(self.tips[e.x2Slot]), self.width,
                    left, right, self.wgt)
            elif e.tipCase == TIP_INNER:
                x3, inc = O.newview_dna_cat(
                    TIP_INNER, EV, self.cptr, None, self.clv[e.x2Slot],
                    tipVector, np.ascontiguousarray(self.tips[e.x1Slot]),
                    None, self.width, left, right, self.wgt)
            else:
                x3, inc = O.newview_dna_cat(
                    INNER_INNER, EV, self.cptr, self.clv[e.x1Slot],
                    self.clv[e.x2Slot], tipVector, None, None, self.width,
                    left, right, self.wgt)
            self.clv[e.x3Slot] = x3
            self.scalers[e.pNumber] = (self.scalers[e.qNumber] +
                                       self.scalers[e.rNumber] + inc)

    def evaluate_root(self, tree, p, q, z):
        EIGN, EV, EI, tipVector, _ = self._arrays()
        diag = O.calc_diagptable(z, 4, self.num_cats, self._rptr(), EIGN)
        p_tip, q_tip = tree.is_tip(p), tree.is_tip(q)
        if q_tip:
            lnl = O.evaluate_dna_cat(
                self.cptr, self.wgt, None, self.clv[tree.clv_slot(p)],
                tipVector, np.ascontiguousarray(self.tips[q]), self.width,
                diag)
        elif p_tip:
            lnl = O.evaluate_dna_cat(
                self.cptr, self.wgt, None, self.clv[tree.clv_slot(q)],
                tipVector, np.ascontiguousarray(self.tips[p]), self.width,
                diag)
        else:
            lnl = O.evaluate_dna_cat(
                self.cptr, self.wgt, self.clv[tree.clv_slot(p)],
                self.clv[tree.clv_slot(q)], tipVector, None, self.width,
                diag)
        lnl += float(self.scalers[p] + self.scalers[q]) * \
            math.log(O.MINLIKELIHOOD)
        return lnl

    def sum_root(self, tree, p, q):
        EIGN, EV, EI, tipVector, _ = self._arrays()
        p_tip, q_tip = tree.is_tip(p), tree.is_tip(q)
        if p_tip and q_tip:
            self.sumtable = O.sum_dna_cat(
                TIP_TIP, None, None, tipVector,
                np.ascontiguousarray(self.tips[p]),
                np.ascontiguousarray(self.tips[q]), self.width)
        elif q_tip:
            self.sumtable = O.sum_dna_cat(
                TIP_INNER, None, self.clv[tree.clv_slot(p)], tipVector,
                np.ascontiguousarray(self.tips[q]), None, self.width)
        elif p_tip:
            self.sumtable = O.sum_dna_cat(
                TIP_INNER, None, self.clv[tree.clv_slot(q)], tipVector,
                np.ascontiguousarray(self.tips[p]), None, self.width)
        else:
            self.sumtable = O.sum_dna_cat(
                INNER_INNER, self.clv[tree.clv_slot(p)],
                self.clv[tree.clv_slot(q)], tipVector, None, None,
                self.width)

    def core_derivs(self, lz):
        EIGN, EV, EI, tipVector, _ = self._arrays()
        return O.core_dna_cat(self.width, self.num_cats, self.sumtable,
                              self.wgt, self._rptr(), EIGN, self.cptr, lz)


class OracleProtCatEngine(OracleCatEngine):
    """CPU protein CAT (PSR) engine over the oracle prot-CAT kernels."""

    def newview_traversal(self, entries):
        EIGN, EV, EI, tipVector, _ = self._arrays()
        rptr = self._rptr()
        for e in entries:
            qz = math.log(e.qz) if e.qz > O.ZMIN else math.log(O.ZMIN)
            rz = math.log(e.rz) if e.rz > O.ZMIN else math.log(O.ZMIN)
            left, right = O.make_p(qz, rz, rptr, EI, EIGN, self.num_cats, 20)
            if e.tipCase == TIP_TIP:
                x3, inc = O.newview_prot_cat(
                    TIP_TIP, EV, self.cptr, None, None, tipVector,
                    np.ascontiguousarray(self.tips[e.x1Slot]),
                    np.ascontiguousarray(self.tips[e.x2Slot]), self.width,
                    left, right, self.wgt)
            elif e.tipCase == TIP_INNER:
                x3, inc = O.newview_prot_cat(
                    TIP_INNER, EV, self.cptr, None, self.clv[e.x2Slot],
                    tipVector, np.ascontiguousarray(self.tips[e.x1Slot]),
                    None, self.width, left, right, self.wgt)
            else:
                x3, inc = O.newview_prot_cat(
                    INNER_INNER, EV, self.cptr, self.clv[e.x1Slot],
                    self.clv[e.x2Slot], tipVector, None, None, self.width,
                    left, right, self.wgt)
            self.clv[e.x3Slot] = x3
            self.scalers[e.pNumber] = (self.scalers[e.qNumber] +
                                       self.scalers[e.rNumber] + inc)

    def evaluate_root(self, tree, p, q, z):
        EIGN, EV, EI, tipVector, _ = self._arrays()
        diag = O.calc_diagptable(z, 20, self.num_cats, self._rptr(), EIGN)
        p_tip, q_tip = tree.is_tip(p), tree.is_tip(q)
        if q_tip:
            lnl = O.evaluate_prot_cat(
                self.cptr, self.wgt, None, self.clv[tree.clv_slot(p)],
                tipVector, np.ascontiguousarray(self.tips[q]), self.width,
                diag)
        elif p_tip:
            lnl = O.evaluate_prot_cat(
                self.cptr, self.wgt, None, self.clv[tree.clv_slot(q)],
                tipVector, np.ascontiguousarray(self.tips[p]), self.width,
                diag)
        else:
            lnl = O.evaluate_prot_cat(
                self.cptr, self.wgt, self.clv[tree.clv_slot(p)],
                self.clv[tree.clv_slot(q)], tipVector, None, self.width,
                diag)
        lnl += float(self.scalers[p] + self.scalers[q]) * \
            math.log(O.MINLIKELIHOOD)
        return lnl

    def sum_root(self, tree, p, q):
        EIGN, EV, EI, tipVector, _ = self._arrays()
        p_tip, q_tip = tree.is_tip(p), tree.is_tip(q)
        if p_tip and q_tip:
            self.sumtable = O.sum_prot_cat(
                TIP_TIP, None, None, tipVector,
                np.ascontiguousarray(self.tips[p]),
                np.ascontiguousarray(self.tips[q]), self.width)
        elif q_tip:
            self.sumtable = O.sum_prot_cat(
                TIP_INNER, None, self.clv[tree.clv_slot(p)], tipVector,
                np.ascontiguousarray(self.tips[q]), None, self.width)
        elif p_tip:
            self.sumtable = O.sum_prot_cat(
                TIP_INNER, None, self.clv[tree.clv_slot(q)], tipVector,
                np.ascontiguousarray(self.tips[p]), None, self.width)
        else:
            self.sumtable = O.sum_prot_cat(
                INNER_INNER, self.clv[tree.clv_slot(p)],
                self.clv[tree.clv_slot(q)], tipVector, None, None,
                self.width)

    def core_derivs(self, lz):
        EIGN, EV, EI, tipVector, _ = self._arrays()
        return O.core_prot_cat(self.width, self.num_cats, self.sumtable,
                               self.wgt, self._rptr(), EIGN, self.cptr, lz)


def oracle_makenewz(entries, root, tree, model, tips, wgt, z0, maxiter=64):
    """CPU restatement of topLevelMakenewz (numBranches=1) over the oracle
    sum/core kernels — the checker for DnaGammaEngine.makenewz."""
    EIGN, EV, EI, tipVector, g = _model_arrays(model)
    states = model.states
    sum_fn = O.sum_dna_gamma if states == 4 else O.sum_prot_gamma
    core_fn = O.core_dna_gamma if states == 4 else O.core_prot_gamma
    width = tips.shape[1]
    _, clv, _ = oracle_full_lnl(entries, root, tree, model, tips, wgt,
                                return_state=True)
    p, q, _ = root
    p_tip, q_tip = tree.is_tip(p), tree.is_tip(q)
    wgt = np.ascontiguousarray(wgt, dtype=np.int32)
    if p_tip and q_tip:
        st = sum_fn(TIP_TIP, None, None, tipVector,
                    np.ascontiguousarray(tips[p]),
                    np.ascontiguousarray(tips[q]), width)
    elif q_tip:
        st = sum_fn(TIP_INNER, None, clv[tree.clv_slot(p)],
                    tipVector, np.ascontiguousarray(tips[q]), None, width)
    elif p_tip:
        st = sum_fn(TIP_INNER, None, clv[tree.clv_slot(q)],
                    tipVector, np.ascontiguousarray(tips[p]), None, width)
    else:
        st = sum_fn(INNER_INNER, clv[tree.clv_slot(p)],
                    clv[tree.clv_slot(q)], tipVector, None, None, width)

    z = float(z0)
    zprev, zstep = z, (1.0 - O.ZMAX) * z + O.ZMIN
    curvat_ok, outer_converged, it = True, False, maxiter
    while not outer_converged:
        if curvat_ok:
            curvat_ok = False
            zprev = z
            zstep = (1.0 - O.ZMAX) * z + O.ZMIN
        z = min(max(z, O.ZMIN), O.ZMAX)
        lz = math.log(z)
        dlnL, d2lnL = core_fn(width, st, EIGN, g, lz, wgt)
        if (d2lnL >= 0.0) and (z < O.ZMAX):
            zprev = z = 0.37 * z + 0.63
            continue
        curvat_ok = True
        if d2lnL < 0.0:
            tantmp = -dlnL / d2lnL
            if tantmp < 100:
                z *= math.exp(tantmp)
                z = max(z, O.ZMIN)
                z = min(z, 0.25 * zprev + 0.75)
            else:
                z = 0.25 * zprev + 0.75
        z = min(z, O.ZMAX)
        it -= 1
        if abs(z - zprev) > zstep:
            if it < -20:
                z = float(z0)
                outer_converged = True
        else:
            outer_converged = True
    return z


def oracle_cat_full_lnl(entries, root, tree, model, tips, wgt, cptr,
                        per_site_rates, return_state=False):
    """CAT replay of a product traversal on the oracle kernels (the
    checker for DnaCatEngine)."""
    EIGN, EV, EI, tipVector, _ = _model_arrays(model)
    rptr = O.aligned(len(per_site_rates))
    rptr[:] = per_site_rates
    num_cats = len(per_site_rates)
    width = tips.shape[1]
    ntips = tips.shape[0] - 1
    cptr = np.ascontiguousarray(cptr, dtype=np.int32)
    wgt = np.ascontiguousarray(wgt, dtype=np.int32)
    clv = {}
    scalers = np.zeros(2 * ntips, dtype=np.int64)
    for e in entries:
        qz = math.log(e.qz) if e.qz > O.ZMIN else math.log(O.ZMIN)
        rz = math.log(e.rz) if e.rz > O.ZMIN else math.log(O.ZMIN)
        left, right = O.make_p(qz, rz, rptr, EI, EIGN, num_cats, 4)
        if e.tipCase == TIP_TIP:
            x3, inc = O.newview_dna_cat(
                TIP_TIP, EV, cptr, None, None, tipVector,
                np.ascontiguousarray(tips[e.x1Slot]),
                np.ascontiguousarray(tips[e.x2Slot]), width, left, right,
                wgt)
        elif e.tipCase == TIP_INNER:
            x3, inc = O.newview_dna_cat(
                TIP_INNER, EV, cptr, None, clv[e.x2Slot], tipVector,
                np.ascontiguousarray(tips[e.x1Slot]), None, width, left,
                right, wgt)
        else:
            x3, inc = O.newview_dna_cat(
                INNER_INNER, EV, cptr, clv[e.x1Slot], clv[e.x2Slot],
                tipVector, None, None, width, left, right, wgt)
        clv[e.x3Slot] = x3
        scalers[e.pNumber] = scalers[e.qNumber] + scalers[e.rNumber] + inc
    p, q, z = root
    diag = O.calc_diagptable(z, 4, num_cats, rptr, EIGN)
    p_tip, q_tip = tree.is_tip(p), tree.is_tip(q)
    if q_tip:
        lnl = O.evaluate_dna_cat(cptr, wgt, None, clv[tree.clv_slot(p)],
                                 tipVector, np.ascontiguousarray(tips[q]),
                                 width, diag)
    elif p_tip:
        lnl = O.evaluate_dna_cat(cptr, wgt, None, clv[tree.clv_slot(q)],
                                 tipVector, np.ascontiguousarray(tips[p]),
                                 width, diag)
    else:
        lnl = O.evaluate_dna_cat(cptr, wgt, clv[tree.clv_slot(p)],
                                 clv[tree.clv_slot(q)], tipVector, None,
                                 width, diag)
    lnl += float(scalers[p] + scalers[q]) * math.log(O.MINLIKELIHOOD)
    if return_state:
        return lnl, clv, scalers
    return lnl


class OracleLg4Engine(OracleEngine):
    """CPU LG4 (LG4M/LG4X) engine — per-category matrices through the
    oracle LG4 kernels (the checker for the GPU LG4 path)."""

    def __init__(self, tips, wgt, model):
        super().__init__(tips, wgt, model)

    def newview_traversal(self, entries):
        m = self.model
        for e in entries:
            qz = math.log(e.qz) if e.qz > O.ZMIN else math.log(O.ZMIN)
            rz = math.log(e.rz) if e.rz > O.ZMIN else math.log(O.ZMIN)
            left, right = O.make_p_lg4(qz, rz, m.gammaRates, m.EI4, m.EIGN4)
            if e.tipCase == TIP_TIP:
                x3, inc = O.newview_prot_lg4(
                    TIP_TIP, None, None, m.EV4, m.tipVector4,
                    np.ascontiguousarray(self.tips[e.x1Slot]),
                    np.ascontiguousarray(self.tips[e.x2Slot]), self.width,
                    left, right, self.wgt)
            elif e.tipCase == TIP_INNER:
                x3, inc = O.newview_prot_lg4(
                    TIP_INNER, None, self.clv[e.x2Slot], m.EV4, m.tipVector4,
                    np.ascontiguousarray(self.tips[e.x1Slot]), None,
                    self.width, left, right, self.wgt)
            else:
                x3, inc = O.newview_prot_lg4(
                    INNER_INNER, self.clv[e.x1Slot], self.clv[e.x2Slot],
                    m.EV4, m.tipVector4, None, None, self.width, left,
                    right, self.wgt)
            self.clv[e.x3Slot] = x3
            self.scalers[e.pNumber] = (self.scalers[e.qNumber] +
                                       self.scalers[e.rNumber] + inc)

    def evaluate_root(self, tree, p, q, z):
        m = self.model
        diag = O.calc_diagptable_lg4(z, m.gammaRates, m.EIGN4)
        p_tip, q_tip = tree.is_tip(p), tree.is_tip(q)
        if q_tip:
            lnl = O.evaluate_prot_lg4(
                self.wgt, None, self.clv[tree.clv_slot(p)], m.tipVector4,
                np.ascontiguousarray(self.tips[q]), self.width, diag,
                m.weights)
        elif p_tip:
            lnl = O.evaluate_prot_lg4(
                self.wgt, None, self.clv[tree.clv_slot(q)], m.tipVector4,
                np.ascontiguousarray(self.tips[p]), self.width, diag,
                m.weights)
        else:
            lnl = O.evaluate_prot_lg4(
                self.wgt, self.clv[tree.clv_slot(p)],
                self.clv[tree.clv_slot(q)], m.tipVector4, None, self.width,
                diag, m.weights)
        lnl += float(self.scalers[p] + self.scalers[q]) * \
            math.log(O.MINLIKELIHOOD)
        return lnl

    def sum_root(self, tree, p, q):
        m = self.model
        p_tip, q_tip = tree.is_tip(p), tree.is_tip(q)
        if p_tip and q_tip:
            self.sumtable = O.sum_prot_lg4(
                TIP_TIP, None, None, m.tipVector4,
                np.ascontiguousarray(self.tips[p]),
                np.ascontiguousarray(self.tips[q]), self.width)
        elif q_tip:
            self.sumtable = O.sum_prot_lg4(
                TIP_INNER, None, self.clv[tree.clv_slot(p)], m.tipVector4,
                np.ascontiguousarray(self.tips[q]), None, self.width)
        elif p_tip:
            self.sumtable = O.sum_prot_lg4(
                TIP_INNER, None, self.clv[tree.clv_slot(q)], m.tipVector4,
                np.ascontiguousarray(self.tips[p]), None, self.width)
        else:
            self.sumtable = O.sum_prot_lg4(
                INNER_INNER, self.clv[tree.clv_slot(p)],
                self.clv[tree.clv_slot(q)], m.tipVector4, None, None,
                self.width)

    def core_derivs(self, lz):
        m = self.model
        return O.core_prot_lg4(self.width, self.sumtable, m.EIGN4,
                               m.gammaRates, m.weights, lz, self.wgt)


class OracleSaveEngine(OracleEngine):
    """CPU -S (saveMemory) DNA engine over the oracle SAVE kernels: gap
    vectors, gap columns and compacted CLV slabs (the checker for
    SaveDnaEngine)."""

    def __init__(self, tips, wgt, model):
        super().__init__(tips, wgt, model)
        assert model.states == 4
        self.gvl = self.width // 32 + 1
        nn = 2 * self.ntips
        self.gap = np.zeros((nn, self.gvl), dtype=np.uint32)
        for t in range(1, self.ntips + 1):
            idx = np.nonzero(tips[t] == 15)[0]
            np.bitwise_or.at(self.gap[t], idx // 32,
                             (np.uint32(1) << (idx % 32).astype(np.uint32)))
        self.gapcol = {}

    def _gapcol_tip(self):
        _, _, _, tipVector, _ = self._arrays()
        return np.ascontiguousarray(tipVector[15 * 4:16 * 4])

    def newview_traversal(self, entries):
        EIGN, EV, EI, tipVector, g = self._arrays()
        import ctypes as C
        dp = lambda a: (a.ctypes.data_as(C.POINTER(C.c_double))
                        if a is not None else C.cast(None,
                                                     C.POINTER(C.c_double)))
        up = lambda a: (a.ctypes.data_as(C.POINTER(C.c_uint))
                        if a is not None else C.cast(None,
                                                     C.POINTER(C.c_uint)))
        u8 = lambda a: (a.ctypes.data_as(C.POINTER(C.c_ubyte))
                        if a is not None else C.cast(None,
                                                     C.POINTER(C.c_ubyte)))
        for e in entries:
            qz = math.log(e.qz) if e.qz > O.ZMIN else math.log(O.ZMIN)
            rz = math.log(e.rz) if e.rz > O.ZMIN else math.log(O.ZMIN)
            left, right = O.make_p(qz, rz, g, EI, EIGN, 4, 4)
            p, q, r = e.pNumber, e.qNumber, e.rNumber
            self.gap[p] = self.gap[q] & self.gap[r]
            nz = self.width - int(
                np.unpackbits(self.gap[p].view(np.uint8),
                              bitorder="little")[:self.width].sum())
            x3 = O.aligned(max(nz, 1) * 16)
            gcol3 = O.aligned(16)
            q_tip = e.tipCase != INNER_INNER
            r_tip = e.tipCase == TIP_TIP
            gc1 = self._gapcol_tip() if q_tip else self.gapcol[e.x1Slot]
            gc2 = self._gapcol_tip() if r_tip else self.gapcol[e.x2Slot]
            inc = C.c_int(0)
            O._orc.oracle_newview_dna_gamma_save(
                C.c_int(e.tipCase),
                dp(None if q_tip else self.clv[e.x1Slot]),
                dp(None if r_tip else self.clv[e.x2Slot]),
                dp(x3), dp(EV), dp(tipVector),
                u8(np.ascontiguousarray(self.tips[e.x1Slot])
                   if q_tip else None),
                u8(np.ascontiguousarray(self.tips[e.x2Slot])
                   if r_tip else None),
                C.c_int(self.width), dp(left), dp(right),
                self.wgt.ctypes.data_as(C.POINTER(C.c_int)),
                C.byref(inc), up(self.gap[q]), up(self.gap[r]),
                up(self.gap[p]), dp(gc1), dp(gc2), dp(gcol3))
            self.clv[e.x3Slot] = x3
            self.gapcol[e.x3Slot] = gcol3
            self.scalers[p] = self.scalers[q] + self.scalers[r] + inc.value

    def evaluate_root(self, tree, p, q, z):
        EIGN, EV, EI, tipVector, g = self._arrays()
        import ctypes as C
        diag = O.calc_diagptable(z, 4, 4, g, EIGN)
        dp = lambda a: (a.ctypes.data_as(C.POINTER(C.c_double))
                        if a is not None else C.cast(None,
                                                     C.POINTER(C.c_double)))
        up = lambda a: (a.ctypes.data_as(C.POINTER(C.c_uint))
                        if a is not None else C.cast(None,
                                                     C.POINTER(C.c_uint)))
        O._orc.oracle_evaluate_dna_gamma_save.restype = C.c_double
        p_tip, q_tip = tree.is_tip(p), tree.is_tip(q)
        if q_tip or p_tip:
            tip, inner = (q, p) if q_tip else (p, q)
            sl = tree.clv_slot(inner)
            lnl = O._orc.oracle_evaluate_dna_gamma_save(
                self.wgt.ctypes.data_as(C.POINTER(C.c_int)), dp(None),
                dp(self.clv[sl]), dp(tipVector),
                np.ascontiguousarray(self.tips[tip]).ctypes.data_as(
                    C.POINTER(C.c_ubyte)),
                C.c_int(self.width), dp(diag), dp(None),
                dp(self.gapcol[sl]), up(None), up(self.gap[inner]))
        else:
            s1, s2 = tree.clv_slot(p), tree.clv_slot(q)
            lnl = O._orc.oracle_evaluate_dna_gamma_save(
                self.wgt.ctypes.data_as(C.POINTER(C.c_int)),
                dp(self.clv[s1]), dp(self.clv[s2]), dp(tipVector),
                C.cast(None, C.POINTER(C.c_ubyte)), C.c_int(self.width),
                dp(diag), dp(self.gapcol[s1]), dp(self.gapcol[s2]),
                up(self.gap[p]), up(self.gap[q]))
        lnl += float(self.scalers[p] + self.scalers[q]) * \
            math.log(O.MINLIKELIHOOD)
        return lnl

    def sum_root(self, tree, p, q):
        EIGN, EV, EI, tipVector, g = self._arrays()
        import ctypes as C
        dp = lambda a: (a.ctypes.data_as(C.POINTER(C.c_double))
                        if a is not None else C.cast(None,
                                                     C.POINTER(C.c_double)))
        up = lambda a: (a.ctypes.data_as(C.POINTER(C.c_uint))
                        if a is not None else C.cast(None,
                                                     C.POINTER(C.c_uint)))
        u8 = lambda a: (a.ctypes.data_as(C.POINTER(C.c_ubyte))
                        if a is not None else C.cast(None,
                                                     C.POINTER(C.c_ubyte)))
        self.sumtable = O.aligned(self.width * 16)
        p_tip, q_tip = tree.is_tip(p), tree.is_tip(q)
        if p_tip and q_tip:
            O._orc.oracle_sum_dna_gamma_save(
                0, dp(self.sumtable), dp(None), dp(None), dp(tipVector),
                u8(np.ascontiguousarray(self.tips[p])),
                u8(np.ascontiguousarray(self.tips[q])),
                C.c_int(self.width), dp(None), dp(None), up(None), up(None))
        elif q_tip or p_tip:
            tip, inner = (q, p) if q_tip else (p, q)
            sl = tree.clv_slot(inner)
            O._orc.oracle_sum_dna_gamma_save(
                1, dp(self.sumtable), dp(None), dp(self.clv[sl]),
                dp(tipVector), u8(np.ascontiguousarray(self.tips[tip])),
                u8(None), C.c_int(self.width), dp(None),
                dp(self.gapcol[sl]), up(None), up(self.gap[inner]))
        else:
            s1, s2 = tree.clv_slot(p), tree.clv_slot(q)
            O._orc.oracle_sum_dna_gamma_save(
                2, dp(self.sumtable), dp(self.clv[s1]), dp(self.clv[s2]),
                dp(tipVector), u8(None), u8(None), C.c_int(self.width),
                dp(self.gapcol[s1]), dp(self.gapcol[s2]), up(self.gap[p]),
                up(self.gap[q]))

    def clv_bytes(self):
        return sum(v.nbytes for v in self.clv.values())


# ---------------------------------------------------------------------------
# Edge-input builders for tests/test_kernel_edges.py: ragged widths, sites
# that sit on either side of the 2^-256 rescale threshold next to each
# other, and a longdouble reference for the reduction kernels.
# ---------------------------------------------------------------------------

EDGE_FAMILIES = ("dna_gamma", "prot_gamma", "dna_cat")
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _al(a, dtype=np.float64):
    out = O.aligned(np.shape(a), dtype)
    out[...] = a
    return out


@functools.lru_cache(maxsize=None)
def edge_family(family):
    """Model block, P pair, diag table and oracle entry points of one kernel
    family.  `cats` is the number of categories inside one site's span (4
    for GAMMA, 1 for CAT); `num_cats` the number of P/diag rows."""
    import examl_amd as ea
    f = types.SimpleNamespace(name=family)
    md = np.load(os.path.join(_GOLDEN, "model_dna.npz"))
    if family == "prot_gamma":
        m = ea.ProtGtrModel.lg(alpha=0.62)
        f.states, f.cats, f.ncodes = 20, 4, 23
    else:
        m = ea.DnaGtrModel(md["m1_freqs"], md["m1_rates6"],
                           float(md["m1_alpha"]))
        f.states, f.cats, f.ncodes = 4, (1 if family == "dna_cat" else 4), 16
    f.model = m
    f.span = f.states * f.cats
    f.EIGN, f.EV, f.EI, f.tipVector = (_al(m.EIGN), _al(m.EV), _al(m.EI),
                                       _al(m.tipVector))
    if family == "dna_cat":
        k = np.load(os.path.join(_GOLDEN, "kernels_dna_cat.npz"))
        f.rates = _al(k["rptr"])
    else:
        f.rates = _al(m.gammaRates)
    f.num_cats = len(f.rates)
    f.z_q, f.z_r, f.z_root, f.lz = 0.84, 0.18, 0.6, -0.65
    f.left, f.right = O.make_p(math.log(f.z_q), math.log(f.z_r), f.rates,
                               f.EI, f.EIGN, f.num_cats, f.states)
    f.diag = O.calc_diagptable(f.z_root, f.states, f.num_cats, f.rates,
                               f.EIGN)
    return f


def edge_newview(f, tc, x1, x2, t1, t2, n, wgt, cptr):
    """Oracle newview of family block `f` -> (x3, inc)."""
    a1 = x1 if tc == INNER_INNER else None
    a2 = x2 if tc != TIP_TIP else None
    u1 = t1 if tc != INNER_INNER else None
    u2 = t2 if tc == TIP_TIP else None
    if f.name == "dna_cat":
        return O.newview_dna_cat(tc, f.EV, cptr, a1, a2, f.tipVector, u1, u2,
                                 n, f.left, f.right, wgt)
    nv = O.newview_dna_gamma if f.states == 4 else O.newview_prot_gamma
    return nv(tc, a1, a2, f.EV, f.tipVector, u1, u2, n, f.left, f.right, wgt)


def edge_sum(f, tc, c):
    """Oracle sum table for the operands of edge case `c`."""
    a1 = c.x1 if tc == INNER_INNER else None
    a2 = c.x2 if tc != TIP_TIP else None
    u1 = c.tipX1 if tc != INNER_INNER else None
    u2 = c.tipX2 if tc == TIP_TIP else None
    fn = {"dna_gamma": O.sum_dna_gamma, "prot_gamma": O.sum_prot_gamma,
          "dna_cat": O.sum_dna_cat}[f.name]
    return fn(tc, a1, a2, f.tipVector, u1, u2, c.n)


def edge_evaluate(f, c, tip):
    """Oracle lnL (no scaler undo) at the operands of `c`; `tip` selects
    the tip body (x1 row = tipVector[tipX1])."""
    x1 = None if tip else c.x1
    t1 = c.tipX1 if tip else None
    if f.name == "dna_cat":
        return O.evaluate_dna_cat(c.cptr, c.wgt, x1, c.x2, f.tipVector, t1,
                                  c.n, f.diag)
    ev = O.evaluate_dna_gamma if f.states == 4 else O.evaluate_prot_gamma
    return ev(c.wgt, x1, c.x2, f.tipVector, t1, c.n, f.diag)


def edge_core(f, c, sumtable):
    """Oracle (dlnL, d2lnL) for `sumtable` at f.lz."""
    if f.name == "dna_cat":
        return O.core_dna_cat(c.n, f.num_cats, sumtable, c.wgt, f.rates,
                              f.EIGN, c.cptr, f.lz)
    core = O.core_dna_gamma if f.states == 4 else O.core_prot_gamma
    return core(c.n, sumtable, f.EIGN, f.rates, f.lz, c.wgt)


def edge_core_dtables(f):
    """The host-built derivative tables the core kernels read (the product's
    examl_host_core_dtables_*), as a float64 array."""
    import ctypes
    import examl_amd as ea
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    if f.name == "dna_cat":
        out = np.zeros(f.num_cats * 4 + 8 + f.num_cats)
        ea.lib().examl_host_core_dtables_dna_cat(
            vp(f.EIGN), vp(f.rates), f.num_cats, ctypes.c_double(f.lz),
            vp(out))
    elif f.states == 4:
        out = np.zeros(48)
        ea.lib().examl_host_core_dtables_dna(vp(f.EIGN), vp(f.rates),
                                             ctypes.c_double(f.lz), vp(out))
    else:
        out = np.zeros(240)
        ea.lib().examl_host_core_dtables_prot(vp(f.EIGN), vp(f.rates),
                                              ctypes.c_double(f.lz), vp(out))
    return out


def _binade(a):
    """floor(log2(a)) of positive finite doubles."""
    return np.frexp(a)[1].astype(np.int64) - 1


# The five site classes of make_rescale_mix.  CAT has one category per
# span, so "every category tiny" is the same site as class 1 and "one
# category blocks the vote" the same as class 2.
_CAT_CLASS = {0: 0, 1: 1, 2: 2, 3: 1, 4: 2}
RESCALING_CLASSES = (1, 3)


def edge_classes(family):
    return (0, 1, 2) if family == "dna_cat" else (0, 1, 2, 3, 4)


def make_rescale_mix(family, tc, n, seed):
    """Operands for one newview call in which neighbouring sites fall on
    both sides of the 2^-256 rescale threshold, with the expected x3 and
    scalerInc known BY CONSTRUCTION.

    x1/x2 are uniform in [0.01, 1), wgt in 1..4, tip codes random.  One
    unscaled oracle newview gives x3_0.  Multiplying the (site, cat) block
    of the inner operand x2 by 2^k multiplies that block of x3_0 by exactly
    2^k (every product and sum commutes with a power of two while nothing
    goes subnormal; all exponents here stay above -900).  With e the binade
    of a site's span maximum and e_c of category c's maximum, each site
    draws a class:

      0  unscaled                                        -> no rescale
      1  whole site * 2^(-257-e): max in [2^-257,2^-256) -> rescale
      2  whole site * 2^(-256-e): max in [2^-256,2^-255) -> no rescale
      3  category c * 2^(-300-e_c) for every c           -> rescale
      4  as 3, one random category * 2^(-256-e_c)        -> no rescale
         (a single category above the threshold blocks the all-span vote)

    Expected x3 = x3_0 * 2^k, times 2^256 on classes 1 and 3; expected
    inc = sum(wgt[class in (1, 3)]).  TIP_TIP never rescales: plain
    operands, inc 0.  Returns a namespace with the operands (x1, x2,
    tipX1, tipX2, wgt, cptr), x3, inc and the per-site classes."""
    f = edge_family(family)
    rng = np.random.default_rng(seed)
    S, C = f.states, f.cats
    x1 = _al(rng.uniform(0.01, 1.0, n * f.span))
    x2 = _al(rng.uniform(0.01, 1.0, n * f.span))
    wgt = np.ascontiguousarray(rng.integers(1, 5, n), dtype=np.int32)
    t1 = np.ascontiguousarray(rng.integers(1, f.ncodes, n), dtype=np.uint8)
    t2 = np.ascontiguousarray(rng.integers(1, f.ncodes, n), dtype=np.uint8)
    cptr = np.ascontiguousarray(rng.integers(0, f.num_cats, n),
                                dtype=np.int32)
    classes = rng.integers(0, 5, n)
    blocker = rng.integers(0, C, n)
    if family == "dna_cat":
        classes = np.array([_CAT_CLASS[int(k)] for k in classes],
                           dtype=np.int64)
    c = types.SimpleNamespace(family=family, tc=tc, n=n, x1=x1, x2=x2,
                              tipX1=t1, tipX2=t2, wgt=wgt, cptr=cptr)
    x3_0, inc0 = edge_newview(f, tc, x1, x2, t1, t2, n, wgt, cptr)
    assert inc0 == 0, "unscaled operands must not rescale"
    if tc == TIP_TIP:
        c.classes = np.zeros(n, dtype=np.int64)
        c.x3, c.inc = x3_0, 0
        return c

    cmax = np.abs(x3_0).reshape(n, C, S).max(axis=2)
    assert (cmax > 0).all()
    e_c = _binade(cmax)                       # [n, C]
    e = e_c.max(axis=1)                       # [n]
    k = np.zeros((n, C), dtype=np.int64)
    k[classes == 1] = (-257 - e[classes == 1])[:, None]
    k[classes == 2] = (-256 - e[classes == 2])[:, None]
    k[classes == 3] = -300 - e_c[classes == 3]
    k4 = -300 - e_c
    rows = np.arange(n)
    k4[rows, blocker] = -256 - e_c[rows, blocker]
    k[classes == 4] = k4[classes == 4]
    assert k.min() > -700

    x2[:] = np.ldexp(x2.reshape(n, C, S), k[:, :, None]).reshape(-1)
    up = np.isin(classes, RESCALING_CLASSES)
    kx = k + 256 * up[:, None]
    c.x3 = np.ldexp(x3_0.reshape(n, C, S), kx[:, :, None]).reshape(-1)
    c.inc = int(wgt[up].sum())
    c.classes = classes
    return c


def tile_edge_case(c, n):
    """Operands of `c` tiled along the site axis and truncated to n sites
    (expected values are NOT tiled: callers run the oracle once at n)."""
    f = edge_family(c.family)
    reps = -(-n // c.n)
    t = types.SimpleNamespace(family=c.family, tc=c.tc, n=n)
    t.x1 = _al(np.tile(c.x1, reps)[:n * f.span])
    t.x2 = _al(np.tile(c.x2, reps)[:n * f.span])
    t.tipX1 = np.ascontiguousarray(np.tile(c.tipX1, reps)[:n])
    t.tipX2 = np.ascontiguousarray(np.tile(c.tipX2, reps)[:n])
    t.wgt = np.ascontiguousarray(np.tile(c.wgt, reps)[:n])
    t.cptr = np.ascontiguousarray(np.tile(c.cptr, reps)[:n])
    t.classes = np.tile(c.classes, reps)[:n]
    return t


# -- longdouble reference for the reductions --------------------------------
# Per-site terms restate the formulas in the kernel header comments of
# examl_amd/csrc/examl_hip.hip (not oracle code), evaluated in np.longdouble
# and totalled with math.fsum.  Each function returns (total, abs_total)
# where abs_total = sum_i |w_i * term_i| is what the tolerances scale with.

LNL_RTOL = 1e-12     # the suite's existing rtol for lnL (test_gpu_parity)
DERIV_RTOL = 1e-11   # ... and for the NR derivatives

_LD_CHUNK = 1 << 16


def _fsum2(parts):
    v = np.concatenate(parts).astype(np.float64)
    return math.fsum(v), math.fsum(np.abs(v))


def ld_lnl(f, c, tip):
    """sum_i wgt_i * log(0.25*|sum_{c,k} x1*x2*diag|) for GAMMA;
    sum_i wgt_i * log(|sum_k x1*x2*diag[cptr_i]|) for CAT (no 0.25)."""
    L = np.longdouble
    S, C, n = f.states, f.cats, c.n
    diag = np.asarray(f.diag).astype(L).reshape(f.num_cats, S)
    tv = np.asarray(f.tipVector).astype(L).reshape(f.ncodes, S)
    parts = []
    for lo in range(0, n, _LD_CHUNK):
        hi = min(n, lo + _LD_CHUNK)
        b = c.x2[lo * f.span:hi * f.span].astype(L).reshape(-1, C, S)
        if tip:
            a = tv[c.tipX1[lo:hi]][:, None, :]
        else:
            a = c.x1[lo * f.span:hi * f.span].astype(L).reshape(-1, C, S)
        if f.name == "dna_cat":
            d = diag[c.cptr[lo:hi]][:, None, :]
            site = np.log(np.abs((a * b * d).sum(axis=(1, 2))))
        else:
            site = np.log(L(0.25) *
                          np.abs((a * b * diag[None]).sum(axis=(1, 2))))
        parts.append(c.wgt[lo:hi].astype(L) * site)
    return _fsum2(parts)


def ld_core(f, c, sumtable, dtab):
    """GAMMA: tmp = d0*sum; a0 = S tmp; a1 = S tmp*d1; a2 = S tmp*d2 over
    (c,k); inv = 1/|a0|; dlnL += w*(a1*inv); d2lnL += w*(a2*inv -
    (a1*inv)^2).  CAT: d row of the site's category, e1/e2 shared, weights
    r*w and r*r*w.  dtab is edge_core_dtables(f).  Returns
    ((d1, abs1), (d2, abs2))."""
    L = np.longdouble
    S, C, n = f.states, f.cats, c.n
    dt = np.asarray(dtab).astype(L)
    p1, p2 = [], []
    for lo in range(0, n, _LD_CHUNK):
        hi = min(n, lo + _LD_CHUNK)
        s = sumtable[lo * f.span:hi * f.span].astype(L).reshape(-1, C, S)
        w = c.wgt[lo:hi].astype(L)
        if f.name == "dna_cat":
            nc = f.num_cats
            d = dt[:nc * 4].reshape(nc, 4)[c.cptr[lo:hi]][:, None, :]
            e1 = dt[nc * 4:nc * 4 + 4][None, None, :]
            e2 = dt[nc * 4 + 4:nc * 4 + 8][None, None, :]
            r = dt[nc * 4 + 8:][c.cptr[lo:hi]]
            tmp = d * s
            w1, w2 = r * w, r * r * w
        else:
            m = C * S
            d0 = dt[:m].reshape(1, C, S)
            e1 = dt[m:2 * m].reshape(1, C, S)
            e2 = dt[2 * m:3 * m].reshape(1, C, S)
            tmp = d0 * s
            w1 = w2 = w
        inv = 1 / np.abs(tmp.sum(axis=(1, 2)))
        dl = (tmp * e1).sum(axis=(1, 2)) * inv
        d2l = (tmp * e2).sum(axis=(1, 2)) * inv
        p1.append(w1 * dl)
        p2.append(w2 * (d2l - dl * dl))
    return _fsum2(p1), _fsum2(p2)


# -- deep trees for the engine-level and fused rescaling tests --------------
# Caterpillars with long branches (z = 0.1) over random_tips data, sized
# with the oracle engines on the CPU; the tests re-assert
# scalers.max() > 0.  DEEP_TIPS_PROT is the smallest count at which both
# protein CAT and LG4 rescale at width 77 (CAT alone: 50).  The fused
# GAMMA partitions first rescale at 55 (protein) and 116 (DNA) tips; a
# 4-state CLV loses only ~2 bits per level where a 20-state one loses ~5,
# so the DNA case cannot share the protein tree.  The fused counts sit a
# few levels above those minima so that more than one site rescales.
DEEP_Z = 0.1
DEEP_TIPS_PROT = 54
DEEP_TIPS_FUSED = {20: 60, 4: 120}   # widths (37, 131, 1, 260)


def deep_caterpillar(ntips):
    from examl_amd import PhyloTree
    return PhyloTree.caterpillar(ntips, z=DEEP_Z)


AA_CODES = tuple(range(1, 21))
DNA_BASES = (1, 2, 4, 8)


def prot_cat_inputs(ntips, width, seed):
    """(tips, wgt, model, cptr, rates) for the protein CAT engines."""
    import examl_amd as ea
    aa = np.load(os.path.join(os.path.dirname(_GOLDEN), os.pardir,
                              "examl_amd", "data", "aa_models.npz"))
    tips, wgt = random_tips(ntips, width, AA_CODES, seed)
    rng = np.random.default_rng(seed + 1)
    rates = np.array([0.2, 0.6, 1.0, 1.7, 3.0])
    cptr = rng.integers(0, len(rates), width).astype(np.int32)
    model = ea.ProtGtrModel(aa["frequencies"][4], aa["rates190"][4], 1.0)
    return tips, wgt, model, cptr, rates


def fused_deep_inputs(states, widths=(37, 131, 1, 260), seed=5):
    """Per-partition (tips, wgt, model) on the deep caterpillar for the
    fused-path rescaling case of tests/test_multi_fused.py."""
    import examl_amd as ea
    ntips = DEEP_TIPS_FUSED[states]
    rng = np.random.default_rng(seed)
    aa = np.load(os.path.join(os.path.dirname(_GOLDEN), os.pardir,
                              "examl_amd", "data", "aa_models.npz"))
    parts = []
    for i, w in enumerate(widths):
        if states == 4:
            tips, wgt = random_tips(ntips, w, DNA_BASES, seed + i)
            freqs = rng.uniform(0.1, 0.4, 4)
            freqs /= freqs.sum()
            rates = list(rng.uniform(0.3, 3.0, 5)) + [1.0]
            m = ea.DnaGtrModel(list(freqs), rates,
                               alpha=float(rng.uniform(0.2, 1.5)))
        else:
            tips, wgt = random_tips(ntips, w, AA_CODES, seed + i)
            m = ea.ProtGtrModel(aa["frequencies"][4 + i % 3],
                                aa["rates190"][4 + i % 3],
                                float(rng.uniform(0.4, 1.2)))
        parts.append((tips, wgt, m))
    return ntips, parts


def random_tips(ntips, width, codes, seed):
    """Uniformly random tip rows (no conserved columns, so CLV magnitudes
    fall as fast as the tree allows) and pattern weights in 1..3."""
    rng = np.random.default_rng(seed)
    codes = np.asarray(codes, dtype=np.uint8)
    tips = np.zeros((ntips + 1, width), dtype=np.uint8)
    tips[1:] = codes[rng.integers(0, len(codes), (ntips, width))]
    wgt = rng.integers(1, 4, width).astype(np.int32)
    return tips, wgt


def edge_identity_family(family):
    """`edge_family` with EV = P_left = P_right = I and tipVector = 1, so
    that newview computes x3 = x1 * x2 exactly and a test can place values
    ON the rescale threshold."""
    f = edge_family(family)
    g = types.SimpleNamespace(**vars(f))
    S = f.states
    eye = np.eye(S).reshape(-1)
    g.EV = _al(eye)
    g.tipVector = _al(np.ones(f.ncodes * S))
    g.left = _al(np.tile(eye, f.num_cats))
    g.right = _al(np.tile(eye, f.num_cats))
    return g


def make_threshold_exact(family, tc):
    """Eight sites for the identity model whose span maxima are exactly
    2^-256 (must NOT rescale: the rule is strict <), one ulp below it, and
    2^-257 with and without a single entry on the threshold.  Returns the
    case with expected x3/inc by construction."""
    f = edge_identity_family(family)
    T = O.MINLIKELIHOOD
    n, span = 8, f.span
    below = np.nextafter(T, 0.0)
    rows = np.empty((n, span))
    rows[0] = T                      # every entry on the threshold: stays
    rows[1] = T / 2                  # rescales
    rows[2] = T / 2
    rows[2, span - 1] = T            # one entry on the threshold: stays
    rows[3] = below                  # one ulp under: rescales
    rows[4] = 1.0
    rows[5], rows[6], rows[7] = rows[0], rows[1], rows[2]
    rows[7, span - 1], rows[7, 0] = T / 2, T
    scale = np.array([0, 1, 0, 1, 0, 0, 1, 0], dtype=bool)
    c = types.SimpleNamespace(family=family, tc=tc, n=n)
    c.x1 = _al(np.ones(n * span))
    c.x2 = _al(rows.reshape(-1))
    c.tipX1 = np.arange(1, n + 1, dtype=np.uint8)
    c.tipX2 = np.arange(2, n + 2, dtype=np.uint8)
    c.wgt = np.array([1, 2, 4, 8, 16, 32, 64, 128], dtype=np.int32)
    c.cptr = (np.arange(n) % f.num_cats).astype(np.int32)
    c.x3 = (rows * np.where(scale, O.TWOTOTHE256, 1.0)[:, None]).reshape(-1)
    c.inc = int(c.wgt[scale].sum())
    c.classes = scale.astype(np.int64)
    return f, c
