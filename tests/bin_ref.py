"""Vectorised numpy restatement of the reference's four binary (two-state)
GTRGAMMA kernels, in the reference's operation order, plus a CPU engine
with the interface of tests.helpers.OracleEngine built on them.

  newview   newviewGTRGAMMA_BINARY  (newviewGenericSpecial.c:6034)
  evaluate  evaluateGTRGAMMA_BINARY (evaluateGenericSpecial.c:1074)
  sum       sumGAMMA_BINARY         (makenewzGenericSpecial.c:1543)
  core      coreGTRGAMMA_BINARY     (makenewzGenericSpecial.c:1464)

numpy's elementwise float64 +, * are IEEE operations with no contraction,
so newview and sum reproduce the reference bit for bit; evaluate and core
differ only in the order of the final sum over sites (tests pin both
against tests/golden/bin_kernels.npz).  TEST INFRASTRUCTURE ONLY.

Layouts: CLV x[site, cat, state] (8 doubles per site), P blocks
left[cat, row, col], tipVector[code, state], EV[row, col].
"""

import math

import numpy as np

from examl_amd import INNER_INNER, TIP_INNER, TIP_TIP, ZMIN, lib
from examl_amd.engine import DnaGammaEngine

TWOTOTHE256 = 2.0 ** 256
MINLIKELIHOOD = 2.0 ** -256


def _vp(a):
    import ctypes
    return a.ctypes.data_as(ctypes.c_void_p)


def newview(tip_case, x1, x2, EV, tipVector, tipX1, tipX2, n, left, right,
            wgt):
    """Returns (x3 [n*8], scaler increment)."""
    L = np.asarray(left, dtype=np.float64).reshape(4, 2, 2)
    R = np.asarray(right, dtype=np.float64).reshape(4, 2, 2)
    ev = np.asarray(EV, dtype=np.float64).reshape(2, 2)
    tv = np.asarray(tipVector, dtype=np.float64).reshape(4, 2)
    if tip_case == INNER_INNER:
        a = np.asarray(x1).reshape(n, 4, 2)
    else:
        a = np.broadcast_to(tv[np.asarray(tipX1)][:, None, :], (n, 4, 2))
    if tip_case == TIP_TIP:
        b = np.broadcast_to(tv[np.asarray(tipX2)][:, None, :], (n, 4, 2))
    else:
        b = np.asarray(x2).reshape(n, 4, 2)
    x3 = np.zeros((n, 4, 2))
    for l in range(2):
        # mul, hadd, mul (the al/ar of the reference)
        al = a[:, :, 0] * L[None, :, l, 0] + a[:, :, 1] * L[None, :, l, 1]
        ar = b[:, :, 0] * R[None, :, l, 0] + b[:, :, 1] * R[None, :, l, 1]
        t = al * ar
        x3 = x3 + t[:, :, None] * ev[l][None, None, :]
    inc = 0
    if tip_case != TIP_TIP:
        scale = (np.abs(x3) < MINLIKELIHOOD).reshape(n, 8).all(axis=1)
        x3[scale] = x3[scale] * TWOTOTHE256
        inc = int(np.asarray(wgt, dtype=np.int64)[scale].sum())
    return np.ascontiguousarray(x3.reshape(n * 8)), inc


def site_terms(x1, x2, tipVector, tipX1, n, diag):
    """The per-site t[0] + t[1] of evaluateGTRGAMMA_BINARY."""
    d = np.asarray(diag, dtype=np.float64).reshape(4, 2)
    b = np.asarray(x2).reshape(n, 4, 2)
    if tipX1 is not None:
        tv = np.asarray(tipVector, dtype=np.float64).reshape(4, 2)
        a = np.broadcast_to(tv[np.asarray(tipX1)][:, None, :], (n, 4, 2))
    else:
        a = np.asarray(x1).reshape(n, 4, 2)
    termv = np.zeros((n, 2))
    for j in range(4):
        termv = termv + (a[:, j, :] * b[:, j, :]) * d[j][None, :]
    return termv[:, 0] + termv[:, 1]


def evaluate(wgt, x1, x2, tipVector, tipX1, n, diag):
    t = site_terms(x1, x2, tipVector, tipX1, n, diag)
    term = np.log(0.25 * np.abs(t))
    return float(math.fsum(np.asarray(wgt, dtype=np.float64) * term))


def sumtable(tip_case, x1, x2, tipVector, tipX1, tipX2, n):
    tv = np.asarray(tipVector, dtype=np.float64).reshape(4, 2)
    if tip_case == INNER_INNER:
        a = np.asarray(x1).reshape(n, 4, 2)
    else:
        a = np.broadcast_to(tv[np.asarray(tipX1)][:, None, :], (n, 4, 2))
    if tip_case == TIP_TIP:
        b = np.broadcast_to(tv[np.asarray(tipX2)][:, None, :], (n, 4, 2))
    else:
        b = np.asarray(x2).reshape(n, 4, 2)
    return np.ascontiguousarray((a * b).reshape(n * 8))


def core_dtables(EIGN, gammaRates, lz):
    """{d0[8], d1[8], d2[8]} through the product's host builder."""
    out = np.zeros(24)
    lib().examl_host_core_dtables_bin(
        _vp(np.ascontiguousarray(EIGN, dtype=np.float64)),
        _vp(np.ascontiguousarray(gammaRates, dtype=np.float64)),
        float(lz), _vp(out))
    return out


def core(n, sumtab, dtab, wgt):
    d0 = np.asarray(dtab[0:8]).reshape(4, 2)
    d1 = np.asarray(dtab[8:16]).reshape(4, 2)
    d2 = np.asarray(dtab[16:24]).reshape(4, 2)
    s = np.asarray(sumtab).reshape(n, 4, 2)
    a0 = np.zeros((n, 2))
    a1 = np.zeros((n, 2))
    a2 = np.zeros((n, 2))
    for j in range(4):
        tmp = d0[j][None, :] * s[:, j, :]
        a0 = a0 + tmp
        a1 = a1 + tmp * d1[j][None, :]
        a2 = a2 + tmp * d2[j][None, :]
    inv = 1.0 / np.abs(a0[:, 0] + a0[:, 1])
    dl = (a1[:, 0] + a1[:, 1]) * inv
    d2l = (a2[:, 0] + a2[:, 1]) * inv
    w = np.asarray(wgt, dtype=np.float64)
    return (float(math.fsum(w * dl)),
            float(math.fsum(w * (d2l - dl * dl))))


def make_p(qz, rz, model):
    """P block of one entry through the product's host makeP (states=2);
    qz/rz are raw branch lengths."""
    z1 = math.log(qz) if qz > ZMIN else math.log(ZMIN)
    z2 = math.log(rz) if rz > ZMIN else math.log(ZMIN)
    left = np.zeros(16)
    right = np.zeros(16)
    lib().examl_host_make_p(z1, z2, _vp(model.gammaRates), _vp(model.EI),
                            _vp(model.EIGN), 4, _vp(left), _vp(right), 2)
    return left, right


def diagptable(z, model):
    diag = np.zeros(8)
    lib().examl_host_calc_diagptable(float(z), 2, 4, _vp(model.gammaRates),
                                     _vp(model.EIGN), _vp(diag))
    return diag


class BinRefEngine:
    """CPU engine over the numpy kernels; same interface as
    tests.helpers.OracleEngine (and DnaGammaEngine's host-visible part)."""

    states = 2

    def __init__(self, tips, wgt, model):
        assert model.states == 2
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

    def upload_model(self):
        pass  # the kernels read the model arrays directly

    def newview_traversal(self, entries):
        m = self.model
        n = self.width
        for e in entries:
            left, right = make_p(e.qz, e.rz, m)
            if e.tipCase == TIP_TIP:
                x3, inc = newview(TIP_TIP, None, None, m.EV, m.tipVector,
                                  self.tips[e.x1Slot], self.tips[e.x2Slot],
                                  n, left, right, self.wgt)
            elif e.tipCase == TIP_INNER:
                x3, inc = newview(TIP_INNER, None, self.clv[e.x2Slot], m.EV,
                                  m.tipVector, self.tips[e.x1Slot], None, n,
                                  left, right, self.wgt)
            else:
                x3, inc = newview(INNER_INNER, self.clv[e.x1Slot],
                                  self.clv[e.x2Slot], m.EV, m.tipVector,
                                  None, None, n, left, right, self.wgt)
            self.clv[e.x3Slot] = x3
            self.scalers[e.pNumber] = (self.scalers[e.qNumber] +
                                       self.scalers[e.rNumber] + inc)

    def evaluate_root(self, tree, p, q, z, all_reduce=False):
        m = self.model
        diag = diagptable(z, m)
        if tree.is_tip(q):
            lnl = evaluate(self.wgt, None, self.clv[tree.clv_slot(p)],
                           m.tipVector, self.tips[q], self.width, diag)
        elif tree.is_tip(p):
            lnl = evaluate(self.wgt, None, self.clv[tree.clv_slot(q)],
                           m.tipVector, self.tips[p], self.width, diag)
        else:
            lnl = evaluate(self.wgt, self.clv[tree.clv_slot(p)],
                           self.clv[tree.clv_slot(q)], m.tipVector, None,
                           self.width, diag)
        lnl += float(self.scalers[p] + self.scalers[q]) * \
            math.log(MINLIKELIHOOD)
        return lnl

    def full_lnl(self, tree, root_edge=None):
        entries, (p, q, z) = tree.full_traversal(root_edge)
        self.newview_traversal(entries)
        return self.evaluate_root(tree, p, q, z)

    def sum_root(self, tree, p, q):
        m = self.model
        n = self.width
        p_tip, q_tip = tree.is_tip(p), tree.is_tip(q)
        if p_tip and q_tip:
            self.sumtable = sumtable(TIP_TIP, None, None, m.tipVector,
                                     self.tips[p], self.tips[q], n)
        elif q_tip:
            self.sumtable = sumtable(TIP_INNER, None,
                                     self.clv[tree.clv_slot(p)], m.tipVector,
                                     self.tips[q], None, n)
        elif p_tip:
            self.sumtable = sumtable(TIP_INNER, None,
                                     self.clv[tree.clv_slot(q)], m.tipVector,
                                     self.tips[p], None, n)
        else:
            self.sumtable = sumtable(INNER_INNER, self.clv[tree.clv_slot(p)],
                                     self.clv[tree.clv_slot(q)], m.tipVector,
                                     None, None, n)

    def core_derivs(self, lz, all_reduce=False):
        m = self.model
        return core(self.width, self.sumtable,
                    core_dtables(m.EIGN, m.gammaRates, lz), self.wgt)

    def core_derivs_async(self, lz):
        return self.core_derivs(lz)

    # topLevelMakenewz restated once, in the product engine: it only calls
    # sum_root and core_derivs
    makenewz = DnaGammaEngine.makenewz
