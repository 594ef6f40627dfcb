#!/usr/bin/env python3
"""Step time of the DNA PSR (CAT) path: 50 taxa x 1,000,000 sites, 25 rate
categories, the bench tree.  One step is DnaCatEngine.full_lnl: a full
traversal (48 newview entries) plus the root evaluation.

  python tools/cat_step_time.py --steps K --warmup W --fused 0|1
                                [--partitions N] [--entries E] [--makenewz K]

--fused sets examl_hip_use_fused; on a build without the on-chip CAT kernel
it changes nothing on this path.  Inputs are seeded and generated here.
--partitions N splits the sites equally into N partitions with one category
set each; a step is then one traversal of all partitions (through
MultiDnaCatEngine where the build has it, else the loop over the engines)
plus the root evaluation of every partition and ONE synchronise.  --entries
E times a partial traversal instead: the last E entries of the list, after
one full traversal.  --makenewz K (with partitions) times a branch-length
step instead: sum_root of all partitions plus K core evaluations, each read
back to the host as the Newton-Raphson loop of TreeSearch.makenewz_generic
does.  Evaluate, sum and core go through MultiDnaCatEngine where the build
has them there (root_ops in the output), else through the loop over the
engines.  With partitions, host_p_ms is the executor's own host
timer around the make_p loop of the last step
(examl_hip_multi_cat_host_p_ms; null on a build without it) and upload_ms
the time of one pinned copy of one step's P bytes, made and synchronised
here.
--rate-opt times the per-site rate search of optimize_rate_categories alone
(no categorisation, none of the full evaluations around it), from all rates
1.0 at the first round's spacing: --rate-kernel 1 the GPU kernel (host clock
around upload, launch and readback, plus HIP events around the rate
upload and the launch;
--rate-lds B passes an LDS budget in bytes, 0 = global slots), --rate-kernel
0 the host loop.  rate_digest sums the chosen rates for comparing the two.
--protein (with --rate-opt) scans an amino-acid alignment under WAG (from
examl_amd/data/aa_models.npz) with a ProtCatEngine instead.  --protein alone
times ProtCatEngine.full_lnl on such an alignment, as the DNA step above,
and reports examl_hip_prot_cat_fused_launches.  --protein --gamma times
DnaGammaEngine.full_lnl under WAG+GAMMA (4 rates, no categories) instead and
reports examl_hip_prot_gamma_fused_launches.  --protein --gamma --partitions
N splits the sites equally into N partitions with an empirical model and
alpha each and times MultiEngine (one traversal of all partitions plus the
root evaluation); --fused then sets examl_hip_multi_use_fused, and
on_chip_launches is MultiEngine.prot_fused_launches.
Prints ONE JSON line; lnl is printed with repr() precision so two builds
can be compared digit for digit.  The time is a host clock around K steps
that end in a device synchronise.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import examl_amd as ea  # noqa: E402
from examl_amd.synthetic import make_alignment, make_alignment_aa  # noqa: E402

# traffic model of DESIGN §7g, bytes per site: II 32+32 in, 32 out, 4 cptr
ENTRY_BYTES = {ea.TIP_TIP: 38, ea.TIP_INNER: 69, ea.INNER_INNER: 100}


def upload_ms(engs, entries):
    """ms of one pinned, synchronised copy of one step's P blocks."""
    src = torch.empty(len(entries) * sum(e.num_cats for e in engs) * 32,
                      dtype=torch.float64).pin_memory()
    dst = torch.empty_like(src, device="cuda:0")
    dst.copy_(src, non_blocking=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        dst.copy_(src, non_blocking=True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e2


def partitioned(args):
    assert torch.cuda.is_available(), "cat_step_time needs a GPU"
    L = ea.lib()
    NP = args.partitions
    tips, wgt = make_alignment(args.taxa, args.sites, seed=42)
    tree = ea.PhyloTree.random(args.taxa, seed=7)
    entries, (p, q, z) = tree.full_traversal()
    cut = np.linspace(0, args.sites, NP + 1).astype(int)
    engs = []
    for i in range(NP):
        w = int(cut[i + 1] - cut[i])
        rng = np.random.default_rng(100 + i)
        freqs = rng.uniform(0.2, 0.3, 4)
        model = ea.DnaGtrModel(list(freqs / freqs.sum()),
                               list(rng.uniform(0.5, 3.0, 5)) + [1.0],
                               alpha=0.6)
        cptr = (np.arange(w) % args.cats).astype(np.int32)
        rng.shuffle(cptr)
        engs.append(ea.DnaCatEngine(
            np.ascontiguousarray(tips[:, cut[i]:cut[i + 1]]),
            wgt[cut[i]:cut[i + 1]], model, cptr,
            np.linspace(0.05, 4.0, args.cats) * (1 + 0.01 * i),
            device="cuda:0"))
    cls = getattr(ea, "MultiDnaCatEngine", None)
    multi = cls(engs) if cls else None
    timed = entries[-args.entries:] if args.entries else entries

    def traverse(lst):
        if multi is not None:
            multi.newview_traversal(lst)
        else:
            for e in engs:
                e.newview_traversal(lst)

    root_ops = hasattr(multi, "core_derivs_vec")
    lzs = np.log(np.linspace(0.2, 0.9, max(args.makenewz, 1)))

    def evaluate():
        if root_ops:
            return [multi.evaluate_root(tree, p, q, z)]
        return [e.evaluate_root(tree, p, q, z) for e in engs]

    def makenewz():
        if root_ops:
            multi.sum_root(tree, p, q)
        else:
            for e in engs:
                e.sum_root(tree, p, q)
        for lz in lzs:
            if root_ops:
                vals = multi.core_derivs_vec(float(lz)).cpu()
            else:
                vals = torch.stack([e.core_derivs_async(float(lz))
                                    for e in engs]).cpu()
            d1, d2 = float(vals[:, 0].sum()), float(vals[:, 1].sum())
        return d1, d2

    def step():
        if args.makenewz:
            return makenewz()
        traverse(timed)
        return evaluate()

    L.examl_hip_use_fused(args.fused)
    try:
        traverse(entries)
        for _ in range(args.warmup):
            outs = step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            outs = step()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
    finally:
        L.examl_hip_use_fused(1)
    launches = multi.fused_launches() if multi is not None else 0
    timer = getattr(L, "examl_hip_multi_cat_host_p_ms", None)
    make_ms = timer(multi.h) if timer and multi is not None else None
    up_ms = upload_ms(engs, timed)
    print(json.dumps({
        "metric": "partitioned DNA PSR step time",
        "ms_per_step": elapsed / args.steps * 1e3,
        "steps": args.steps,
        "warmup": args.warmup,
        "fused": args.fused,
        "multi_engine": multi is not None,
        "on_chip_launches": launches,
        "taxa": args.taxa,
        "sites": args.sites,
        "partitions": NP,
        "cats": args.cats,
        "entries": len(timed),
        "host_p_ms": make_ms,
        "upload_ms": up_ms,
        "root_ops": root_ops,
        "makenewz": args.makenewz,
        "lnl": repr(float(sum(float(v) for o in evaluate()
                              for v in o.cpu().reshape(-1)))),
        "derivs": [repr(x) for x in outs] if args.makenewz else None,
    }), flush=True)


def wag_model():
    aa = np.load(os.path.join(os.path.dirname(ea.__file__), "data",
                              "aa_models.npz"))
    return ea.ProtGtrModel(aa["frequencies"][4], aa["rates190"][4], 1.0)


def partitioned_prot_gamma(args):
    """--protein --gamma --partitions N: MultiEngine over N equal 20-state
    GAMMA partitions with models of their own; a step is one traversal of
    all partitions plus the root evaluation.  --fused sets
    examl_hip_multi_use_fused."""
    assert torch.cuda.is_available(), "cat_step_time needs a GPU"
    L = ea.lib()
    NP = args.partitions
    tips, wgt = make_alignment_aa(args.taxa, args.sites, seed=42)
    tree = ea.PhyloTree.random(args.taxa, seed=7)
    entries, (p, q, z) = tree.full_traversal()
    aa = np.load(os.path.join(os.path.dirname(ea.__file__), "data",
                              "aa_models.npz"))
    cut = np.linspace(0, args.sites, NP + 1).astype(int)
    engs = [ea.DnaGammaEngine(
        np.ascontiguousarray(tips[:, cut[i]:cut[i + 1]]),
        wgt[cut[i]:cut[i + 1]],
        ea.ProtGtrModel(aa["frequencies"][4 + i % 3], aa["rates190"][4 + i % 3],
                        0.5 + 0.05 * i), device="cuda:0") for i in range(NP)]
    multi = ea.MultiEngine(engs)

    def step():
        multi.newview_traversal(entries)
        return multi.evaluate_root(tree, p, q, z)

    L.examl_hip_multi_use_fused(args.fused)
    try:
        for _ in range(args.warmup):
            lnl = step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            lnl = step()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
    finally:
        L.examl_hip_multi_use_fused(1)
    # a build from before the on-chip kernel has no such counter
    count = getattr(multi, "prot_fused_launches", None)
    print(json.dumps({
        "metric": "partitioned protein GAMMA step time",
        "ms_per_step": elapsed / args.steps * 1e3, "steps": args.steps,
        "warmup": args.warmup, "fused": args.fused,
        "on_chip_launches": count() if count else 0, "taxa": args.taxa,
        "sites": args.sites, "partitions": NP, "entries": len(entries),
        "lnl": repr(float(lnl.sum().item())),
    }), flush=True)


def rate_opt(args):
    assert torch.cuda.is_available(), "cat_step_time needs a GPU"
    from examl_amd.search import TreeSearch
    if args.protein:
        tips, wgt = make_alignment_aa(args.taxa, args.sites, seed=42)
        model = wag_model()
        cls = ea.ProtCatEngine
    else:
        tips, wgt = make_alignment(args.taxa, args.sites, seed=42)
        model = ea.DnaGtrModel([0.28, 0.22, 0.24, 0.26],
                               [1.2, 2.9, 0.7, 1.0, 3.2, 1.0], alpha=0.6)
        cls = ea.DnaCatEngine
    tree = ea.PhyloTree.random(args.taxa, seed=7, rng_z=True)
    eng = cls(tips, wgt, model, np.zeros(args.sites, dtype=np.int32),
              np.array([1.0]), device="cuda:0")
    ts = TreeSearch(tree, [eng], rate_het="CAT")
    ts.evaluate_generic(full=True)
    entries, p, q, zv = ts._last_full
    ms, ev_ms = [], []
    for it in range(args.warmup + args.steps):
        ts.cat_patrat[0][:] = 1.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if args.rate_kernel:
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in "01")
            e0.record()
            res = eng.rate_scan_launch(entries, p, q, float(zv[0]),
                                       ts.cat_patrat[0], 0.5, 1.0,
                                       lds_budget=args.rate_lds)
            e1.record()
            ts.cat_patrat[0][:], ts.cat_lhs[0][:] = \
                (r.cpu().numpy() for r in res)
            e1.synchronize()
            ev_ms.append(e0.elapsed_time(e1))
        else:
            ts._rate_scan_host(0, 0.5, 1.0)
        ms.append((time.perf_counter() - t0) * 1e3)
    ms, ev_ms = ms[args.warmup:], ev_ms[args.warmup:]
    print(json.dumps({
        "metric": ("protein" if args.protein else "DNA")
        + " PSR per-site rate scan",
        "rate_kernel": args.rate_kernel,
        "ms_median": float(np.median(ms)), "ms_min": min(ms),
        "ms_max": max(ms),
        "launch_ms_median": float(np.median(ev_ms)) if ev_ms else None,
        "launch_ms_min": min(ev_ms) if ev_ms else None,
        "launch_ms_max": max(ev_ms) if ev_ms else None,
        "slot_home": (ea.lib().examl_hip_rate_scan_slot_home()
                      if args.rate_kernel else None),
        "steps": args.steps, "warmup": args.warmup, "taxa": args.taxa,
        "sites": args.sites,
        "rate_digest": repr(float(ts.cat_patrat[0].sum())),
        "lhs_sum": repr(float(ts.cat_lhs[0].sum())),
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--fused", type=int, choices=(0, 1), default=1)
    ap.add_argument("--sites", type=int, default=1_000_000)
    ap.add_argument("--taxa", type=int, default=50)
    ap.add_argument("--cats", type=int, default=25)
    ap.add_argument("--partitions", type=int, default=1)
    ap.add_argument("--entries", type=int, default=0)
    ap.add_argument("--makenewz", type=int, default=0)
    ap.add_argument("--rate-opt", action="store_true")
    ap.add_argument("--rate-kernel", type=int, choices=(0, 1), default=1)
    ap.add_argument("--rate-lds", type=int, default=-1)
    ap.add_argument("--protein", action="store_true")
    ap.add_argument("--gamma", action="store_true")
    args = ap.parse_args()
    assert args.protein or not args.gamma, "--gamma goes with --protein"
    if args.rate_opt:
        return rate_opt(args)
    if args.partitions > 1 and args.protein and args.gamma:
        return partitioned_prot_gamma(args)
    if args.partitions > 1:
        return partitioned(args)

    assert torch.cuda.is_available(), "cat_step_time needs a GPU"
    L = ea.lib()
    if args.protein and args.gamma:
        tips, wgt = make_alignment_aa(args.taxa, args.sites, seed=42)
        model, cls = wag_model(), ea.DnaGammaEngine
        counter = "examl_hip_prot_gamma_fused_launches"
    elif args.protein:
        tips, wgt = make_alignment_aa(args.taxa, args.sites, seed=42)
        model, cls = wag_model(), ea.ProtCatEngine
        counter = "examl_hip_prot_cat_fused_launches"
    else:
        tips, wgt = make_alignment(args.taxa, args.sites, seed=42)
        model = ea.DnaGtrModel([0.28, 0.22, 0.24, 0.26],
                               [1.2, 2.9, 0.7, 1.0, 3.2, 1.0], alpha=0.6)
        cls, counter = ea.DnaCatEngine, "examl_hip_cat_fused_launches"
    rates = np.linspace(0.05, 4.0, args.cats)
    cptr = (np.arange(args.sites) % args.cats).astype(np.int32)
    np.random.default_rng(1).shuffle(cptr)
    tree = ea.PhyloTree.random(args.taxa, seed=7)
    entries, _ = tree.full_traversal()
    if args.gamma:
        eng = cls(tips, wgt, model, device="cuda:0")
    else:
        eng = cls(tips, wgt, model, cptr, rates, device="cuda:0")

    L.examl_hip_use_fused(args.fused)
    try:
        for _ in range(args.warmup):
            lnl = eng.full_lnl(tree)
        eng.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            lnl = eng.full_lnl(tree)
        eng.sync()
        elapsed = time.perf_counter() - t0
    finally:
        L.examl_hip_use_fused(1)

    # a build from before the on-chip CAT kernel has no launch counter
    count = getattr(L, counter, None)
    launches = count() if count else 0
    ms = elapsed / args.steps * 1e3
    if args.protein:
        print(json.dumps({
            "metric": "protein %s full_lnl step time"
                      % ("GAMMA" if args.gamma else "PSR"),
            "ms_per_step": ms, "steps": args.steps, "warmup": args.warmup,
            "fused": args.fused, "on_chip_launches": launches,
            "taxa": args.taxa, "sites": args.sites, "cats": args.cats,
            "entries": len(entries), "lnl": repr(float(lnl.item())),
        }), flush=True)
        return
    per_entry = sum(ENTRY_BYTES[e.tipCase] for e in entries)
    ntip_reads = sum((e.tipCase != ea.INNER_INNER) + (e.tipCase == ea.TIP_TIP)
                     for e in entries)
    on_chip = 32 * len(entries) + ntip_reads + 4
    model_bytes = (on_chip if launches else per_entry) * args.sites
    print(json.dumps({
        "metric": "DNA PSR full_lnl step time",
        "ms_per_step": ms,
        "steps": args.steps,
        "warmup": args.warmup,
        "fused": args.fused,
        "on_chip_launches": launches,
        "taxa": args.taxa,
        "sites": args.sites,
        "cats": args.cats,
        "entries": len(entries),
        "model_bytes_per_site": {"per_entry": per_entry, "on_chip": on_chip},
        "model_tb_per_s": model_bytes / (ms * 1e-3) / 1e12,
        "lnl": repr(float(lnl.item())),
    }), flush=True)


if __name__ == "__main__":
    main()
