"""Planner cases for tools/fused_plan_check.cpp, on stdout: the trees of
tests/test_fused_traversal.py (bench tree, 200 random 50-taxon trees, a
caterpillar, shallow stacks, a long list, a partial root path, lists out of
stack order and a malformed one)."""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import examl_amd as ea  # noqa: E402

TIP_TIP, TIP_INNER, INNER_INNER = ea.TIP_TIP, ea.TIP_INNER, ea.INNER_INNER


def root_path(tree):
    entries, _ = tree.full_traversal()
    parent = {}
    for e in entries:
        parent[e.qNumber] = parent[e.rNumber] = e.pNumber
    v = next(e for e in entries if e.tipCase == TIP_TIP).pNumber
    chain = set()
    while v in parent:
        v = parent[v]
        chain.add(v)
    return [e for e in entries if e.pNumber in chain]


def main():
    cases = []
    bench = ea.PhyloTree.random(50, seed=7).full_traversal()[0]
    for depth in (1, 2, 3, 4, 16):
        cases.append((bench, depth))
    for seed in range(200):
        cases.append((ea.PhyloTree.random(50, seed=1000 + seed)
                      .full_traversal()[0], 4))
    cases.append((ea.PhyloTree.caterpillar(50).full_traversal()[0], 4))
    cases.append((ea.PhyloTree.caterpillar(500).full_traversal()[0], 4))
    cases.append((ea.PhyloTree.random(1000, seed=3).full_traversal()[0], 4))
    cases.append((root_path(ea.PhyloTree.random(12, seed=5)), 4))
    swapped = ea.PhyloTree.random(50, seed=7).full_traversal()[0]
    e = next(x for x in swapped if x.tipCase == INNER_INNER)
    e.x1Slot, e.x2Slot = e.x2Slot, e.x1Slot
    cases.append((swapped, 4))
    cases.append((list(reversed(bench)), 4))
    bad = ea.PhyloTree.random(6, seed=1).full_traversal()[0]
    bad[1].tipCase = 7
    cases.append((bad, 4))
    cases.append(([], 4))
    print(len(cases))
    for entries, depth in cases:
        print(len(entries), depth)
        for e in entries:
            print(e.tipCase, e.pNumber, e.qNumber, e.rNumber, e.x1Slot,
                  e.x2Slot, e.x3Slot)


if __name__ == "__main__":
    main()
