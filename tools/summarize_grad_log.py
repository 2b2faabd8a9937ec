#!/usr/bin/env python3
"""Worst per-column gradient errors of a backward test run (tests/helpers.py writes one JSON line per comparison when
LEAF_GRAD_LOG is set):

    LEAF_GRAD_LOG=gpurun_out/r06/grad_log.jsonl python -m pytest tests/test_gpu_backward.py -m gpu -q
    python tools/summarize_grad_log.py gpurun_out/r06/grad_log.jsonl > profiles/r06/backward_column_errors.txt

`of column max` = max |g - r| / max |r_col| (bound 1e-4); `of entry bound` = max |g - r| / (1e-3 |r_f| + 1e-6 max |r_col|) (bound 1).

    python tools/summarize_grad_log.py --by-family grad_log.jsonl > profiles/backward_edges.txt

groups the comparisons of tests/test_gpu_backward_edges.py by the `family=` of their context instead: per family the worst figure of
each kind with its column and the clip length T it occurred at, and every comparison past a bound.  `*` marks a column judged with the
floor of tiny clips (scale max(max |r_col|, 1e-3 max |r_col at T = h + 1|))."""
import collections
import json
import re
import sys

args = [a for a in sys.argv[1:] if not a.startswith("--")]
rows = [json.loads(l) for l in open(args[0])]

if "--by-family" in sys.argv:
    fam = collections.defaultdict(list)
    for r in rows:
        m = re.search(r"family=(\S+) T=(\d+)", r["ctx"])
        if m:
            fam[m.group(1)].append((r, int(m.group(2))))
    mark = lambda r: "*" if r.get("floored") else ""
    print(f"{sum(len(v) for v in fam.values())} gradient-column comparisons against fp64 autograd through the oracle (tests/test_gpu_backward_edges.py)")
    print(f"{'family':40s} {'n':>5s} {'lengths':>7s} {'of column max':>14s} {'at T':>7s}  {'column':34s} {'of entry bound':>15s} {'at T':>7s}  column")
    missed = []
    for name, items in sorted(fam.items()):
        wa = max(items, key=lambda it: it[0]["rel_to_col_max"])
        wb = max(items, key=lambda it: it[0]["entry_bound_used"] or 0.0)
        print(f"{name:40s} {len(items):5d} {len({t for _, t in items}):7d} {wa[0]['rel_to_col_max']:14.2e} {wa[1]:7d}  "
              f"{wa[0]['column'] + mark(wa[0]):34s} {wb[0]['entry_bound_used'] or 0.0:15.3f} {wb[1]:7d}  {wb[0]['column'] + mark(wb[0])}")
        missed += [(name, t, r) for r, t in items if r["rel_to_col_max"] >= 1e-4 or (r["entry_bound_used"] or 0.0) >= 1.0]
    print(f"\n{len(missed)} comparisons past a bound (1e-4 of the column's scale; 1.0 of the entry bound):")
    for name, t, r in missed:
        print(f"{name:40s} T={t:<6d} {r['column'] + mark(r):34s} {r['rel_to_col_max']:10.2e} {r['entry_bound_used'] or 0.0:8.2f}   {r['ctx']}")
    sys.exit(0)

worst = collections.defaultdict(lambda: [0.0, 0.0, None, None, 0])
for r in rows:
    w = worst[r["column"]]
    w[4] += 1
    if r["rel_to_col_max"] > w[0]:
        w[0], w[2] = r["rel_to_col_max"], r["ctx"]
    if r["entry_bound_used"] is not None and r["entry_bound_used"] > w[1]:
        w[1], w[3] = r["entry_bound_used"], r["ctx"]
print(f"{len(rows)} gradient-column comparisons against fp64 autograd through the oracle (tests/test_gpu_backward.py)")
print(f"{'column':34s} {'n':>5s} {'of column max':>14s} {'of entry bound':>15s}   worst cases")
for c, w in sorted(worst.items()):
    print(f"{c:34s} {w[4]:5d} {w[0]:14.2e} {w[1]:15.3f}   {w[2]} | {w[3]}")
