#!/usr/bin/env python3
"""Per-kernel table and product -> next-kernel census of a `rocprofv3 --kernel-trace --stats -f csv` run of bench.py
(profiles/spmv_fused_reduce.json: what follows every panel product on the device, and how long each takes).

    python tools/kernel_trace_census.py DIR_OR_CSV --iterations 125 [--out FILE.json]

DIR_OR_CSV: the *_kernel_trace.csv of the run, or a directory searched for one.  --iterations: what the per-step figures are
divided by -- ALL iterations of the traced run (bench.py: warm-up + steps), so the products and kernels of setup, which the trace
cannot tell from those of the steps, are spread over them; the per-step figures are upper bounds of the timed window's.

A kernel's name is the identifier in front of its template and call arguments, without namespaces (the anonymous one
included: its parentheses are not an argument list)."""
import argparse
import csv
import json
import os
import re
import sys

PRODUCTS = ("k_spmv_sell", "k_spmv_sell_fused", "k_spmv_sell_pair")


def short(name):
    s = name.replace("(anonymous namespace)::", "")
    s = re.sub(r"\s*\[clone[^\]]*\]|\.kd$", "", s)
    depth, cut = 0, len(s)
    for i, ch in enumerate(s):  # the first '<' or '(' outside any bracket ends the qualified name
        if ch in "<(" and depth == 0:
            cut = i
            break
    s = s[:cut].strip()
    s = s.split(" ")[-1]       # drop a return type ("void oq::k")
    return s.split("::")[-1] or name[:60]


def find_csv(path):
    if os.path.isfile(path):
        return path
    hits = []
    for d, _, files in os.walk(path):
        hits += [os.path.join(d, f) for f in files if f.endswith("kernel_trace.csv")]
    if len(hits) != 1:
        raise SystemExit("expected one *kernel_trace.csv under %s, found %d" % (path, len(hits)))
    return hits[0]


def census(path, iterations):
    with open(find_csv(path), newline="") as fh:
        rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])) for r in csv.DictReader(fh)]
    rows.sort()
    by = {}
    for st, en, k in rows:
        e = by.setdefault(k, [0, 0])
        e[0] += 1
        e[1] += en - st
    total = sum(e[1] for e in by.values()) or 1
    kernels = [dict(name=k, calls=n, total_ms=round(t / 1e6, 3), avg_us=round(t / n / 1e3, 3), ms_per_step=round(t / 1e6 / iterations, 4),
                    pct=round(100.0 * t / total, 2)) for k, (n, t) in sorted(by.items(), key=lambda kv: -kv[1][1])]
    products = {}
    for i, (st, en, k) in enumerate(rows):
        if k not in PRODUCTS:
            continue
        p = products.setdefault(k, dict(count=0, total_ns=0, next={}, gap_ns=0, next_ns={}))
        p["count"] += 1
        p["total_ns"] += en - st
        if i + 1 < len(rows):
            nst, nen, nk = rows[i + 1]
            p["next"][nk] = p["next"].get(nk, 0) + 1
            p["next_ns"][nk] = p["next_ns"].get(nk, 0) + (nen - nst)
            p["gap_ns"] += max(0, nst - en)
    out = {}
    for k, p in products.items():
        n = p["count"]
        out[k] = dict(count=n, per_step=round(n / iterations, 3), avg_us=round(p["total_ns"] / n / 1e3, 3),
                      ms_per_step=round(p["total_ns"] / 1e6 / iterations, 4), followed_by=dict(sorted(p["next"].items(), key=lambda kv: -kv[1])),
                      followed_by_reduce=p["next"].get("k_panel_reduce", 0), followed_by_row_sums=p["next"].get("k_panel_row_sums", 0),
                      next_avg_us={nk: round(t / p["next"][nk] / 1e3, 3) for nk, t in p["next_ns"].items()},
                      gap_to_next_avg_us=round(p["gap_ns"] / n / 1e3, 3))
    return dict(divided_by_iterations=iterations, dispatches=len(rows), kernel_ms_total=round(total / 1e6, 3), products=out, kernels=kernels)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("path")
    ap.add_argument("--iterations", type=int, required=True)
    ap.add_argument("--top", type=int, default=16, help="kernels kept in the table (by total time)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rec = census(a.path, a.iterations)
    rec["kernels"] = rec["kernels"][:a.top]
    text = json.dumps(rec, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    sys.stdout.write(text + "\n")
