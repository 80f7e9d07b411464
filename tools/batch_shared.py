#!/usr/bin/env python3
"""What the shared batch (batch.SharedBatch, k_batch_solve_shared) delivers next to the resident batch
on the same data with the matrix values replicated per instance.  Writes profiles/batch_shared.json (or --out).  A report.

    batch_shared.py measure [--copies N] [--rounds R] [--baseline-lib PATH] [--out FILE]
        N instances (default 4096) of the boxed family of tests/batch_shared_cases.py on banded(256, 512, 6), random(144, 200, 7)
        and banded(100, 200, 4), settings OPTS of that file with warm_start off (every timed solve is the same cold solve).
        Baseline: `ResidentBatch` of the library at PATH (default: this tree's; pass the parent commit's build) with Px, Ax
        replicated N times, large=True where n > 128.  Per shape: an untimed solve of each side, then R rounds, the two sides
        alternated, a host clock around the blocking call with device outputs; median, minimum and maximum of each side, the
        instance-iterations per second, setup time and device bytes.

    batch_shared.py trace [--copies N]
        One shape (banded(256, 512, 6)), one warm-up and one solve of each side: what a kernel-trace run wraps.

    batch_shared.py nonregression LINES [--out FILE]
        LINES: `side<TAB>round<TAB>json line of bench.py --workload mpc-batch`, parent and change alternated; adds them with
        the verdict: packed_sha16 equal on every line, the times of the change inside the spread of the parent's."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_OUT = os.path.join(HERE, "profiles", "batch_shared.json")
SHAPES = [("banded", (256, 512, 6), 14), ("random", (144, 200, 7), 13), ("banded", (100, 200, 4), 12)]


def _paths():
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))


def _merge(path, key, value):
    rec = json.load(open(path)) if os.path.exists(path) else {}
    rec.setdefault("device", "MI355X")
    rec.setdefault("what", "the shared batch: one model, many right-hand sides on one KKT inverse (DESIGN.md section 13.3)")
    rec[key] = value
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def _sides(lib, base_lib, kind, shape, seed, copies):
    import numpy as np
    import scipy.sparse as sp

    from osqp_jl_amd import batch
    import batch_shared_cases as S

    opts = dict(S.OPTS, warm_start=False)
    base, q, l, u = S.boxed_spec(kind, shape, seed, 0, copies)
    P0, q0, A0, l0, u0 = base
    n, m = A0.shape[1], A0.shape[0]
    t0 = time.perf_counter()
    sb = batch.SharedBatch(lib, P0, A0, q0, l0, u0, copies, **opts)
    sb.update(q=q, l=l, u=u)
    t_shared = time.perf_counter() - t0
    Pu = sp.csc_matrix(sp.triu(P0)); Pu.sort_indices()
    Px, Ax = np.tile(Pu.data, (copies, 1)), np.tile(sp.csc_matrix(A0).data, (copies, 1))
    t0 = time.perf_counter()
    rb = batch.ResidentBatch(base_lib, P0, A0, Px, Ax, q, l, u, large=n > 128, **opts)
    t_resident = time.perf_counter() - t0
    resident_bytes = 8 * copies * (Pu.nnz + A0.nnz + n + 2 * m + (4 + 2 * n + 3 * m) + (n * n if n > 128 else 0))
    return sb, rb, dict(n=n, m=m, setup_s=dict(shared=round(t_shared, 4), resident=round(t_resident, 4)),
                        device_bytes=dict(shared=sb.device_bytes(), resident_data_records_scratch=resident_bytes),
                        plan=batch.shared_plan(lib, P0, A0))


def _timed(call):
    t = time.perf_counter()
    call()
    return (time.perf_counter() - t) * 1e3


def measure(a):
    _paths()
    import osqp_jl_amd as oq

    lib = oq.load_library()
    base_lib = oq.load_library(a.baseline_lib) if a.baseline_lib else lib
    out = {}
    for kind, shape, seed in SHAPES:
        name = "%s(%s)" % (kind, ", ".join(str(v) for v in shape))
        sb, rb, rec = _sides(lib, base_lib, kind, shape, seed, a.copies)
        so, ro = sb.alloc(), rb.alloc()
        sb.solve(out=so); rb.solve(out=ro)  # warm-up
        si, ri = so[2].numpy(), ro[2].numpy()
        ts, tr = [], []
        for _ in range(a.rounds):  # the two sides alternated
            tr.append(_timed(lambda: rb.solve(out=ro)))
            ts.append(_timed(lambda: sb.solve(out=so)))
        sb.close(); rb.close()
        iters = dict(shared=int(si[:, 0].sum()), resident=int(ri[:, 0].sum()))
        ms, mr = statistics.median(ts), statistics.median(tr)
        rec.update(
            instances=a.copies, rounds=a.rounds, solved=dict(shared=int((si[:, 1] == 1).sum()), resident=int((ri[:, 1] == 1).sum())),
            instance_iterations=iters, iteration_counts_equal=bool((si[:, 0] == ri[:, 0]).all()),
            ms_resolve=dict(shared=[round(t, 3) for t in ts], resident=[round(t, 3) for t in tr]),
            ms_resolve_median=dict(shared=round(ms, 3), resident=round(mr, 3)),
            ms_resolve_spread=dict(shared=round(max(ts) - min(ts), 3), resident=round(max(tr) - min(tr), 3)),
            instance_iterations_per_s=dict(shared=round(iters["shared"] / (ms * 1e-3), 1), resident=round(iters["resident"] / (mr * 1e-3), 1)),
            ns_per_instance_iteration=dict(shared=round(ms * 1e6 / iters["shared"], 2), resident=round(mr * 1e6 / iters["resident"], 2)),
            resident_over_shared=round(mr / ms, 3), shared_faster_by_more_than_the_baseline_spread=bool(mr - ms > max(tr) - min(tr)))
        out[name] = rec
        print(name, json.dumps(rec), flush=True)
    _merge(a.out, "shapes", out)
    _merge(a.out, "baseline_library", "the parent commit's build" if a.baseline_lib else "this tree's build (the resident path is the parent's code)")


def trace(a):
    _paths()
    import osqp_jl_amd as oq

    lib = oq.load_library()
    kind, shape, seed = SHAPES[0]
    sb, rb, _ = _sides(lib, lib, kind, shape, seed, a.copies)
    so, ro = sb.alloc(), rb.alloc()
    for _ in range(2):
        sb.solve(out=so); rb.solve(out=ro)
    sb.close(); rb.close()


def nonregression(a):
    lines = []
    for row in open(a.lines):
        row = row.rstrip("\n")
        if not row:
            continue
        side, rnd, js = row.split("\t", 2)
        rec = json.loads(js)
        lines.append(dict(side=side, round=int(rnd), ms_per_step=rec["ms_per_step"], value=rec["value"], unit=rec.get("unit"),
                          packed_sha16=rec.get("packed_sha16"), solved=rec.get("solved")))
    parent = [r["ms_per_step"] for r in lines if r["side"] == "parent"]
    change = [r["ms_per_step"] for r in lines if r["side"] == "change"]
    verdict = dict(sha_equal=len({r["packed_sha16"] for r in lines}) == 1, parent_ms=parent, change_ms=change,
                   change_inside_parent_spread=bool(parent and change and min(parent) <= min(change) and max(change) <= max(parent)),
                   change_not_slower_than_parent_max=bool(parent and change and max(change) <= max(parent)))
    _merge(a.out, "bench_mpc_batch", dict(
        command="bench.py --gpus 1 --steps 100 --warmup 25 --workload mpc-batch --no-cpu; the parent's library and this tree's "
                "alternated three times in one job, one process each", lines=lines, verdict=verdict))
    print(json.dumps(verdict))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    m = sub.add_parser("measure")
    m.add_argument("--copies", type=int, default=4096)
    m.add_argument("--rounds", type=int, default=5)
    m.add_argument("--baseline-lib", default=None)
    m.add_argument("--out", default=DEFAULT_OUT)
    t = sub.add_parser("trace")
    t.add_argument("--copies", type=int, default=4096)
    r = sub.add_parser("nonregression")
    r.add_argument("lines")
    r.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    {"measure": measure, "trace": trace, "nonregression": nonregression}[a.cmd](a)


if __name__ == "__main__":
    main()
