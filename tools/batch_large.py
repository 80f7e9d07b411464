#!/usr/bin/env python3
"""What the opt-in batched path for 128 < n <= 256 (osqp_amd_batch_large, k_batch_solve_large) delivers,
next to the CPU oracle on the same instances.  Writes profiles/batch_large.json (or --out).  A report, not a gate.

    batch_large.py measure [--copies N] [--rounds R] [--cpu-seconds S] [--out FILE]
        N instances (default 4096) each of random(144, 200, 7) and banded(256, 512, 6) -- the builders and `instances` of
        tests/batch_entry_families.py with that file's OPTS (seed 4000 + the shape's position) -- on one resident handle built
        with large=True, cold starts (warm_start off, the rho of every record put back before a solve): an untimed solve,
        then R timed ones, a host clock around the blocking call with device outputs.  Per shape: ms per launch, instance-
        iterations per second, bytes of the inverse read per iteration (8 n^2 per instance) and per launch, the plan of the
        kernel; and the oracle's QPs/s (setup + solve) on the first instances of the same batch, one process per core on 16
        cores, for S seconds -- the form of BASELINE.md for mpc-batch.

    batch_large.py nonregression LINES [--out FILE]
        LINES: a file of `side<TAB>round<TAB>json line of bench.py --workload mpc-batch` rows, parent and change alternated.
        Adds them to the profile with the verdict: packed_sha16 equal on every line, and every time of the change inside the
        spread of the parent's times."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_OUT = os.path.join(HERE, "profiles", "batch_large.json")
SHAPES = [("random", (144, 200, 7)), ("banded", (256, 512, 6))]
CORES = 16


def _paths():
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))


def _merge(path, key, value):
    rec = json.load(open(path)) if os.path.exists(path) else {}
    rec.setdefault("device", "MI355X")
    rec.setdefault("what", "the opt-in batched path for 128 < n <= 256 (DESIGN.md section 13.1)")
    rec[key] = value
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def _cpu_worker(task):
    """One host core: setup + solve of instances first, first + stride, ... of the first `have` of the batch, until the deadline."""
    kind, args, seed, have, first, stride, seconds = task
    _paths()
    import osqp_jl_amd as oq
    import batch_entry_families as F

    ora = oq.load_library(oq.ORACLE_LIB_PATH)
    _, probs = F.instances(F.BUILDERS[kind](*args), have, seed)  # the generator draws instance by instance: the first `have` of the batch
    t0 = time.perf_counter()
    k, its, i = 0, 0, first
    while time.perf_counter() - t0 < seconds:
        its += F.oracle_solve(ora, probs[i % have], **F.OPTS).info.iter
        k += 1
        i += stride
    return k, its, time.perf_counter() - t0


def measure(a):
    _paths()
    import multiprocessing as mp
    import subprocess

    import numpy as np

    import osqp_jl_amd as oq
    from osqp_jl_amd import batch
    import batch_entry_families as F

    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "oracle")])
    lib = oq.load_library()
    out = {}
    for pos, (kind, args) in enumerate(SHAPES):
        seed = 4000 + pos
        name = "%s(%s)" % (kind, ", ".join(str(v) for v in args))
        # the CPU leg first, in fresh processes that never open the device
        have = 4 * CORES
        with mp.get_context("spawn").Pool(CORES) as pool:
            res = pool.map(_cpu_worker, [(kind, args, seed, have, r, CORES, a.cpu_seconds) for r in range(CORES)])
        kk, ii, tmax = sum(r[0] for r in res), sum(r[1] for r in res), max(r[2] for r in res)
        cpu = dict(cores=CORES, qps_per_s=round(kk / tmax, 1), iterations_per_s=round(ii / tmax, 1),
                   sample=f"{kk} solves (setup + solve) of the first {have} instances over {CORES} processes in {tmax:.1f} s")
        pat = F.BUILDERS[kind](*args)
        t0 = time.perf_counter()
        (P, A, Px, Ax, q, l, u), _ = F.instances(pat, a.copies, seed)
        gen_s = time.perf_counter() - t0
        plan = batch.large_plan(lib, P, A)
        rb = batch.ResidentBatch(lib, P, A, Px, Ax, q, l, u, large=True, **dict(F.OPTS, warm_start=False))
        dev = rb.alloc()
        rho = F.OPTS.get("rho", 0.1)

        def run():
            rb.update_settings(rho=rho)  # every record back to the first rho: each timed solve is the same cold solve
            t = time.perf_counter()
            rb.solve(out=dev)
            return (time.perf_counter() - t) * 1e3

        run()
        info = dev[2].numpy()
        sched = batch.last_schedule(lib)
        times = [run() for _ in range(a.rounds)]
        rb.close()
        n = args[0]
        iters = int(info[:, 0].sum())
        ms = statistics.median(times)
        out[name] = dict(
            n=n, m=args[1], instances=a.copies, seed=seed, kernel=sched["entry"], lds_bytes=sched["lds_bytes"], plan=plan,
            solved=int((info[:, 1] == 1).sum()), instance_iterations=iters, mean_iterations=round(iters / a.copies, 2),
            rho_updates=int(info[:, 5].sum()), ms_per_launch=[round(t, 3) for t in times], ms_per_launch_median=round(ms, 3),
            qps_per_s=round(a.copies / (ms * 1e-3), 1), instance_iterations_per_s=round(iters / (ms * 1e-3), 1),
            inverse_bytes_per_iteration_per_instance=8 * n * n, inverse_bytes_per_iteration_all_workgroups=8 * n * n * 256,
            inverse_bytes_per_launch=8 * n * n * iters, inverse_read_gb_per_s=round(8 * n * n * iters / (ms * 1e-3) / 1e9, 1),
            host_seconds_to_generate_the_instances=round(gen_s, 1), cpu_oracle=cpu,
            gpu_over_cpu_16_cores=round((a.copies / (ms * 1e-3)) / (kk / tmax), 2))
        print(name, json.dumps(out[name]))
    _merge(a.out, "shapes", out)
    _merge(a.out, "settings", dict(F.OPTS, warm_start=False, copies=a.copies, rounds=a.rounds))


def nonregression(a):
    lines = []
    for row in open(a.lines):
        row = row.rstrip("\n")
        if not row:
            continue
        side, rnd, js = row.split("\t", 2)
        rec = json.loads(js)
        lines.append(dict(side=side, round=int(rnd), ms_per_step=rec["ms_per_step"], value=rec["value"], unit=rec.get("unit"),
                          instances_per_s=rec.get("instances_per_s"), packed_sha16=rec.get("packed_sha16"), solved=rec.get("solved")))
    parent = [r["ms_per_step"] for r in lines if r["side"] == "parent"]
    change = [r["ms_per_step"] for r in lines if r["side"] == "change"]
    verdict = dict(sha_equal=len({r["packed_sha16"] for r in lines}) == 1, parent_ms=parent, change_ms=change,
                   change_inside_parent_spread=bool(parent and change and min(parent) <= min(change) and max(change) <= max(parent)),
                   change_not_slower_than_parent_max=bool(parent and change and max(change) <= max(parent)))
    _merge(a.out, "bench_mpc_batch", dict(
        command="bench.py --gpus 1 --steps 100 --warmup 25 --workload mpc-batch --no-cpu; the parent's batch kernels linked into a "
                "library of their own and this tree alternated three times in one job, one process each; the switch is off",
        lines=lines, verdict=verdict))
    print(json.dumps(verdict))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    m = sub.add_parser("measure")
    m.add_argument("--copies", type=int, default=4096)
    m.add_argument("--rounds", type=int, default=5)
    m.add_argument("--cpu-seconds", type=float, default=8.0)
    m.add_argument("--out", default=DEFAULT_OUT)
    r = sub.add_parser("nonregression")
    r.add_argument("lines")
    r.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    {"measure": measure, "nonregression": nonregression}[a.cmd](a)


if __name__ == "__main__":
    main()
