#!/usr/bin/env python3
"""What polish, adjoint and JVP cost on resident handles with 128 < n <= 256 (osqp_amd_batch_large_factor: the factor in the
instance's global scratch).  Writes profiles/batch_large_factor.json (or --out).  A report, not a gate:
the parent of the change could not run any of these launches, so there is no ratio to hold.

    batch_large_factor.py measure [--copies N] [--rounds R] [--cpu-seconds S] [--out FILE]   (S = 0: without the CPU leg)
        N instances (default 4096) each of random(144, 200, 7) and banded(256, 512, 6) -- the builders and `instances` of
        tests/batch_entry_families.py with that file's OPTS (seed 4000 + the shape's position, as tools/batch_large.py) -- on
        one resident handle built with large=True, large_factor=True; a host clock around the blocking call, device pointers
        in and out, an untimed call and then R timed ones of each:
          the solve launch       cold (warm_start off, the rho of every record put back), polish = 0;
          the polish launch      the same cold resolve with polish = 1, minus the solve launch (the library has no timer per
                                 launch; both resolves run the same ADMM work);
          adjoint                dq, dl, du from (dx, dy), ncot = 1 and 8;
          jvp                    tx, ty along (tq, tl, tu), ndir = 1 and 8;
        beside them the CPU oracle's polish_time, summed over solves of the first instances of the same batch with
        polish = 1, one process per core on 16 cores for S seconds (instances polished per second of wall time, and the mean
        polish_time of one instance), and -- as a neighbour -- the polish launch of the LDS form on N instances of
        banded(128, 192, 4) measured the same way.

    batch_large_factor.py controls LINES [--out FILE]
        LINES: a file of `control<TAB>side<TAB>round<TAB>json line` rows, parent and change alternated three times in one job:
          bench     a line of `bench.py --gpus 1 --workload mpc-batch --no-cpu`: packed_sha16 equal on all lines and the times of
                    the change inside the parent's spread;
          adjoint   a line of `tools/batch_closed_loop.py --adjoint` (the resolve, the resolve + polish launch, the adjoint);
          jvp       a line of `tools/batch_closed_loop.py --jvp` (the calls behind profiles/batch_jvp.json);
        on 4096 MPC QPs.  The parent's side is the parent's libosqp_amd.so named by OSQP_AMD_LIB.  Adds the lines with the
        verdict per timed figure: the change's median inside [min, max] of the parent's."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_OUT = os.path.join(HERE, "profiles", "batch_large_factor.json")
SHAPES = [("random", (144, 200, 7)), ("banded", (256, 512, 6))]
NEIGHBOUR = ("banded", (128, 192, 4))
CORES = 16
MANY = 8


def _paths():
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))


def _merge(path, key, value):
    rec = json.load(open(path)) if os.path.exists(path) else {}
    rec.setdefault("device", "MI355X")
    rec.setdefault("what", "polish, adjoint and JVP on resident handles with 128 < n <= 256, the factor in global scratch (DESIGN.md section 13.2)")
    rec[key] = value
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def _cpu_worker(task):
    """One host core: setup + polished solve of instances first, first + stride, ... of the first `have`, until the deadline."""
    kind, args, seed, have, first, stride, seconds = task
    _paths()
    import osqp_jl_amd as oq
    import batch_entry_families as F

    ora = oq.load_library(oq.ORACLE_LIB_PATH)
    _, probs = F.instances(F.BUILDERS[kind](*args), have, seed)
    t0 = time.perf_counter()
    k, accepted, polish_s, i = 0, 0, 0.0, first
    while time.perf_counter() - t0 < seconds:
        r = F.oracle_solve(ora, probs[i % have], **dict(F.OPTS, polish=True))
        polish_s += r.info.polish_time
        accepted += int(r.info.status_polish == 1)
        k += 1
        i += stride
    return k, accepted, polish_s, time.perf_counter() - t0


class _View:
    """A [lead x k x cols] view of a DeviceArray of lead * k rows, as `ResidentBatch.adjoint` / `jvp` take it by address."""

    def __init__(self, arr, lead):
        self.arr, self.shape = arr, (lead, arr.shape[0] // lead, arr.shape[1])

    def data_ptr(self):
        return self.arr.data_ptr()


def _timed(fn, rounds):
    fn()
    out = []
    for _ in range(rounds):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def _stats(times):
    return dict(ms=[round(t, 3) for t in times], ms_median=round(statistics.median(times), 3), ms_min=round(min(times), 3))


def _resolves(rb, rounds, rho):
    """(ms of the cold polish = 0 resolve, ms of the cold polish = 1 resolve, accepted polishes), alternated round by round."""
    import numpy as np

    dev = rb.alloc()

    def run(polish):
        rb.update_polish(polish)
        rb.update_settings(rho=rho)  # every record back to the first rho: each timed solve is the same cold solve
        t = time.perf_counter()
        rb.solve(out=dev)
        return (time.perf_counter() - t) * 1e3

    run(0); run(1)
    plain, polished = [], []
    for _ in range(rounds):
        plain.append(run(0)); polished.append(run(1))
    accepted = int(np.sum(rb.polish_status() == 1))
    info = dev[2].numpy()
    return plain, polished, accepted, info


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
    rho = F.OPTS.get("rho", 0.1)
    rng = np.random.default_rng(1)
    out = {}
    for pos, (kind, args) in enumerate(SHAPES):
        seed = 4000 + pos
        name = "%s(%s)" % (kind, ", ".join(str(v) for v in args))
        have = 4 * CORES
        cpu = None
        if a.cpu_seconds > 0:  # the CPU leg first, in fresh processes that never open the device (0: left out, for a run under a profiler)
            with mp.get_context("spawn").Pool(CORES) as pool:
                res = pool.map(_cpu_worker, [(kind, args, seed, have, r, CORES, a.cpu_seconds) for r in range(CORES)])
            kk, acc, ps, tmax = sum(r[0] for r in res), sum(r[1] for r in res), sum(r[2] for r in res), max(r[3] for r in res)
            cpu = dict(cores=CORES, polished_solves=kk, accepted=acc, polish_time_mean_ms=round(1e3 * ps / kk, 4),
                       ms_to_polish_all_instances_on_16_cores=round(1e3 * (ps / kk) * a.copies / CORES, 1),
                       sample=f"{kk} solves (setup + solve + polish) of the first {have} instances over {CORES} processes in {tmax:.1f} s; polish_time is the oracle's own timer")
        (P, A, Px, Ax, q, l, u), _ = F.instances(F.BUILDERS[kind](*args), a.copies, seed)
        plan = batch.large_factor_plan(lib, P, A)
        rb = batch.ResidentBatch(lib, P, A, Px, Ax, q, l, u, large=True, large_factor=True, **dict(F.OPTS, warm_start=False))
        plain, polished, accepted, info = _resolves(rb, a.rounds, rho)
        n, m, cnt = rb.n, rb.m, rb.count
        filled = lambda rows, w: batch.DeviceArray(lib, rows, w).upload(rng.standard_normal((rows, w)))
        calls = {}
        for lead in (1, MANY):
            gx, gy = _View(filled(lead * cnt, n), lead), _View(filled(lead * cnt, m), lead)
            og = {k: _View(batch.DeviceArray(lib, lead * cnt, w), lead) for k, w in (("q", n), ("l", m), ("u", m))}
            og["status"] = batch.DeviceArray(lib, cnt, 1)
            calls[f"adjoint_ncot{lead}"] = _timed(lambda: rb.adjoint(dx=gx, dy=gy, want=("q", "l", "u"), out=og), a.rounds)
            st_a = float(np.mean(og["status"].numpy() == 1))
            tq, tl, tu = _View(filled(lead * cnt, n), lead), _View(filled(lead * cnt, m), lead), _View(filled(lead * cnt, m), lead)
            ot = dict(x=_View(batch.DeviceArray(lib, lead * cnt, n), lead), y=_View(batch.DeviceArray(lib, lead * cnt, m), lead),
                      status=batch.DeviceArray(lib, cnt, 1))
            calls[f"jvp_ndir{lead}"] = _timed(lambda: rb.jvp(q=tq, l=tl, u=tu, out=ot), a.rounds)
            st_j = float(np.mean(ot["status"].numpy() == 1))
            for arr in (gx, gy, tq, tl, tu, og["q"], og["l"], og["u"], ot["x"], ot["y"]):
                arr.arr.free()
        rb.close()
        solve_ms, pol_ms = statistics.median(plain), statistics.median(polished) - statistics.median(plain)
        out[name] = dict(
            n=n, m=m, instances=cnt, seed=seed, plan=plan, solved=int((info[:, 1] == 1).sum()), polish_accepted=accepted,
            differentiated_fraction=dict(adjoint=st_a, jvp=st_j), mean_iterations=round(float(info[:, 0].mean()), 2),
            solve_launch=_stats(plain), resolve_with_polish=_stats(polished), polish_launch_ms=round(pol_ms, 3),
            polish_launch_over_solve_launch=round(pol_ms / solve_ms, 3),
            launches={k: dict(_stats(v), over_solve_launch=round(statistics.median(v) / solve_ms, 3)) for k, v in calls.items()},
            ms_per_further_cotangent=round((statistics.median(calls[f"adjoint_ncot{MANY}"]) - statistics.median(calls["adjoint_ncot1"])) / (MANY - 1), 3),
            ms_per_further_direction=round((statistics.median(calls[f"jvp_ndir{MANY}"]) - statistics.median(calls["jvp_ndir1"])) / (MANY - 1), 3),
            cpu_oracle=cpu)
        print(name, json.dumps(out[name]))
    # the neighbour: the LDS form of the polish kernel at n = 128
    kind, args = NEIGHBOUR
    (P, A, Px, Ax, q, l, u), _ = F.instances(F.BUILDERS[kind](*args), a.copies, 4100)
    rb = batch.ResidentBatch(lib, P, A, Px, Ax, q, l, u, **dict(F.OPTS, warm_start=False))
    plain, polished, accepted, info = _resolves(rb, a.rounds, rho)
    kernel = batch.last_schedule(lib)["entry"]
    rb.close()
    out["neighbour %s(%s), k_batch_polish with M in LDS" % (kind, ", ".join(str(v) for v in args))] = dict(
        n=args[0], m=args[1], instances=a.copies, seed=4100, solve_kernel=kernel, solved=int((info[:, 1] == 1).sum()), polish_accepted=accepted,
        solve_launch=_stats(plain), resolve_with_polish=_stats(polished),
        polish_launch_ms=round(statistics.median(polished) - statistics.median(plain), 3))
    print(json.dumps(out[list(out)[-1]]))
    _merge(a.out, "shapes", out)
    _merge(a.out, "settings", dict(F.OPTS, warm_start=False, copies=a.copies, rounds=a.rounds, gradients="dq, dl, du", tangents="tq, tl, tu"))


BENCH_KEYS = ("ms_per_step",)
TIMED_SUFFIX = "_median"


def controls(a):
    rows = {}
    for row in open(a.lines):
        row = row.rstrip("\n")
        if not row:
            continue
        control, side, rnd, js = row.split("\t", 3)
        rows.setdefault(control, []).append((side, int(rnd), json.loads(js)))
    result = {}
    for control, lines in rows.items():
        keys = BENCH_KEYS if control == "bench" else sorted(k for k in lines[0][2] if k.startswith("ms_") and k.endswith(TIMED_SUFFIX))
        figures = {}
        for k in keys:
            parent = [rec[k] for side, _, rec in lines if side == "parent"]
            change = [rec[k] for side, _, rec in lines if side == "change"]
            figures[k] = dict(parent=parent, change=change, change_median=statistics.median(change),
                              inside_parent_spread=bool(min(parent) <= statistics.median(change) <= max(parent)),
                              not_slower_than_parent_max=bool(statistics.median(change) <= max(parent)))
        entry = dict(figures=figures, rounds=[dict(side=s, round=r) for s, r, _ in lines])
        if control == "bench":
            entry["packed_sha16"] = sorted({rec.get("packed_sha16") for _, _, rec in lines})
            entry["sha_equal"] = len(entry["packed_sha16"]) == 1
            entry["lines"] = [dict(side=s, round=r, ms_per_step=rec["ms_per_step"], value=rec["value"], unit=rec.get("unit"),
                                   packed_sha16=rec.get("packed_sha16"), solved=rec.get("solved")) for s, r, rec in lines]
        result[control] = entry
        print(control, json.dumps({k: (v["inside_parent_spread"], v["not_slower_than_parent_max"]) for k, v in figures.items()}))
    _merge(a.out, "controls", dict(
        how="the parent's libosqp_amd.so (OSQP_AMD_LIB) and this tree alternated three times in one job, one process per line; "
            "bench: bench.py --gpus 1 --steps 100 --warmup 25 --workload mpc-batch --no-cpu; adjoint / jvp: tools/batch_closed_loop.py "
            "--adjoint / --jvp on 4096 MPC QPs (the LDS forms of k_batch_polish, k_batch_adjoint, k_batch_jvp: the kernels that gained a "
            "template argument)", **result))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    m = sub.add_parser("measure")
    m.add_argument("--copies", type=int, default=4096)
    m.add_argument("--rounds", type=int, default=5)
    m.add_argument("--cpu-seconds", type=float, default=6.0)
    m.add_argument("--out", default=DEFAULT_OUT)
    r = sub.add_parser("controls")
    r.add_argument("lines")
    r.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    {"measure": measure, "controls": controls}[a.cmd](a)


if __name__ == "__main__":
    main()
