#!/usr/bin/env python3
"""What the duality-gap stopping rule changes and what it costs (osqp_amd_duality_gap_check).

    duality_gap.py effect
        the three cases of tests/duality_cases.py (portfolio(300, 10) with scaling 10 and 0, huber(20, 200); eps 1e-3,
        adaptive_rho_interval 25, direct back-end) on the GPU with the rule off and on: status, iterations, objective, dual
        objective, gap, and the error of the objective against the optimum of a polished solve at eps 1e-9.  One JSON line.
    duality_gap.py check-cost [--steps K] [--rounds R]
        bench.py's lasso-5e5 with check_termination = 1: K iterations (osqp_amd_iterate: one residual evaluation each) with
        the rule off and on, alternated R times in one process after an untimed warm-up of each; a host clock around the
        blocking call.  The difference per evaluation is the cost of the support pass.  One JSON line.
    duality_gap.py bench --root TREE --workload W [--steps K] [--warmup W]
        `bench.py --gpus 1 --steps K --warmup W --workload W --no-cpu` of the tree TREE (this one, or the parent commit
        built in a tree of its own); prints the line's iterations_per_s and ms_per_step.
    duality_gap.py run [--parent TREE] [--out FILE]
        effect, check-cost, and per workload (lasso-5e5 and bench.py's default) three rounds of parent, this tree -- each
        step a process of its own under a time limit of its own; the first that fails ends the run.  Writes
        profiles/duality_gap.json.  A report, not a gate."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _imports(root=HERE):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))


def effect(args):
    _imports()
    import osqp_jl_amd as oq
    import duality_cases as dc

    lib = oq.load_library()
    out = {}
    for name, (make, extra) in dc.RULE_CASES.items():
        prob = make()
        ref = oq.Model(lib)
        oq.setup(ref, **prob, verbose=False, eps_abs=1e-9, eps_rel=1e-9, max_iter=100000, adaptive_rho_interval=25, polish=True,
                 linsys_solver="direct", **extra)
        r = oq.solve(ref)
        best = float(r.info.obj_val)
        rec = dict(optimum=best, optimum_status=r.info.status, optimum_polish=int(r.info.status_polish))
        oq.clean(ref)
        for rule in (False, True):
            m = oq.Model(lib)
            oq.setup(m, **prob, linsys_solver="direct", **dc.RULE_SETTINGS, **extra)
            oq.duality_gap_check(m, rule)
            r = oq.solve(m)
            d = oq.duality(m)
            rec["rule_on" if rule else "rule_off"] = dict(
                status=r.info.status, iter=int(r.info.iter), obj=float(r.info.obj_val), dual_obj=d["dual_obj"], gap=d["gap"],
                obj_error=abs(float(r.info.obj_val) - best), dual_obj_error=abs(d["dual_obj"] - best), gap_refusals=d["gap_refusals"],
                eps_gap_last_check=d["eps_gap"])
            oq.clean(m)
        out[name] = rec
    print(json.dumps(out))


def check_cost(args):
    _imports()
    import torch

    import bench
    import osqp_jl_amd as oq

    lib = oq.load_library()
    kind, n, per_row, linsys = bench.WORKLOADS["lasso-5e5"]
    model = oq.Model(lib)
    oq.setup_generated(model, kind, n, per_row, 1, linsys_solver=linsys, **dict(bench.SETTINGS, check_termination=1))
    nn, mm = oq.dimensions(model)
    ws = model.workspace

    def timed(rule, steps):
        oq.duality_gap_check(model, rule)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert lib.osqp_amd_iterate(ws, steps) == 0
        return (time.perf_counter() - t0) * 1e3 / steps

    timed(False, 10); timed(True, 10)  # warm-up of both
    rounds = [dict(off_ms_per_iteration=timed(False, args.steps), on_ms_per_iteration=timed(True, args.steps)) for _ in range(args.rounds)]
    for r in rounds:
        r["difference_us_per_check"] = 1e3 * (r["on_ms_per_iteration"] - r["off_ms_per_iteration"])
    print(json.dumps(dict(workload="lasso-5e5", n=nn, m=mm, check_termination=1, steps=args.steps, rounds=rounds,
                          support_pass_bytes=24 * mm, duality=oq.duality(model))))


def bench_line(args):
    root = os.path.abspath(args.root)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--workload", args.workload, "--no-cpu"]
    env = dict(os.environ)
    env.pop("OSQP_AMD_LIB", None)
    out = subprocess.run(cmd, cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=args.limit, check=True).stdout.decode()
    line = [l for l in out.splitlines() if l.startswith("{") and '"value"' in l][-1]
    rec = json.loads(line)
    print(json.dumps(dict(root=root, workload=args.workload, iterations_per_s=rec["value"], ms_per_step=rec["ms_per_step"])))


def _child(argv, limit):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, stdout=subprocess.PIPE, timeout=limit, check=True).stdout.decode()
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def run(args):
    rec = dict(command="tools/duality_gap.py run" + (" --parent TREE" if args.parent else ""))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():  # after every step: a run that is cut short leaves what it has
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)

    rec["effect_of_the_rule"] = _child(["effect"], 300)
    save()
    rec["cost_of_a_check"] = _child(["check-cost"], 300)
    save()
    if args.parent:
        default = "rand-1e6"
        rec["bench_command"] = "bench.py --gpus 1 --steps 20 --warmup 5 --workload W --no-cpu"
        rec["bench"] = {}
        for workload, limit in (("lasso-5e5", 240), (default, 420)):
            legs = dict(parent=[], change=[])
            for _ in range(3):
                for leg, root in (("parent", args.parent), ("change", HERE)):
                    r = _child(["bench", "--root", root, "--workload", workload, "--limit", str(limit)], limit + 30)
                    legs[leg].append(dict(iterations_per_s=r["iterations_per_s"], ms_per_step=r["ms_per_step"]))
                    rec["bench"][workload] = legs
                    save()
    save()
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["effect", "check-cost", "bench", "run"])
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--workload", default="lasso-5e5")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "duality_gap.json"))
    args = ap.parse_args()
    if args.steps is None:
        args.steps = 200 if args.what == "check-cost" else 20
    {"effect": effect, "check-cost": check_cost, "bench": bench_line, "run": run}[args.what](args)


if __name__ == "__main__":
    main()
