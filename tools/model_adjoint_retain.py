#!/usr/bin/env python3
"""What keeping the derivative factor across solves buys (osqp_amd_adjoint_retain): on control-1e6 and
grid2d-5e5, built as tools/model_adjoint.py builds them (bench.py's settings with polish = 1), the loop a training step runs.

    model_adjoint_retain.py loop --root TREE --workload W --retain 0|1 [--polish 0]
        one process on TREE's library: setup, solve, the first derivative call, K later calls on the same solution (the
        figure a reused call is held against), the check kernel by itself (osqp_amd_time_kernel id 8: HIP events around it),
        then STEPS steps of  update(q (1 + 1e-4 k)) -- every fifth step update(Px (1 + 1e-4)) instead --, osqp_solve,
        adjoint with dq, dl, du; everything in the device form.  Per step: the time of the derivative call (a host clock
        around the blocking call), of the solve, the builds so far, the retain counters.  One JSON line.  A TREE whose
        library lacks the symbols (the parent commit) runs with --retain 0 only.
    model_adjoint_retain.py run [--parent TREE] [--out FILE] [--rounds R] [--scale F]
        per workload R rounds of: the parent with retain off, this tree with retain off, this tree with retain on -- each a
        process of its own under a time limit of its own; the first child that fails ends the run.  Writes
        profiles/model_adjoint_retain.json.  A report, not a gate."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, K = 10, 5


def loop(args):
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import numpy as np
    import torch

    import bench
    import osqp_jl_amd as oq
    import qp_zoo

    lib = oq.load_library()
    dev = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda:0")
    kind, size, _, linsys = bench.WORKLOADS[args.workload]
    prob = bench.control_problem(max(4, int(size * args.scale))) if kind == "control" else qp_zoo.grid2d(max(8, int(size * args.scale ** 0.5)))
    model = oq.Model(lib)
    oq.setup(model, linsys_solver=linsys, **prob, **dict(bench.SETTINGS, polish=bool(args.polish)))
    has_retain = hasattr(oq, "adjoint_retain")
    if args.retain:
        oq.adjoint_retain(model)
    n, m = oq.dimensions(model)
    cols = oq.interface._data_cols(model)
    rec = dict(root=root, workload=args.workload, retain=int(args.retain), polish=int(args.polish), n=n, m=m, nnzP_triu=cols["Px"], steps=[])
    r = oq.solve(model)
    rec.update(status=r.info.status, iters=r.info.iter, solve_ms=r.info.solve_time * 1e3, polish_ms=r.info.polish_time * 1e3)
    rng = np.random.default_rng(1)
    gx, gy = dev(rng.standard_normal(n)), dev(rng.standard_normal(m))
    q0 = np.asarray(prob["q"], dtype=np.float64)
    import scipy.sparse as sp

    Pt = sp.triu(sp.csc_matrix(prob["P"]), format="csc")
    Pt.sort_indices()
    Px1 = dev(np.asarray(Pt.data, dtype=np.float64) * (1.0 + 1e-4))
    want = ("q", "l", "u")
    outs = dict(q=dev(np.zeros(n)), l=dev(np.zeros(m)), u=dev(np.zeros(m)), act=dev(np.zeros(m)))
    torch.cuda.synchronize()

    def derive():
        t0 = time.perf_counter()
        oq.adjoint(model, dx=gx, dy=gy, want=want, out=outs)
        return (time.perf_counter() - t0) * 1e3

    if r.info.status == "Solved":
        rec["first_call_ms"] = derive()
        later = [derive() for _ in range(K)]
        rec["later_same_solution_ms"] = dict(median=float(np.median(later)), low=min(later), high=max(later))
        rec["factor_bytes"] = oq.adjoint_stats(model)["bytes"]
        if has_retain:
            rec["check_kernel_ms"] = float(lib.osqp_amd_time_kernel(model.workspace, 8, 20))
        act0 = outs["act"].clone()
        for k in range(1, STEPS + 1):
            if k % 5 == 0:
                oq.update(model, Px=Px1)
                what = "Px"
            else:
                oq.update(model, q=dev(q0 * (1.0 + 1e-4 * k)))
                what = "q"
            r = oq.solve(model)
            step = dict(k=k, update=what, status=r.info.status, iters=r.info.iter, solve_ms=r.info.solve_time * 1e3)
            if r.info.status == "Solved":
                step["derivative_ms"] = derive()
                step["rows_changed_since_first"] = int((outs["act"] != act0).sum().item())
            step["builds"] = oq.adjoint_stats(model)["builds"]
            if has_retain:
                step["retain"] = oq.adjoint_retain_stats(model)
            rec["steps"].append(step)
    oq.clean(model)
    print("RECORD " + json.dumps(rec), flush=True)


def child(root, workload, retain, scale, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "loop", "--root", root, "--workload", workload, "--retain", str(retain), "--scale", str(scale)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit)
    if p.returncode != 0:
        sys.stderr.write(p.stdout.decode()[-2000:] + p.stderr.decode()[-4000:])
        raise SystemExit("child failed with %d: %s" % (p.returncode, " ".join(cmd)))
    return json.loads([l for l in p.stdout.decode().splitlines() if l.startswith("RECORD ")][-1][7:])


def summary(runs):
    """Over the rounds of one configuration: per step the derivative times, and the medians by what the step did."""
    import numpy as np

    per_step = [[rnd["steps"][i].get("derivative_ms") for rnd in runs] for i in range(len(runs[0]["steps"]))]
    out = dict(per_step_derivative_ms=per_step, first_call_ms=[rnd.get("first_call_ms") for rnd in runs],
               later_same_solution_ms=[rnd.get("later_same_solution_ms") for rnd in runs])
    last = runs[-1]["steps"][-1] if runs[-1]["steps"] else {}
    if "retain" in last:
        out["counters_after_the_loop"] = last["retain"]
    out["builds_after_the_loop"] = last.get("builds")
    for what in ("q", "Px"):
        v = [t for rnd in runs for s in rnd["steps"] if s["update"] == what and (t := s.get("derivative_ms")) is not None]
        if v:
            out["derivative_ms_after_%s_update" % what] = dict(median=float(np.median(v)), low=min(v), high=max(v))
    return out


def run(args):
    configs = ([("parent_retain_off", os.path.abspath(args.parent), 0)] if args.parent else []) + [("retain_off", HERE, 0), ("retain_on", HERE, 1)]
    report = dict(scale=args.scale, steps=STEPS, K=K, rounds=args.rounds, workloads={})
    for workload in args.workloads:
        runs = {name: [] for name, _, _ in configs}
        for _ in range(args.rounds):
            for name, root, retain in configs:
                runs[name].append(child(root, workload, retain, args.scale, args.limit))
                print(workload, name, [round(s.get("derivative_ms", -1.0), 2) for s in runs[name][-1]["steps"]], flush=True)
        first = runs["retain_on"][0]
        rec = dict(n=first["n"], m=first["m"], factor_bytes=first.get("factor_bytes"), check_kernel_ms=[rnd.get("check_kernel_ms") for rnd in runs["retain_on"]],
                   rows_changed_since_first=[s.get("rows_changed_since_first") for s in first["steps"]],
                   solve_ms=[s["solve_ms"] for s in first["steps"]], polish_ms_of_the_first_solve=first["polish_ms"])
        rec.update({name: summary(v) for name, v in runs.items()})
        report["workloads"][workload] = rec
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["loop", "run"])
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--workload", default="grid2d-5e5")
    ap.add_argument("--workloads", nargs="*", default=["control-1e6", "grid2d-5e5"])
    ap.add_argument("--retain", type=int, default=0)
    ap.add_argument("--polish", type=int, default=1, help="loop: 0 runs the solves without polish (bench.py's own setting)")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "model_adjoint_retain.json"))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--limit", type=int, default=420, help="seconds a child may take")
    a = ap.parse_args()
    {"loop": loop, "run": run}[a.what](a)
