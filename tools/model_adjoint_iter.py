#!/usr/bin/env python3
"""What the iterative adjoint of a single model costs (osqp_amd_derivative_method): on rand-1e5 as
bench.py builds it (its CSR arrays kept), on rand-1e5 forced compact (OSQP_AMD_PANEL=2, OSQP_AMD_COMPACT_NNZ=0) and on
rand-1e6 itself (compact by its size) -- bench.py's settings, the indirect back-end, method "iterative" -- one solve, then
the first adjoint call (classification on the device, one cotangent, dq / dl / du) and later calls with dq / dl / du only and
with all five gradients, host arrays and device arrays; after each the outer steps, the CG iterations and the reached drop
of that call.  The time of the osqp_solve beside them.  A call that does not converge is recorded with its message.  A host
clock around the blocking calls.  One JSON object per configuration into the output file.  A report, not a gate.
usage: python tools/model_adjoint_iter.py [--out FILE] [--only NAME[,NAME]] [--skip MEASUREMENT[,...]] [--max-outer N] [--rel-drop X]
       names: rand-1e5, rand-1e5-compact, rand-1e6; a second run merges into an existing output file"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import osqp_jl_amd as oq  # noqa: E402
import bench  # noqa: E402
from osqp_jl_amd.batch import DeviceArray  # noqa: E402

CONFIGS = {"rand-1e5": ("rand-1e5", {}), "rand-1e5-compact": ("rand-1e5", dict(OSQP_AMD_PANEL="2", OSQP_AMD_COMPACT_NNZ="0")), "rand-1e6": ("rand-1e6", {})}
VECTORS = ("q", "l", "u")
MEASUREMENTS = ("first_host_vectors", "later_host_vectors", "later_host_all", "later_device_vectors", "later_device_all")

argv = sys.argv[1:]
opt = {"--out": os.path.join(ROOT, "profiles", "model_adjoint_iter.json"), "--only": ",".join(CONFIGS), "--skip": "", "--max-outer": "", "--rel-drop": ""}
for flag in list(opt):
    if flag in argv:
        at = argv.index(flag)
        opt[flag] = argv[at + 1]
        del argv[at:at + 2]
method_args = {}
if opt["--max-outer"]:
    method_args["max_outer"] = int(opt["--max-outer"])
if opt["--rel-drop"]:
    method_args["rel_drop"] = float(opt["--rel-drop"])
skip = set(filter(None, opt["--skip"].split(",")))
lib = oq.load_library()

report = dict(settings=dict(bench.SETTINGS), method="iterative", method_args=method_args, configurations={})
if os.path.exists(opt["--out"]):
    with open(opt["--out"]) as f:
        report["configurations"] = json.load(f).get("configurations", {})


def call(model, fn):
    """One derivative call: its time and what osqp_amd_derivative_iter_stats says it took."""
    s0 = oq.derivative_iter_stats(model)
    t0 = time.perf_counter()
    try:
        fn()
        err = None
    except oq.OSQPError as ex:
        err = str(ex)
    ms = (time.perf_counter() - t0) * 1e3
    s1 = oq.derivative_iter_stats(model)
    rec = dict(ms=ms, outer_steps=s1["outer_steps"] - s0["outer_steps"], cg_iters=s1["cg_iters"] - s0["cg_iters"], drop=s1["last_drop"])
    if err:
        rec["error"] = err
    return rec


for name in opt["--only"].split(","):
    workload, env = CONFIGS[name]
    kind, size, per_row, linsys = bench.WORKLOADS[workload]
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    model = oq.Model(lib)
    t0 = time.time()
    oq.setup_generated(model, kind, size, per_row, 1, linsys_solver=linsys, **bench.SETTINGS)
    setup_s = time.time() - t0
    for k, v in keep.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    n, m = oq.dimensions(model)
    oq.derivative_method(model, "iterative", **method_args)
    r = oq.solve(model)
    st = oq.stats(model)
    rec = dict(workload=workload, n=n, m=m, nnzA=int(st[1]), nnzP_triu=int(st[3]), compact=int(st[18]), setup_s=setup_s, status=r.info.status,
               iters=r.info.iter, solve_time_ms=r.info.solve_time * 1e3, solve_cg_iters=int(st[6]), skipped=sorted(skip))
    if r.info.status == "Solved":
        rng = np.random.default_rng(1)
        gx, gy = rng.standard_normal(n), rng.standard_normal(m)
        dgx, dgy = DeviceArray(lib, 1, n).upload(gx[None]), DeviceArray(lib, 1, m).upload(gy[None])
        runs = dict(first_host_vectors=lambda: oq.adjoint(model, dx=gx, dy=gy, want=VECTORS),
                    later_host_vectors=lambda: oq.adjoint(model, dx=gx, dy=gy, want=VECTORS),
                    later_host_all=lambda: oq.adjoint(model, dx=gx, dy=gy),
                    later_device_vectors=lambda: oq.adjoint(model, dx=dgx, dy=dgy, want=VECTORS),
                    later_device_all=lambda: oq.adjoint(model, dx=dgx, dy=dgy))
        for what in MEASUREMENTS:
            if what not in skip:
                rec[what] = call(model, runs[what])
                print(name, what, json.dumps(rec[what]), flush=True)
        s, it = oq.adjoint_stats(model), oq.derivative_iter_stats(model)
        rec.update(n_low=s["n_low"], n_upp=s["n_upp"], state_bytes=it["bytes"], builds=it["builds"], solve_cg_iters_after=int(oq.stats(model)[6]))
    oq.clean(model)
    report["configurations"][name] = rec
    print(name, json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opt["--out"])), exist_ok=True)
    with open(opt["--out"], "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
print("wrote", opt["--out"])
