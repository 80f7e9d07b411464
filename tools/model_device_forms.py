#!/usr/bin/env python3
"""Host form against device form of a single model's calls: on control-1e6 and grid2d-5e5, built as
tools/model_adjoint.py builds them, one solve and one first adjoint (the factor is kept), then ONE job that alternates the
host form and the device form, ROUNDS rounds each of K calls, for: a later adjoint with all five gradients; a later adjoint
with dq, dl, du only; a jvp along all five data arrays; the solution read (host form: the two host mirrors copied out and
uploaded into CUDA tensors, what the host route of `QPLayer` pays to have x, y on the device; device form:
osqp_amd_solution_dev into CUDA tensors); `update(q, l, u)`.  Host form: numpy arrays in and out.  Device form: float64 CUDA
tensors in and out.  A host clock around the blocking calls.  Per figure: the median of every round and, over the rounds, the
middle median with the spread (lowest and highest round median).  A report, not a gate.
usage: python tools/model_device_forms.py [--out FILE] [--scale F] [K]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import osqp_jl_amd as oq  # noqa: E402
import bench  # noqa: E402
import qp_zoo  # noqa: E402
import torch  # noqa: E402

argv = sys.argv[1:]
out_path, scale = os.path.join(ROOT, "profiles", "model_device_forms.json"), 1.0
for flag in ("--out", "--scale"):
    if flag in argv:
        at = argv.index(flag)
        if flag == "--out":
            out_path = argv[at + 1]
        else:
            scale = float(argv[at + 1])
        del argv[at:at + 2]
K = int(argv[0]) if argv else 5
ROUNDS = 3
lib = oq.load_library()
SETTINGS = dict(bench.SETTINGS, polish=True)
DEV = torch.device("cuda:0")


def build(workload):
    kind, size, _, linsys = bench.WORKLOADS[workload]
    if kind == "control":
        prob = bench.control_problem(max(4, int(size * scale)))
    else:
        prob = qp_zoo.grid2d(max(8, int(size * scale ** 0.5)))
    model = oq.Model(lib)
    oq.setup(model, linsys_solver=linsys, **prob, **SETTINGS)
    return model, prob


def dev(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def round_median(fn):
    ts = []
    for _ in range(K):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def alternate(host_fn, dev_fn):
    """ROUNDS rounds, host then device in each; one untimed call of each first."""
    host_fn(); dev_fn()
    med = dict(host=[], device=[])
    for _ in range(ROUNDS):
        med["host"].append(round_median(host_fn))
        med["device"].append(round_median(dev_fn))
    out = {}
    for form, v in med.items():
        out[form] = dict(round_medians_ms=v, median_ms=float(np.median(v)), low_ms=min(v), high_ms=max(v))
    spread = max(out["host"]["high_ms"] - out["host"]["low_ms"], out["device"]["high_ms"] - out["device"]["low_ms"])
    out["host_minus_device_ms"] = out["host"]["median_ms"] - out["device"]["median_ms"]
    out["spread_ms"] = spread
    out["device_faster_beyond_spread"] = bool(out["host_minus_device_ms"] > spread)
    return out


report = dict(scale=scale, K=K, rounds=ROUNDS, settings={k: v for k, v in SETTINGS.items()}, workloads={})
for workload in ("control-1e6", "grid2d-5e5"):
    model, prob = build(workload)
    n, m = oq.dimensions(model)
    r = oq.solve(model)
    cols = oq.interface._data_cols(model)
    rec = dict(n=n, m=m, nnzA=cols["Ax"], nnzP_triu=cols["Px"], status=r.info.status, iters=r.info.iter)
    if r.info.status == "Solved":
        rng = np.random.default_rng(1)
        gx, gy = rng.standard_normal(n), rng.standard_normal(m)
        tang = {k: rng.standard_normal(cols[k]) for k in ("q", "l", "u", "Px", "Ax")}
        dgx, dgy, dtang = dev(gx), dev(gy), {k: dev(v) for k, v in tang.items()}
        torch.cuda.synchronize()
        oq.adjoint(model, dx=gx, dy=gy)  # builds and keeps the factor
        rec["adjoint_five"] = alternate(lambda: oq.adjoint(model, dx=gx, dy=gy), lambda: oq.adjoint(model, dx=dgx, dy=dgy))
        rec["adjoint_vectors"] = alternate(lambda: oq.adjoint(model, dx=gx, dy=gy, want=("q", "l", "u")),
                                           lambda: oq.adjoint(model, dx=dgx, dy=dgy, want=("q", "l", "u")))
        rec["jvp_five"] = alternate(lambda: oq.jvp(model, **tang), lambda: oq.jvp(model, **dtang))
        h, d = oq.adjoint(model, dx=gx, dy=gy), oq.adjoint(model, dx=dgx, dy=dgy)
        hj, dj = oq.jvp(model, **tang), oq.jvp(model, **dtang)
        rec["bit_identical"] = bool(all(np.array_equal(h[k], d[k].cpu().numpy()) for k in h) and
                                    all(np.array_equal(hj[k], dj[k].cpu().numpy()) for k in hj))
        s = oq.adjoint_stats(model)
        rec.update(builds=s["builds"], kkt_solves=s["solves"])
        sol = model.workspace.contents.solution.contents
        hx, hy = np.empty(n), np.empty(m)
        tx, ty = torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(m, dtype=torch.float64, device=DEV)

        def host_solution():
            C.memmove(hx.ctypes.data, sol.x, 8 * n)
            C.memmove(hy.ctypes.data, sol.y, 8 * m)
            tx.copy_(torch.from_numpy(hx)); ty.copy_(torch.from_numpy(hy))
            torch.cuda.synchronize()

        rec["solution_read"] = alternate(host_solution, lambda: oq.solution(model, x=tx, y=ty))
        q, l, u = (np.asarray(prob[k], dtype=np.float64) for k in ("q", "l", "u"))
        dq, dl, du = dev(q), dev(np.maximum(l, -oq.OSQP_INFTY)), dev(np.minimum(u, oq.OSQP_INFTY))
        torch.cuda.synchronize()
        rec["update_q_l_u"] = alternate(lambda: oq.update(model, q=q, l=l, u=u), lambda: oq.update(model, q=dq, l=dl, u=du))
        rec["device_form_calls"] = oq.device_form_calls(model)
    oq.clean(model)
    report["workloads"][workload] = rec
    print(workload, json.dumps(rec), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(report, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", out_path)
