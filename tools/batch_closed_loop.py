#!/usr/bin/env python3
"""The closed loop of a batched model-predictive controller, four ways: `count` MPC instances (host generator, seed 5),
W warm-up and K timed control periods; between periods every instance gets the perturbation of the warm-start test
(batch_resident_ref.closed_loop_steps: the initial-state rows and q[0:6] move a little).  Legs, alternated period by period
inside one process, each ending in a device synchronise (every library call blocks until done):
  A  batch.solve_batch per period: upload everything, Ruiz, cold start, download (the only option before the handle);
  B  ResidentBatch with warm_start = 0: what residency and the kept scaling buy alone;
  C  ResidentBatch, warm, host-pointer updates and outputs;
  D  ResidentBatch, warm, device-pointer updates and device outputs (the period's q, l, u are already in HBM).
One JSON line per leg: ms per period (median and mean over the timed periods), ADMM iterations per period, ms per 1000
instance-iterations.  The library has no per-kernel event timer for the batched path, so the kernel's share is not reported.
--polish: the resident legs B, C, D run with settings.polish = 1 (a second launch per period polishes the Solved instances);
leg A, the one-shot entry, ignores the setting.  Their lines then carry `polished_fraction`: accepted polishes per
instance-period.
--adjoint: instead of the four legs, the cost of differentiating the loop.  Two leg-D handles (device pointers) take the same
updates, one with polish = 0 and one with polish = 1; per period, alternated, each call timed on its own (every call blocks):
the resolve of the first, the resolve + polish launch of the second, then on the second `adjoint` with all five gradients
and with dq, dl, du only (device inputs and outputs).  One JSON line: the median over the timed periods of each, the mean
iterations of the two resolves, and the polish launch estimated as the second resolve minus the first scaled by their
iteration counts (the two handles warm-start from different points, so their ADMM launches are not the same work).
--jvp: the cost of the forward sensitivities next to the adjoint of the same job.  One leg-D handle (polish = 0, device
pointers); per period, each call timed on its own: the resolve, `adjoint` with all five gradients and with dq, dl, du only,
then `jvp` with all five tangents and with tq, tl, tu only, each at ndir = 1 and ndir = 8 (device inputs and outputs; one
launch per call: one factorisation per instance, one solve per direction).  One JSON line with the medians and minima over the
timed periods, also written to profiles/batch_jvp.json (--out=PATH: elsewhere).
usage: python tools/batch_closed_loop.py [--polish | --adjoint | --jvp [--out=PATH]] [count] [K] [W]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import osqp_jl_amd as oq  # noqa: E402
from osqp_jl_amd import batch  # noqa: E402
import batch_resident_ref as ref  # noqa: E402

POLISH = "--polish" in sys.argv[1:]
ADJOINT = "--adjoint" in sys.argv[1:]
JVP = "--jvp" in sys.argv[1:]
JVP_OUT = ([a[6:] for a in sys.argv[1:] if a.startswith("--out=")] or [os.path.join(ROOT, "profiles", "batch_jvp.json")])[-1]
argv = [a for a in sys.argv[1:] if a not in ("--polish", "--adjoint", "--jvp") and not a.startswith("--out=")]
count = int(argv[0]) if len(argv) > 0 else 4096
K = int(argv[1]) if len(argv) > 1 else 10
W = int(argv[2]) if len(argv) > 2 else 2
lib = oq.load_library()
olib = oq.load_library(oq.ORACLE_LIB_PATH)  # the host generator only
OPTS = dict(verbose=False, eps_abs=1e-5, eps_rel=1e-5, adaptive_rho_interval=50, max_iter=4000, polish=POLISH)

args = ref.stack(ref.mpc_instances(olib, 0, count, 5))
P0, A0, Px, Ax, q, l, u = args
steps = ref.closed_loop_steps(q, l, u, steps=W + K + 1)
dev = lambda a: batch.DeviceArray(lib, *a.shape).upload(a)


def adjoint_legs():
    h0, h1 = batch.ResidentBatch(lib, *args, **dict(OPTS, polish=False)), batch.ResidentBatch(lib, *args, **dict(OPTS, polish=True))
    out0, out1 = h0.alloc(), h1.alloc()
    h0.solve(out=out0); h1.solve(out=out1)
    rng = np.random.default_rng(0)
    gx, gy = dev(rng.standard_normal((count, h1.n))), dev(rng.standard_normal((count, h1.m)))
    cols = dict(q=h1.n, l=h1.m, u=h1.m, Px=h1.nnzP, Ax=h1.nnzA, act=h1.m, status=1)
    outs = {k: batch.DeviceArray(lib, count, c) for k, c in cols.items()}
    t = {k: [] for k in ("resolve", "resolve_polish", "adjoint_all", "adjoint_qlu")}
    its, differentiated = {"resolve": [], "resolve_polish": []}, 0
    for k in range(1, W + K + 1):
        dq, dl, du = (dev(a) for a in steps[k])
        for name, h, out in (("resolve", h0, out0), ("resolve_polish", h1, out1)):
            h.update(q=dq, l=dl, u=du)
            t0 = time.perf_counter()
            h.solve(out=out)
            t[name].append(1e3 * (time.perf_counter() - t0))
            its[name].append(float(np.sum(out[2].numpy()[:, 0])))
        for name, want in (("adjoint_all", ("q", "l", "u", "Px", "Ax")), ("adjoint_qlu", ("q", "l", "u"))):
            t0 = time.perf_counter()
            h1.adjoint(dx=gx, dy=gy, want=want, out=outs)
            t[name].append(1e3 * (time.perf_counter() - t0))
        if k > W:
            differentiated += int(np.sum(outs["status"].numpy() == 1))
        for a in (dq, dl, du):
            a.free()
    med = {k: float(np.median(v[W:])) for k, v in t.items()}
    it = {k: float(np.mean(v[W:])) for k, v in its.items()}
    print(json.dumps(dict(what="adjoint of the closed loop, device pointers", instances=count, periods=K, warmup=W,
                          kernel=int(lib.osqp_amd_batch_last_kernel()), ms_resolve_median=med["resolve"],
                          ms_resolve_with_polish_median=med["resolve_polish"], iterations_resolve=it["resolve"],
                          iterations_resolve_with_polish=it["resolve_polish"],
                          ms_polish_launch_estimate=med["resolve_polish"] - med["resolve"] * it["resolve_polish"] / it["resolve"],
                          ms_adjoint_all_median=med["adjoint_all"], ms_adjoint_qlu_median=med["adjoint_qlu"],
                          ms_adjoint_all_min=float(np.min(t["adjoint_all"][W:])), ms_adjoint_qlu_min=float(np.min(t["adjoint_qlu"][W:])),
                          differentiated_fraction=differentiated / (count * K))))
    h0.close(); h1.close()


class Directions:
    """A [ndir x count x cols] device array for `ResidentBatch.jvp`: a DeviceArray of ndir * count rows, passed by address."""

    def __init__(self, ndir, rows, cols, host=None):
        self.arr, self.shape = batch.DeviceArray(lib, ndir * rows, cols), (ndir, rows, cols)
        if host is not None:
            self.arr.upload(host.reshape(ndir * rows, cols))

    def data_ptr(self):
        return self.arr.data_ptr()


def jvp_legs():
    h = batch.ResidentBatch(lib, *args, **dict(OPTS, polish=False))
    out = h.alloc()
    h.solve(out=out)
    rng = np.random.default_rng(0)
    gx, gy = dev(rng.standard_normal((count, h.n))), dev(rng.standard_normal((count, h.m)))
    cols = dict(q=h.n, l=h.m, u=h.m, Px=h.nnzP, Ax=h.nnzA, act=h.m, status=1)
    outs = {k: batch.DeviceArray(lib, count, c) for k, c in cols.items()}
    dirs = (1, 8)
    tang = {nd: {k: Directions(nd, count, cols[k], rng.standard_normal((nd, count, cols[k]))) for k in ("q", "l", "u", "Px", "Ax")} for nd in dirs}
    touts = {nd: dict(x=Directions(nd, count, h.n), y=Directions(nd, count, h.m), status=outs["status"]) for nd in dirs}
    names = ["resolve", "adjoint_all", "adjoint_qlu"] + [f"jvp_{w}_ndir{nd}" for w in ("all", "qlu") for nd in dirs]
    t = {k: [] for k in names}
    its, differentiated = [], 0
    for k in range(1, W + K + 1):
        dq, dl, du = (dev(a) for a in steps[k])
        h.update(q=dq, l=dl, u=du)
        t0 = time.perf_counter()
        h.solve(out=out)
        t["resolve"].append(1e3 * (time.perf_counter() - t0))
        its.append(float(np.sum(out[2].numpy()[:, 0])))
        for name, want in (("adjoint_all", ("q", "l", "u", "Px", "Ax")), ("adjoint_qlu", ("q", "l", "u"))):
            t0 = time.perf_counter()
            h.adjoint(dx=gx, dy=gy, want=want, out=outs)
            t[name].append(1e3 * (time.perf_counter() - t0))
        for w, keys in (("all", ("q", "l", "u", "Px", "Ax")), ("qlu", ("q", "l", "u"))):
            for nd in dirs:
                t0 = time.perf_counter()
                h.jvp(**{key: tang[nd][key] for key in keys}, out=touts[nd])
                t[f"jvp_{w}_ndir{nd}"].append(1e3 * (time.perf_counter() - t0))
        if k > W:
            differentiated += int(np.sum(outs["status"].numpy() == 1))
        for a in (dq, dl, du):
            a.free()
    res = dict(what="forward sensitivities of the closed loop next to its adjoint, device pointers, one call timed at a time",
               instances=count, periods=K, warmup=W, kernel=int(lib.osqp_amd_batch_last_kernel()), iterations_resolve=float(np.mean(its[W:])),
               differentiated_fraction=differentiated / (count * K))
    for name in names:
        res[f"ms_{name}_median"] = float(np.median(t[name][W:]))
        res[f"ms_{name}_min"] = float(np.min(t[name][W:]))
    res["ms_per_further_direction_all"] = (res["ms_jvp_all_ndir8_median"] - res["ms_jvp_all_ndir1_median"]) / 7
    res["ms_per_further_direction_qlu"] = (res["ms_jvp_qlu_ndir8_median"] - res["ms_jvp_qlu_ndir1_median"]) / 7
    line = json.dumps(res)
    print(line)
    with open(JVP_OUT, "w") as f:
        f.write(line + "\n")
    h.close()


if ADJOINT:
    adjoint_legs()
    sys.exit(0)
if JVP:
    jvp_legs()
    sys.exit(0)
handles = {"B": batch.ResidentBatch(lib, *args, **dict(OPTS, warm_start=False)), "C": batch.ResidentBatch(lib, *args, **OPTS),
           "D": batch.ResidentBatch(lib, *args, **OPTS)}
out_d = handles["D"].alloc()
for h in handles.values():  # period 0: the data as set up
    h.solve()
times = {k: [] for k in "ABCD"}
iters = {k: [] for k in "ABCD"}
solved = {k: 0 for k in "ABCD"}
polished = {k: 0 for k in "ABCD"}
for k in range(1, W + K + 1):
    qk, lk, uk = steps[k]
    dq, dl, du = dev(qk), dev(lk), dev(uk)  # leg D's inputs live in HBM before its period starts
    for leg in "ABCD":
        t0 = time.perf_counter()
        if leg == "A":
            x, y, info = batch.solve_batch(lib, P0, A0, Px, Ax, qk, lk, uk, **OPTS)
        elif leg == "D":
            handles[leg].update(q=dq, l=dl, u=du)
            handles[leg].solve(out=out_d)
        else:
            handles[leg].update(q=qk, l=lk, u=uk)
            x, y, info = handles[leg].solve()
        dt = time.perf_counter() - t0
        if leg == "D":
            info = out_d[2].numpy()  # outside the timed stretch: a controller would consume it on the device
        if POLISH and leg != "A" and k > W:
            polished[leg] += int(np.sum(handles[leg].polish_status() == 1))  # outside the timed stretch too
        if k > W:
            times[leg].append(1e3 * dt); iters[leg].append(float(np.sum(info[:, 0]))); solved[leg] += int(np.sum(info[:, 1] == 1))
    for a in (dq, dl, du):
        a.free()
what = {"A": "solve_batch per period (upload, Ruiz, cold, download)", "B": "resident, warm_start=0", "C": "resident, warm, host pointers",
        "D": "resident, warm, device pointers and device outputs"}
for leg in "ABCD":
    ms, it = float(np.median(times[leg])), float(np.mean(iters[leg]))
    print(json.dumps(dict(leg=leg, what=what[leg], instances=count, periods=K, warmup=W, kernel=int(lib.osqp_amd_batch_last_kernel()),
                          ms_per_period_median=ms, ms_per_period_mean=float(np.mean(times[leg])), ms_per_period_min=float(np.min(times[leg])),
                          iterations_per_period=it, ms_per_1000_instance_iterations=1e3 * float(np.mean(times[leg])) / it,
                          solved_fraction=solved[leg] / (count * K),
                          **(dict(polish=1, polished_fraction=polished[leg] / (count * K)) if POLISH and leg != "A" else {}))))
for h in handles.values():
    h.close()
