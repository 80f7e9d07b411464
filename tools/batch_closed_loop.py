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
usage: python tools/batch_closed_loop.py [--polish] [count] [K] [W]"""
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
argv = [a for a in sys.argv[1:] if a != "--polish"]
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
