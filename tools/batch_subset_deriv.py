#!/usr/bin/env python3
"""What the derivatives of a selection of the resident batch cost: a handle of `count` MPC instances (64 instances of the host
generator, seed 5, tiled), polish = 0, solved once, and the time of `adjoint` (all five gradients) and of `jvp` (all five
tangents; ndir = 1 and ndir = 8) -- every instance, one launch of `count` workgroups -- against the same calls with `rows=` of
64, 512, 768 and 2048 instances (the first k of one random permutation of the instance numbers, so every selection holds
the same mix of instances as the batch).  Device-pointer form: gradients, tangents and results stay in HBM; the selection
itself is host data, uploaded inside the call.  A host clock around the blocking call, W warm-up calls, then K timed ones
per leg, the legs alternated call by call.  One JSON object: min / median / max ms per call and leg, and ms per 4096
instances for comparison.  A report, not a gate.
usage: python tools/batch_subset_deriv.py [--out FILE] [count] [K] [W]"""
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

argv = sys.argv[1:]
out_path = None
if "--out" in argv:
    at = argv.index("--out")
    out_path = argv[at + 1]
    del argv[at:at + 2]
count = int(argv[0]) if len(argv) > 0 else 4096
K = int(argv[1]) if len(argv) > 1 else 50
W = int(argv[2]) if len(argv) > 2 else 5
SIZES = [k for k in (64, 512, 768, 2048) if k <= count]
NDIRS = (1, 8)
TILE = 64

lib = oq.load_library()
olib = oq.load_library(oq.ORACLE_LIB_PATH)  # the host generator only
OPTS = dict(verbose=False, eps_abs=1e-5, eps_rel=1e-5, adaptive_rho_interval=50, max_iter=4000, polish=False)

P0, A0, *arrays = ref.stack(ref.mpc_instances(olib, 0, min(TILE, count), 5))
reps = -(-count // TILE)
arrays = [np.tile(a, (reps, 1))[:count] for a in arrays]
h = batch.ResidentBatch(lib, P0, A0, *arrays, **OPTS)
info = h.solve()[2]
cols = dict(q=h.n, l=h.m, u=h.m, Px=h.nnzP, Ax=h.nnzA)
rng = np.random.default_rng(1)


class View:
    """A [ndir x k x cols] view of a DeviceArray of ndir * k rows, as `ResidentBatch.jvp` takes it by address."""

    def __init__(self, arr, ndir):
        self.arr, self.shape = arr, (ndir, arr.shape[0] // ndir, arr.shape[1])

    def data_ptr(self):
        return self.arr.data_ptr()


def filled(rows, width):
    return batch.DeviceArray(lib, rows, width).upload(rng.standard_normal((rows, width)))


def leg(rows):
    """The device arrays of the three calls for a leg of k instances."""
    k = count if rows is None else len(rows)
    calls = dict(adjoint=dict(dx=filled(k, h.n), dy=filled(k, h.m), out={name: batch.DeviceArray(lib, k, w) for name, w in cols.items()},
                              rows=rows))
    for nd in NDIRS:
        tang = {name: View(filled(nd * k, w), nd) for name, w in cols.items()}
        calls[f"jvp_ndir{nd}"] = dict(**tang, out=dict(x=View(batch.DeviceArray(lib, nd * k, h.n), nd), y=View(batch.DeviceArray(lib, nd * k, h.m), nd),
                                                       status=batch.DeviceArray(lib, k, 1)), rows=rows)
    calls["adjoint"]["out"]["status"] = batch.DeviceArray(lib, k, 1)
    return k, calls


order = np.random.default_rng(0).permutation(count)
legs = [("whole", leg(None))] + [(str(k), leg(np.ascontiguousarray(order[:k]))) for k in SIZES]
names = list(legs[0][1][1])
times = {call: {name: [] for name, _ in legs} for call in names}
for rep in range(W + K):
    for call in names:
        fn = h.adjoint if call == "adjoint" else h.jvp
        for name, (k, calls) in legs:
            t0 = time.perf_counter()
            fn(**calls[call])
            dt = time.perf_counter() - t0
            if rep >= W:
                times[call][name].append(1e3 * dt)
res = dict(what="resident MPC batch, polish = 0, device pointers: adjoint (five gradients) and jvp (five tangents) of the whole batch "
                "against rows= of k instances; host clock around the blocking call, legs alternated call by call",
           instances=count, tile=TILE, repetitions=K, warmup=W, solved_fraction=float(np.mean(info[:, 1] == 1)), calls={})
for call in names:
    res["calls"][call] = {}
    for name, (k, calls) in legs:
        status = calls[call]["out"]["status"].numpy()
        t = np.array(times[call][name])
        res["calls"][call][name] = dict(instances=k, workgroups=k, ms_min=float(t.min()), ms_median=float(np.median(t)), ms_max=float(t.max()),
                                        ms_median_per_4096_instances=float(np.median(t)) * 4096 / k,
                                        differentiated_fraction=float(np.mean(status == 1)),
                                        fraction_of_whole_median=float(np.median(t) / np.median(times[call]["whole"])))
line = json.dumps(res)
print(line)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
h.close()
