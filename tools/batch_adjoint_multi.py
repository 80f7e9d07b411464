#!/usr/bin/env python3
"""What further cotangents of one adjoint launch cost: the handle of tools/batch_subset_deriv.py (`count` MPC instances: 64
of the host generator, seed 5, tiled; polish = 0, solved once) and the time of `adjoint` with all five gradients at ncot = 1,
4 and 8 cotangents per launch -- the whole batch, and `rows=` of 64 instances (the first 64 of one random permutation) --
beside 8 separate one-cotangent calls.  Device-pointer form: cotangents and gradients stay in HBM.  A host clock around the
blocking call (around all eight for the separate calls), W warm-up rounds, then K timed ones, the legs alternated call by
call.  One JSON object: min / median / max ms per leg, and the cost of each cotangent after the first against a
one-cotangent call.  A report, not a gate.
usage: python tools/batch_adjoint_multi.py [--out FILE] [count] [K] [W]"""
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
NCOTS = (1, 4, 8)
SEPARATE = 8
SUBSET = min(64, count)
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
    """A [ncot x k x cols] view of a DeviceArray of ncot * k rows, as `ResidentBatch.adjoint` takes it by address."""

    def __init__(self, arr, ncot):
        self.arr, self.shape = arr, (ncot, arr.shape[0] // ncot, arr.shape[1])

    def data_ptr(self):
        return self.arr.data_ptr()


def filled(rows, width):
    return batch.DeviceArray(lib, rows, width).upload(rng.standard_normal((rows, width)))


def multi(rows, ncot):
    """The arguments of one launch with ncot cotangents."""
    k = count if rows is None else len(rows)
    out = {name: View(batch.DeviceArray(lib, ncot * k, w), ncot) for name, w in cols.items()}
    out["status"] = batch.DeviceArray(lib, k, 1)
    return dict(dx=View(filled(ncot * k, h.n), ncot), dy=View(filled(ncot * k, h.m), ncot), out=out, rows=rows)


def single(rows):
    """The arguments of a one-cotangent call without the leading axis: the existing entry."""
    k = count if rows is None else len(rows)
    out = {name: batch.DeviceArray(lib, k, w) for name, w in cols.items()}
    out["status"] = batch.DeviceArray(lib, k, 1)
    return dict(dx=filled(k, h.n), dy=filled(k, h.m), out=out, rows=rows)


order = np.random.default_rng(0).permutation(count)
legs = {}
for tag, rows in (("whole", None), (f"rows{SUBSET}", np.ascontiguousarray(order[:SUBSET]))):
    for nc in NCOTS:
        legs[f"{tag}_ncot{nc}"] = (rows, nc, [multi(rows, nc)])
    legs[f"{tag}_separate{SEPARATE}"] = (rows, SEPARATE, [single(rows) for _ in range(SEPARATE)])
times = {name: [] for name in legs}
for rep in range(W + K):
    for name, (rows, nc, calls) in legs.items():
        t0 = time.perf_counter()
        for kw in calls:
            h.adjoint(**kw)
        dt = time.perf_counter() - t0
        if rep >= W:
            times[name].append(1e3 * dt)
res = dict(what="resident MPC batch, polish = 0, device pointers: adjoint (five gradients) with ncot cotangents per launch, the whole batch "
                "and rows= of a selection, beside separate one-cotangent calls; host clock around the blocking call(s), legs alternated "
                "call by call", instances=count, tile=TILE, repetitions=K, warmup=W, solved_fraction=float(np.mean(info[:, 1] == 1)), legs={})
for name, (rows, nc, calls) in legs.items():
    t = np.array(times[name])
    status = calls[0]["out"]["status"].numpy()
    res["legs"][name] = dict(instances=count if rows is None else len(rows), cotangents=nc, launches=len(calls), ms_min=float(t.min()),
                             ms_median=float(np.median(t)), ms_max=float(t.max()), differentiated_fraction=float(np.mean(status == 1)))
for tag in ("whole", f"rows{SUBSET}"):
    one = res["legs"][f"{tag}_ncot1"]["ms_median"]
    for nc in NCOTS[1:]:
        leg = res["legs"][f"{tag}_ncot{nc}"]
        leg["ms_per_further_cotangent"] = (leg["ms_median"] - one) / (nc - 1)
        leg["further_cotangent_over_one_call"] = leg["ms_per_further_cotangent"] / one
    res["legs"][f"{tag}_ncot{SEPARATE}"]["fraction_of_separate_calls"] = (res["legs"][f"{tag}_ncot{SEPARATE}"]["ms_median"] /
                                                                         res["legs"][f"{tag}_separate{SEPARATE}"]["ms_median"])
line = json.dumps(res)
print(line)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
h.close()
