#!/usr/bin/env python3
"""What a subset resolve of the resident batch costs: a handle of `count` MPC instances (64 instances of the host generator,
seed 5, tiled), warm_start = 0 so that every resolve of an instance is a cold solve of the same data, and the time of
`solve(out=...)` -- every instance, one launch of `count` workgroups -- against `solve(out=..., rows=...)` of 64, 512, 768
and 2048 instances (the first k of one random permutation of the instance numbers, so every selection holds the same mix of
instances as the batch).  Device-pointer form: results stay in HBM; the selection itself is host data, uploaded inside the
call.  A host clock around the blocking call, W warm-up calls, then K timed ones per leg, the legs alternated call by call.
One JSON object: min / median / max ms per leg, and ms per 4096 instances for comparison.  A report, not a gate.
usage: python tools/batch_subset.py [--out FILE] [count] [K] [W]"""
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
TILE = 64

lib = oq.load_library()
olib = oq.load_library(oq.ORACLE_LIB_PATH)  # the host generator only
OPTS = dict(verbose=False, eps_abs=1e-5, eps_rel=1e-5, adaptive_rho_interval=50, max_iter=4000, warm_start=False)

P0, A0, *arrays = ref.stack(ref.mpc_instances(olib, 0, min(TILE, count), 5))
reps = -(-count // TILE)
arrays = [np.tile(a, (reps, 1))[:count] for a in arrays]
h = batch.ResidentBatch(lib, P0, A0, *arrays, **OPTS)
order = np.random.default_rng(0).permutation(count)
legs = [("whole", None, h.alloc())] + [(str(k), np.ascontiguousarray(order[:k]), h.alloc(k)) for k in SIZES]
times = {name: [] for name, _, _ in legs}
launched = {}
for rep in range(W + K):
    for name, rows, out in legs:
        t0 = time.perf_counter()
        h.solve(out=out, rows=rows)
        dt = time.perf_counter() - t0
        launched[name] = batch.last_schedule(lib)["instances"]
        if rep >= W:
            times[name].append(1e3 * dt)
whole_info = legs[0][2][2].numpy()
res = dict(what="resident MPC batch, warm_start = 0, device-pointer outputs: a whole resolve against solve(rows=...) of k instances; "
                "host clock around the blocking call, legs alternated call by call",
           instances=count, tile=TILE, repetitions=K, warmup=W, kernel=int(lib.osqp_amd_batch_last_kernel()),
           mean_iterations=float(np.mean(whole_info[:, 0])), solved_fraction=float(np.mean(whole_info[:, 1] == 1)), legs={})
for name, rows, out in legs:
    k = count if rows is None else len(rows)
    assert launched[name] == k, (name, launched[name])
    info = out[2].numpy()  # of the leg's last call (rho is kept per instance, so the counts may differ a little between legs)
    t = np.array(times[name])
    res["legs"][name] = dict(instances=k, workgroups=launched[name], ms_min=float(t.min()), ms_median=float(np.median(t)), ms_max=float(t.max()),
                             ms_median_per_4096_instances=float(np.median(t)) * 4096 / k, mean_iterations=float(np.mean(info[:, 0])),
                             fraction_of_whole_median=float(np.median(t) / np.median(times["whole"])))
line = json.dumps(res)
print(line)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
h.close()
