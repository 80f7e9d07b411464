#!/usr/bin/env python3
"""What a forward sensitivity of a single model costs (osqp_amd_jvp): on control-1e6 and grid2d-5e5, built as
tools/model_adjoint.py builds them (bench.py's problems and settings with polish = 1) -- one solve, then: the first jvp call
(classification, analysis, factorisation, one direction in q, l, u), K further calls at ndir = 1 and at ndir = 8 on the kept
factor with tq, tl, tu only and with all five tangents (host arrays in and out, so the copies are inside; the first call
with tPx / tAx also builds the two maps and is timed on its own), one adjoint call with dq, dl, du only on the same factor
for comparison, and the bytes of the two maps.  A host clock around the blocking calls.  One JSON object per workload into
the output file.  A report, not a gate.
usage: python tools/model_jvp.py [--out FILE] [--scale F] [K]      (--scale 0.01: the same structures 100 times smaller)"""
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

argv = sys.argv[1:]
out_path, scale = os.path.join(ROOT, "profiles", "model_jvp.json"), 1.0
for flag in ("--out", "--scale"):
    if flag in argv:
        at = argv.index(flag)
        if flag == "--out":
            out_path = argv[at + 1]
        else:
            scale = float(argv[at + 1])
        del argv[at:at + 2]
K = int(argv[0]) if argv else 5
lib = oq.load_library()
SETTINGS = dict(bench.SETTINGS, polish=True)


def build(workload):
    kind, size, _, linsys = bench.WORKLOADS[workload]
    if kind == "control":
        prob = bench.control_problem(max(4, int(size * scale)))
    else:
        prob = qp_zoo.grid2d(max(8, int(size * scale ** 0.5)))
    model = oq.Model(lib)
    t0 = time.time()
    oq.setup(model, linsys_solver=linsys, **prob, **SETTINGS)
    return model, time.time() - t0


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(min_ms=min(ts), median_ms=float(np.median(ts)), max_ms=max(ts))


report = dict(scale=scale, K=K, settings={k: v for k, v in SETTINGS.items()}, workloads={})
for workload in ("control-1e6", "grid2d-5e5"):
    model, setup_s = build(workload)
    n, m = oq.dimensions(model)
    r = oq.solve(model)
    st = oq.stats(model)
    nnzA, nnzP = int(st[1]), int(st[3])
    rec = dict(n=n, m=m, nnzA=nnzA, nnzP_triu=nnzP, setup_s=setup_s, status=r.info.status, iters=r.info.iter,
               status_polish=r.info.status_polish, polish_time_ms=r.info.polish_time * 1e3, refine=int(SETTINGS.get("polish_refine_iter", 3)))
    if r.info.status == "Solved":
        rng = np.random.default_rng(1)
        d = dict(q=rng.standard_normal((8, n)), l=rng.standard_normal((8, m)), u=rng.standard_normal((8, m)),
                 Px=rng.standard_normal((8, nnzP)), Ax=rng.standard_normal((8, nnzA)))
        vec = ("q", "l", "u")
        one = lambda names: {k: d[k][0] for k in names}
        t0 = time.perf_counter()
        first = oq.jvp(model, **one(vec))
        rec["first_call_ms"] = (time.perf_counter() - t0) * 1e3
        s = oq.adjoint_stats(model)
        rec.update(n_low=s["n_low"], n_upp=s["n_upp"], factor_bytes=s["bytes"])
        rec["later_ndir1_vectors_only"] = timed(lambda: oq.jvp(model, **one(vec)), K)
        rec["later_ndir8_vectors_only"] = timed(lambda: oq.jvp(model, **{k: d[k] for k in vec}), K)
        gx, gy = rng.standard_normal(n), rng.standard_normal(m)
        rec["adjoint_ncot1_vectors_only_same_factor"] = timed(lambda: oq.adjoint(model, dx=gx, dy=gy, want=vec), K)
        t0 = time.perf_counter()
        oq.jvp(model, **one(d))
        rec["first_call_with_matrix_tangents_ms"] = (time.perf_counter() - t0) * 1e3  # builds the two maps
        rec["later_ndir1"] = timed(lambda: oq.jvp(model, **one(d)), K)
        rec["later_ndir8"] = timed(lambda: oq.jvp(model, **d), K)
        rec["per_further_direction_ms"] = (rec["later_ndir8"]["median_ms"] - rec["later_ndir1"]["median_ms"]) / 7.0
        rec["per_further_direction_vectors_only_ms"] = (rec["later_ndir8_vectors_only"]["median_ms"] - rec["later_ndir1_vectors_only"]["median_ms"]) / 7.0
        again = oq.jvp(model, **one(vec))
        rec["repeat_is_bit_identical"] = all(np.array_equal(first[k], again[k]) for k in first)
        s2 = oq.adjoint_stats(model)
        rec.update(builds=s2["builds"], kkt_solves=s2["solves"])
        # 4 bytes per position of the full symmetric P (2 nnz(triu P) - its diagonal entries) and per entry of A
        rec["map_bytes_A"] = 4 * nnzA
        rec["map_bytes_P"] = 4 * oq.spmv_layout(model, 2)["nnz"]
        oq.adjoint_release(model)
    oq.clean(model)
    report["workloads"][workload] = rec
    print(workload, json.dumps(rec), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(report, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", out_path)
