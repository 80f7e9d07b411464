#!/usr/bin/env python3
"""What the forward sensitivities of the shared batch (`SharedBatch.jvp`, k_shared_jvp) cost next to the
only way to the same tangents before them: a resident batch with the matrix values AND the matrix tangents replicated per
instance, and its whole-batch JVP.  Writes profiles/batch_shared_jvp.json (or --out).  A report: no ratio is asserted.

    batch_shared_jvp.py measure [--copies N] [--rounds R] [--baseline-lib PATH] [--out FILE]
        N instances (default 4096) of the boxed family of tests/batch_shared_cases.py on banded(256, 512, 6), random(144, 200, 7)
        and banded(100, 200, 4), settings OPTS of that file (eps 1e-5).  Both sides solve once; then, per number of directions
        (1 and 8), all five tangents in device arrays -- q, l, u per instance on both sides; Px, Ax ONE row per direction on the
        shared side, that row repeated N times on the resident side -- an untimed first call of each side, then R rounds, the two
        sides alternated, a host clock around the blocking calls; median, minimum and maximum of each side, the bytes of the
        tangent arrays of a call and the device bytes.  Baseline: `ResidentBatch` of the library at PATH (default: this tree's;
        pass the parent commit's build) with large=True and large_factor=True above n = 128.  The two sides differentiate
        different instances (a resident instance scales with its own q, a shared one with q0): recorded are the instances on
        which both end on one active set and the relative difference of tx on those.

    batch_shared_jvp.py nonregression LINES [--out FILE]
        LINES: `side<TAB>round<TAB>json line of bench.py --workload mpc-batch`, parent and change alternated (the format and the
        verdict of tools/batch_shared.py)."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_OUT = os.path.join(HERE, "profiles", "batch_shared_jvp.json")
SHAPES = [("banded", (256, 512, 6), 14), ("random", (144, 200, 7), 13), ("banded", (100, 200, 4), 12)]
NDIRS = (1, 8)
WHAT = "the JVP of the shared batch next to a resident batch with replicated matrix values and tangents (DESIGN.md section 13.5)"


def _paths():
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, os.path.join(HERE, "tools"))


def _merge(path, key, value):
    rec = json.load(open(path)) if os.path.exists(path) else {}
    rec.setdefault("device", "MI355X")
    rec["what"] = WHAT
    rec[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def _timed(call):
    t = time.perf_counter()
    call()
    return (time.perf_counter() - t) * 1e3


def _stats(ts):
    return dict(ms=[round(t, 3) for t in ts], median=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3))


def _shape(lib, base_lib, kind, shape, seed, copies, rounds):
    import numpy as np
    import scipy.sparse as sp
    import torch

    from osqp_jl_amd import batch
    import batch_shared_cases as S

    dev = torch.device("cuda:0")
    opts = dict(S.OPTS)
    base, q, l, u = S.boxed_spec(kind, shape, seed, 0, copies)
    P0, q0, A0, l0, u0 = base
    n, m = A0.shape[1], A0.shape[0]
    sb = batch.SharedBatch(lib, P0, A0, q0, l0, u0, copies, **opts)
    sb.update(q=q, l=l, u=u)
    Pu = sp.csc_matrix(sp.triu(P0)); Pu.sort_indices()
    Px, Ax = np.tile(Pu.data, (copies, 1)), np.tile(sp.csc_matrix(A0).data, (copies, 1))
    big = n > 128
    rb = batch.ResidentBatch(base_lib, P0, A0, Px, Ax, q, l, u, large=big, large_factor=big, **opts)
    si, ri = sb.solve()[2], rb.solve()[2]
    cols = dict(q=n, l=m, u=m, Px=int(Pu.nnz), Ax=int(A0.nnz))
    rec = dict(n=n, m=m, nnzP=int(Pu.nnz), nnzA=int(A0.nnz), instances=copies, rounds=rounds,
               solved=dict(shared=int((si[:, 1] == 1).sum()), resident=int((ri[:, 1] == 1).sum())), calls={})
    rng = np.random.default_rng(seed)
    for ndir in NDIRS:
        lead = (ndir,) if ndir > 1 else ()
        ts_ = {k: torch.tensor(rng.standard_normal(lead + ((cols[k],) if k in ("Px", "Ax") else (copies, cols[k]))), device=dev) for k in cols}
        # the resident side: the row of a direction repeated for every instance
        tr_ = {k: (v.unsqueeze(-2).expand(lead + (copies, cols[k])).contiguous() if k in ("Px", "Ax") else v) for k, v in ts_.items()}
        out = dict(x=torch.empty(lead + (copies, n), dtype=torch.float64, device=dev), y=torch.empty(lead + (copies, m), dtype=torch.float64, device=dev))
        torch.cuda.synchronize()
        shared_call, resident_call = (lambda: sb.jvp(**ts_, out=out)), (lambda: rb.jvp(**tr_, out=out))
        shared_call(); resident_call()  # untimed first calls
        ts, tr = [], []
        for _ in range(rounds):  # the two sides alternated
            tr.append(_timed(resident_call))
            ts.append(_timed(shared_call))
        r = dict(shared=_stats(ts), resident=_stats(tr))
        r["resident_over_shared"] = round(r["resident"]["median"] / r["shared"]["median"], 3)
        r["shared_outside_the_baseline_spread"] = bool(
            abs(r["resident"]["median"] - r["shared"]["median"]) > r["resident"]["max"] - r["resident"]["min"])
        r["tangent_bytes"] = dict(shared=int(sum(v.numel() for v in ts_.values()) * 8), resident=int(sum(v.numel() for v in tr_.values()) * 8))
        rec["calls"]["ndir=%d" % ndir] = r
        if ndir == 1:  # the two sides on the instances both differentiate with ONE active set (two eps-accurate solves of one problem)
            side = []
            for h, t in ((sb, ts_), (rb, tr_)):
                o = dict(x=torch.empty_like(out["x"]), y=torch.empty_like(out["y"]), act=torch.empty((copies, m), dtype=torch.float64, device=dev),
                         status=torch.empty((copies, 1), dtype=torch.float64, device=dev))
                h.jvp(**t, out=o)
                side.append({k: v.cpu().numpy() for k, v in o.items()})
            a, b = side
            same = (a["status"][:, 0] == 1) & (b["status"][:, 0] == 1) & np.all(a["act"] == b["act"], axis=1)
            diff = np.max(np.abs(a["x"] - b["x"]), axis=1) / np.maximum(1.0, np.max(np.abs(b["x"]), axis=1))
            rec["shared_vs_resident"] = dict(instances_with_one_active_set_on_both_sides=int(same.sum()),
                                             tx_rel_diff_on_those_max=float(diff[same].max()) if same.any() else None,
                                             tx_rel_diff_on_those_median=float(np.median(diff[same])) if same.any() else None)
        del ts_, tr_, out
    resident_bytes = 8 * copies * (Pu.nnz + A0.nnz + n + 2 * m + (4 + 2 * n + 3 * m) + (n * n if big else 0))
    rec["device_bytes"] = dict(shared_handle_after_the_calls=sb.device_bytes(), resident_data_records_scratch=int(resident_bytes))
    rec["plan"] = batch.shared_plan(lib, P0, A0)
    sb.close(); rb.close()
    return rec


def measure(a):
    _paths()
    import osqp_jl_amd as oq

    lib = oq.load_library()
    base_lib = oq.load_library(a.baseline_lib) if a.baseline_lib else lib
    out = {}
    for kind, shape, seed in SHAPES:
        name = "%s(%s)" % (kind, ", ".join(str(v) for v in shape))
        out[name] = _shape(lib, base_lib, kind, shape, seed, a.copies, a.rounds)
        print(name, json.dumps(out[name]), flush=True)
        _merge(a.out, "shapes", out)
    _merge(a.out, "baseline_library", "the parent commit's build" if a.baseline_lib else "this tree's build (the resident path is the parent's code)")


def nonregression(a):
    _paths()
    import batch_shared as BS

    _merge(a.out, "what", WHAT)
    BS.nonregression(a)
    _merge(a.out, "what", WHAT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    m = sub.add_parser("measure")
    m.add_argument("--copies", type=int, default=4096)
    m.add_argument("--rounds", type=int, default=5)
    m.add_argument("--baseline-lib", default=None)
    m.add_argument("--out", default=DEFAULT_OUT)
    r = sub.add_parser("nonregression")
    r.add_argument("lines")
    r.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    {"measure": measure, "nonregression": nonregression}[a.cmd](a)


if __name__ == "__main__":
    main()
