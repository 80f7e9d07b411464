#!/usr/bin/env python3
"""Bit digests of the direct back-end over every (form, structure) pair of tests/test_kkt_reference_gpu.py's CASES (the table
is imported, not copied): per pair the form's environment, a setup with linsys_solver="direct", one KKT solve
(osqp_amd_apply, op 3) of a fixed right-hand side before and after update_settings(rho=0.731), twenty ADMM iterations, and a
SHA-256 of each output plus the statistics.  The library is the one OSQP_AMD_LIB names, so one checkout runs two builds.

usage: python tools/direct_forms_digest.py                  one JSON line per pair, for the library in use
       python tools/direct_forms_digest.py --compare A B    both libraries in fresh child processes; exit 1 on any difference
       python tools/direct_forms_digest.py --mark           the same, with one torch kernel launched before every pair: a marker
              that no kernel of the library or of the HIP runtime can be taken for (namespace at::), for a run under a kernel trace
       python tools/direct_forms_digest.py --dispatches A.db B.db A.jsonl B.jsonl
              the kernel dispatch sequences (name, grid, workgroup, LDS, in time order) of two rocpd databases, each written
              by `rocprofv3 --kernel-trace -d DIR -o NAME -- python tools/direct_forms_digest.py --mark > A.jsonl` (a run of its
              own: no counters, no other tracing), and the dispatches of every pair: split at the markers, or, where the trace
              does not hold torch's kernels, at the times the run noted when each pair began"""
import ctypes as C
import hashlib
import json
import os
import sqlite3
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _sha(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


def run(mark=False):
    import numpy as np
    import osqp_jl_amd as oq
    import test_kkt_reference_gpu as t

    lib = oq.load_library()
    fptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    form_keys = sorted({k for env, _, _ in t.FORMS.values() for k in env})
    if mark:
        import torch
        marker = torch.zeros(1, device="cuda")
    for form, structure in t.CASES:
        # when the pair begins, on the clocks a profiler may stamp dispatches with (the device is idle here: every call before returned synchronised)
        began = {"boottime": time.clock_gettime_ns(time.CLOCK_BOOTTIME), "monotonic": time.clock_gettime_ns(time.CLOCK_MONOTONIC), "realtime": time.time_ns()}
        if mark:
            marker.add_(1.0)
            torch.cuda.synchronize()
        for k in form_keys:
            os.environ.pop(k, None)
        os.environ.update(t.FORMS[form][0])
        prob = t.STRUCTURES[structure]()
        N = prob["P"].shape[0] + prob["A"].shape[0]
        rhs = np.cos(0.37 * np.arange(N) + 0.11)
        m = oq.Model(lib)
        oq.setup(m, linsys_solver="direct", verbose=False, adaptive_rho=False, max_iter=20, check_termination=0, **prob)
        out = {"form": form, "structure": structure, "N": N}
        out["began_ns"] = began
        for tag in ("solve", "solve_after_rho"):
            x = np.empty(N)
            assert lib.osqp_amd_apply(m.workspace, 3, fptr(rhs), fptr(x)) == 0
            out[tag] = _sha(x)
            if tag == "solve":
                oq.update_settings(m, rho=0.731)
        r = oq.solve(m)  # (stops at max_iter: the iterates are read from the workspace whatever the status)
        sol, dat = m.workspace.contents.solution.contents, m.workspace.contents.data.contents
        x, y = np.empty(int(dat.n)), np.empty(int(dat.m))
        C.memmove(x.ctypes.data, sol.x, 8 * x.size)
        C.memmove(y.ctypes.data, sol.y, 8 * y.size)
        out["x20"], out["y20"], out["iter"], out["status"] = _sha(x), _sha(y), int(r.info.iter), r.info.status
        out["residuals"] = [float(r.info.pri_res).hex(), float(r.info.dua_res).hex()]
        st = np.asarray(oq.stats(m), dtype=np.float64)
        keep = [i for i in range(st.size) if i not in (9, 20, 24)]  # (device bytes, their peak, reserved address space: the allocator's)
        out["stats"] = [float(v) for v in st[keep]]
        oq.clean(m)
        print(json.dumps(out), flush=True)


def compare(libs):
    runs = []
    for lib in libs:
        p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, OSQP_AMD_LIB=os.path.abspath(lib)),
                           stdout=subprocess.PIPE, text=True, check=True)
        runs.append([json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")])
        for d in runs[-1]:
            del d["began_ns"]
    a, b = runs
    bad = [(x["form"], x["structure"]) for x, y in zip(a, b) if x != y]
    print(json.dumps({"pairs": len(a), "pairs_second": len(b), "differing": bad, "digests": a}))
    return 1 if bad or len(a) != len(b) or not a else 0


def _dispatches(db):
    c = sqlite3.connect(db)
    tables = [r[0] for r in c.execute("select name from sqlite_master where type in ('table', 'view')")]
    disp = next(n for n in tables if n.startswith("rocpd_kernel_dispatch"))
    sym = next(n for n in tables if n.startswith("rocpd_info_kernel_symbol"))
    cols = [r[1] for r in c.execute("pragma table_info(%s)" % disp)]
    def pick(*names):
        found = [n for n in names if n in cols]
        if not found:
            raise SystemExit("%s: none of the columns %s in %s" % (db, names, disp))
        return "d." + found[0]
    q = "select d.start, s.kernel_name, %s, %s, %s, %s, %s, %s, d.group_segment_size from %s d join %s s on d.kernel_id = s.id order by d.start" % (
        pick("grid_size_x", "grid_x"), pick("grid_size_y", "grid_y"), pick("grid_size_z", "grid_z"),
        pick("workgroup_size_x", "workgroup_x"), pick("workgroup_size_y", "workgroup_y"), pick("workgroup_size_z", "workgroup_z"), disp, sym)
    return [tuple(r) for r in c.execute(q)]


def _per_pair(seq, run, ncases):
    """Dispatches of every pair: split at the torch markers (namespace at::) where the trace holds them, else at the times the
    tool noted when each pair began, on whichever of its clocks the trace's stamps turn out to be."""
    per, in_marker = [], True
    for _, name, *_ in seq:
        if "at::" in name:
            in_marker = True
            continue
        if in_marker:
            per.append(0)
            in_marker = False
        per[-1] += 1
    if len(per) == ncases:
        return per, "markers"
    began = [json.loads(l)["began_ns"] for l in open(run) if l.startswith("{")]
    for clock in ("boottime", "monotonic", "realtime"):
        t = [b[clock] for b in began]
        if len(t) == ncases and abs(seq[0][0] - t[0]) < 60e9 and 0 <= seq[-1][0] - t[-1] < 600e9:
            per = [0] * ncases
            k = 0
            for start, *_ in seq:
                if start < t[0]:
                    continue  # (before the first pair: the marker tensor's creation)
                while k + 1 < ncases and start >= t[k + 1]:
                    k += 1
                per[k] += 1
            return per, clock
    raise SystemExit("no way to delimit the pairs: %d marked stretches for %d pairs, first dispatch at %d, pairs began at %s" % (len(per), ncases, seq[0][0], began[:1]))


def dispatches(dbs, runs):
    import test_kkt_reference_gpu as t
    a, b = (_dispatches(d) for d in dbs)
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x[1:] != y[1:]), None)
    same = len(a) == len(b) and first is None
    out = {"dispatches": [len(a), len(b)], "same_sequence": same}
    if not same:
        out["first_difference"] = {"index": first, "a": a[first] if first is not None else None, "b": b[first] if first is not None else None}
    (pa, how), (pb, _) = (_per_pair(seq, run, len(t.CASES)) for seq, run in zip((a, b), runs))
    out["per_pair"] = {"%s/%s" % c: [pa[k], pb[k]] for k, c in enumerate(t.CASES)}
    out["per_pair_equal"], out["pairs_delimited_by"] = pa == pb, how
    print(json.dumps(out))
    return 0 if same and pa == pb else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2:]))
    if len(sys.argv) == 6 and sys.argv[1] == "--dispatches":
        sys.exit(dispatches(sys.argv[2:4], sys.argv[4:6]))
    run(mark=sys.argv[1:] == ["--mark"])
