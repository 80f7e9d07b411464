#!/usr/bin/env python
"""Measurements behind profiles/spmv_stream_before_after.json: the panel product of rand-1e6 under the OSQP_AMD_SELL_*
switches of csrc/panel.hip, against another build of the library (the parent commit, checked out and built in a tree of
its own).

    spmv_stream_measure.py kernels --root TREE            one process: build rand-1e6 from TREE's library, print one JSON
                                                          line with the layout (slices, padded, nnz of A, A', P) and
                                                          osqp_amd_time_kernel(ws, which, 20) for which = 0, 1, 2
    spmv_stream_measure.py switches --out FILE            three alternating rounds of `kernels` on this tree with every
                                                          switch on, each one off in turn, and all off
                                                          [--parent TREE: the parent's `kernels` before and after]
    spmv_stream_measure.py bench --parent TREE --out FILE `python bench.py` (defaults) from the parent and from this tree,
                                                          alternating, --pairs times; then --dump-outputs of rand-1e6 and
                                                          rand-1e5 from both and whether x.npy / y.npy are array_equal
                                                          [--bench-args ...: the pairs only, with these arguments]
    spmv_stream_measure.py traffic --parent TREE --out FILE  fetched / written bytes per product (bench.live_traffic: two
                                                          rocprofv3 --pmc passes, a run of their own) for both trees

Every child runs under a time limit of its own, and the first one that fails ends the run: nothing more is started on the
device after a failure."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the switches of this build; the record's rounds 1 and 2 were taken on a build that also had OSQP_AMD_SELL_MASK and
# OSQP_AMD_SELL_AHEAD (--switches names whatever a build has)
SWITCHES = ("OSQP_AMD_SELL_NT",)


def kernels(root):
    sys.path.insert(0, root)
    import bench
    import osqp_jl_amd as oq

    lib = oq.load_library()
    assert lib.osqp_amd_set_device(0) == 0
    model, _, setup_s = bench.build_model(oq, lib, "rand-1e6", 1)
    rec = {"root": root, "setup_s": round(setup_s, 3), "switches": {k: os.environ.get(k) for k in SWITCHES if k in os.environ}}
    rec["layout"] = {name: {k: oq.spmv_layout(model, which)[k] for k in ("slices", "padded", "nnz", "tiles", "Gp", "NG")}
                     for which, name in enumerate(("A", "At", "P"))}
    rec["ms"] = {name: round(float(lib.osqp_amd_time_kernel(model.workspace, which, 20)), 5) for which, name in enumerate(("A", "At", "P"))}
    oq.clean(model)
    print("RECORD " + json.dumps(rec))


def child(cmd, env=None, limit=240, cwd=None):
    e = dict(os.environ)
    for k in SWITCHES:
        e.pop(k, None)
    e.update(env or {})
    p = subprocess.run(cmd, env=e, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit)
    if p.returncode != 0:
        sys.stderr.write(p.stdout.decode()[-2000:] + p.stderr.decode()[-4000:])
        raise SystemExit("child failed with %d: %s" % (p.returncode, " ".join(cmd)))
    return p.stdout.decode()


def kernels_child(root, env=None):
    out = child([sys.executable, os.path.abspath(__file__), "kernels", "--root", root], env)
    return json.loads([l for l in out.splitlines() if l.startswith("RECORD ")][-1][7:])


def save(path, rec):
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


def switches(args):
    off = {k: "0" for k in args.switches}
    if args.alone:  # each switch alone on against all off (the switches interact: round 1 of the record)
        configs = [("all_off", off)] + [(k[9:].lower() + "_only", {j: v for j, v in off.items() if j != k}) for k in args.switches]
    else:
        configs = [("all_on", {})] + [(k[9:].lower() + "_off", {k: "0"}) for k in args.switches] + [("all_off", off)]
    rec = {"rounds": [], "parent": []}
    if args.parent:
        rec["parent"].append(kernels_child(args.parent))
        save(args.out, rec)
    for _ in range(3):
        rnd = {}
        for name, env in configs:
            rnd[name] = kernels_child(HERE, env)
            print(name, rnd[name]["ms"], flush=True)
            rec["rounds"].append({name: rnd[name]})
            save(args.out, rec)
    if args.parent:
        rec["parent"].append(kernels_child(args.parent))
    save(args.out, rec)


def bench_line(root, extra=()):
    out = child([sys.executable, os.path.join(root, "bench.py")] + list(extra), cwd=root, limit=420)
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def bench(args):
    import numpy as np

    rec = {"parent_ms_per_step": [], "new_ms_per_step": [], "cg_iters_per_admm_iter": [], "outputs_equal": {}}
    for _ in range(args.pairs):
        for name, root in (("parent", args.parent), ("new", HERE)):
            line = bench_line(root, args.bench_args)
            rec[name + "_ms_per_step"].append(line["ms_per_step"])
            rec["cg_iters_per_admm_iter"].append(line["cg_iters_per_admm_iter"])
            print(name, line["ms_per_step"], flush=True)
            save(args.out, rec)
    with tempfile.TemporaryDirectory() as tmp:
        for workload in () if args.bench_args else ("rand-1e6", "rand-1e5"):
            dirs = {}
            for name, root in (("parent", args.parent), ("new", HERE)):
                dirs[name] = os.path.join(tmp, workload + "_" + name)
                bench_line(root, ["--workload", workload, "--no-cpu", "--dump-outputs", dirs[name]])
            rec["outputs_equal"][workload] = {v: bool(np.array_equal(np.load(os.path.join(dirs["parent"], v + ".npy")),
                                                                     np.load(os.path.join(dirs["new"], v + ".npy")))) for v in ("x", "y")}
            print(workload, rec["outputs_equal"][workload], flush=True)
            save(args.out, rec)


def traffic(args):
    rec = {}
    for name, root in (("parent", args.parent), ("new", HERE)):
        code = ("import sys, json; sys.path.insert(0, %r); import bench; a = bench.parse_args(['--workload', 'rand-1e6', '--no-cpu']); "
                "print('RECORD ' + json.dumps(bench.live_traffic(a, ['k_spmv_sell', 'k_panel_reduce'])))" % root)
        out = child([sys.executable, "-c", code], cwd=root, limit=600)
        rec[name] = json.loads([l for l in out.splitlines() if l.startswith("RECORD ")][-1][7:])
        print(name, rec[name], flush=True)
        save(args.out, rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "switches", "bench", "traffic"])
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--switches", nargs="*", default=list(SWITCHES))
    ap.add_argument("--alone", action="store_true")
    ap.add_argument("--bench-args", nargs=argparse.REMAINDER, default=[], help="bench: run bench.py with these instead of its defaults (pairs only)")
    a = ap.parse_args()
    if a.what == "kernels":
        kernels(os.path.abspath(a.root))
    else:
        a.parent = os.path.abspath(a.parent) if a.parent else None
        {"switches": switches, "bench": bench, "traffic": traffic}[a.what](a)
