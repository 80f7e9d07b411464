#!/usr/bin/env python3
"""What the gap stopping rule of the resident batch costs when it is on (osqp_amd_batch_duality_gap_check, DESIGN.md
section 19).

    batch_gap_rule.py cost [--copies N] [--rounds R]
        N copies (default 4096) cycling through the six pf(24, 3) instances of tests/batch_gap_cases.py on one resident
        handle, eps 1e-3, adaptive_rho_interval 25, cold starts (warm_start off, rho reset before every solve): the solve with
        the rule off and on, alternated R times after an untimed solve of each; a host clock around the blocking call with
        device outputs.  Per mode: ms per launch (the median), the instance-iterations of a launch, ms per 1000
        instance-iterations, the refusals.  One JSON line.  A report, not a gate."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cost(args):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import numpy as np

    import osqp_jl_amd as oq
    from osqp_jl_amd import batch
    import batch_gap_cases as cases

    lib = oq.load_library()
    (P, A, Px, Ax, q, l, u), _ = cases.pf_instances("pf24")
    idx = np.arange(args.copies) % Px.shape[0]
    rb = batch.ResidentBatch(lib, P, A, Px[idx], Ax[idx], q[idx], l[idx], u[idx], **dict(cases.SETTINGS, warm_start=False))
    out = (batch.DeviceArray(lib, args.copies, rb.n), batch.DeviceArray(lib, args.copies, rb.m), batch.DeviceArray(lib, args.copies, 6))
    rho = cases.SETTINGS.get("rho", 0.1)

    def run(rule):
        rb.duality_gap_check(rule)
        rb.update_settings(rho=rho)  # every record back to the first rho: each timed solve is the same cold solve
        t0 = time.perf_counter()
        rb.solve(out=out)
        return (time.perf_counter() - t0) * 1e3

    times = {False: [], True: []}
    rec = {}
    for rule in (False, True):
        run(rule)  # untimed
        info = out[2].numpy()
        rec["rule_on" if rule else "rule_off"] = dict(instance_iterations=int(info[:, 0].sum()), solved=int((info[:, 1] == 1).sum()),
                                                      refusals=int(rb.gap_refusals().sum()), kernel=int(lib.osqp_amd_batch_last_kernel()))
    for _ in range(args.rounds):
        for rule in (False, True):
            times[rule].append(run(rule))
    for rule in (False, True):
        r = rec["rule_on" if rule else "rule_off"]
        r["ms_per_launch"] = [round(t, 4) for t in times[rule]]
        r["ms_per_launch_median"] = round(statistics.median(times[rule]), 4)
        r["ms_per_1000_instance_iterations"] = round(r["ms_per_launch_median"] / (r["instance_iterations"] / 1000.0), 6)
    rb.close()
    print(json.dumps(dict(copies=args.copies, family="pf(24, 3)", rounds=args.rounds, **rec)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("cost")
    c.add_argument("--copies", type=int, default=4096)
    c.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    cost(args)


if __name__ == "__main__":
    main()
