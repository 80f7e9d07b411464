"""Every instantiation of the four-wavefront kernel of the batched path (OQ_QUAD_ENTRIES in csrc/batch_common.hpp) and every
branch of its host schedule, at the smallest shapes that reach them: n = 2 NH, 2 NH - 1, NH + 1 and NH per quadrant size,
the two-ended first phase with both ends and at its caps, random patterns with the phase off, a longest row or column above
the narrow entries' bounds and exactly at the wide ones', all 256 row lanes, the try order, the fall-through to the 512-thread
kernel, batches of one and of seven.  The cases and their host side are tests/batch_entry_families.py;
tests/test_batch_entries_host.py checks on the host what the bounds used here rest on.

Per case: (a) the branch that ran is the intended one -- the device's own report of its schedule
(osqp_amd_batch_last_schedule) equals the transcription of the host schedule number by number, so a silent fall-through to a
neighbouring entry fails; (b) statuses and (c) iteration counts are the oracle's (within one check); (d) the returned point
meets OSQP's stopping rule re-evaluated from the raw data, within the factor 2 test_large_property_checks uses; (e) its
distance to the exact optimum is at most twice the oracle's own at its last or its previous check.

With OSQP_AMD_ENTRIES_RECORD=<file> every case adds its figures to that JSON file (the way to write
profiles/r10_batch_entries.json); by default nothing is written."""
import json
import os

import numpy as np
import pytest

import osqp_jl_amd as oq
from osqp_jl_amd import batch
import batch_entry_families as F

pytestmark = pytest.mark.gpu

SCHEDULE_KEYS = ("p1_top", "p1_bot", "bw", "ns", "kew", "lds_bytes")


def _dump(cid, rec):
    path = os.environ.get("OSQP_AMD_ENTRIES_RECORD")
    print(cid, json.dumps(rec))
    if not path:
        return
    allrec = json.load(open(path)) if os.path.exists(path) else {}
    allrec[cid] = rec
    with open(path, "w") as f:
        json.dump(allrec, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.mark.parametrize("cid", F.CASE_IDS)
def test_entry_case(product_lib, oracle_lib, monkeypatch, cid):
    case = F.CASES[F.CASE_IDS.index(cid)]
    ref = F.reference(case, oracle_lib)
    opts, rows, probs = case["opts"], ref["rows"], ref["probs"]
    pat = F._finish(ref["args"][0], ref["args"][1])
    pred = F.predict(pat, -1 if case["force"] is None else case["force"])
    if case["force"] is None:
        monkeypatch.delenv("OSQP_AMD_BATCH_QUAD_CFG", raising=False)
    else:
        monkeypatch.setenv("OSQP_AMD_BATCH_QUAD_CFG", str(case["force"]))
    if case["refused"]:  # beyond the batched path: a loud error, no launch, no other kernel in its place
        with pytest.raises(oq.OSQPError, match=case["refused"]):
            batch.solve_batch(product_lib, *ref["args"], **opts)
        return
    x, y, info = batch.solve_batch(product_lib, *ref["args"], **opts)
    sched = batch.last_schedule(product_lib)

    # the figures first, then the record, then the assertions: a failing case leaves its numbers behind
    iter_diff = [int(abs(info[i, 0] - r["iter"])) for i, r in enumerate(rows)]
    ratios = [F.criteria_ratios(*probs[i], x[i], y[i], opts["eps_abs"], opts["eps_rel"]) for i in range(len(rows))]
    e_K = [(F.rel_err(x[i], r["xs"]), F.rel_err(y[i], r["ys"])) for i, r in enumerate(rows)]
    bound = [tuple(max(r["e_O"][k], r["e_O1"][k]) for k in (0, 1)) for r in rows]
    over = [tuple(e_K[i][k] / bound[i][k] for k in (0, 1)) for i in range(len(rows))]
    rec = dict(entry=sched["entry"], expected_entry=case["expect"], forced=case["force"], n=case["n"], m=case["m"], instances=sched["instances"],
               tight=case["tight"], predicted={k: pred.get(k) for k in SCHEDULE_KEYS}, measured={k: sched[k] for k in SCHEDULE_KEYS},
               lds_bytes=sched["lds_bytes"], statuses=[int(v) for v in info[:, 1]], worst_iter_diff=max(iter_diff),
               worst_criteria_ratios=[float(np.nanmax([r[k] for r in ratios])) for k in (0, 1)],
               worst_eK_over_bound=dict(x=float(np.nanmax([o[0] for o in over])), y=float(np.nanmax([o[1] for o in over]))))
    _dump(cid, rec)

    # (a) the branch
    assert sched["entry"] == case["expect"], sched
    assert sched["instances"] == case["count"] == len(rows), sched
    if case["expect"] >= 0:
        NH = F.entry(case["expect"])[1]
        assert sched["lds_bytes"] <= F.LDS_LIMIT, sched
        if case["phase"] == "on":
            assert sched["p1_top"] + sched["p1_bot"] >= 8, sched
            if case["n"] >= NH + 8:
                assert sched["p1_bot"] > 0, sched
        elif case["phase"] == "off":
            assert sched["p1_top"] == 0 and sched["p1_bot"] == 0, sched
        if case["full_lanes"]:
            assert min(sched["kew"]) > 0, sched
        assert {k: sched[k] for k in SCHEDULE_KEYS} == {k: pred[k] for k in SCHEDULE_KEYS}, (sched, pred)
    for i, r in enumerate(rows):
        # (b) status, (c) iterations: the oracle's
        assert r["status"] == "Solved" and int(info[i, 1]) == r["status_val"], (i, info[i, :2], r["status"])
        assert iter_diff[i] <= F.CHECK, (i, info[i, 0], r["iter"])
        # (d) the stopping rule, re-evaluated
        assert max(ratios[i]) <= 2.0, (i, ratios[i])
        # (e) against the exact optimum: within twice the oracle's own error at its last or its previous check
        assert r["certified"]
        assert e_K[i][0] <= 2.0 * bound[i][0], (i, "x", e_K[i][0], bound[i][0])
        assert e_K[i][1] <= 2.0 * bound[i][1], (i, "y", e_K[i][1], bound[i][1])
