"""The conditions on the inputs of test_batch_gap_rule_gpu.py, asserted on the CPU (the oracle plus numpy, batch_gap_cases.py):
where every instance of the portfolio families stops with the gap rule off and on, with the margins that let the GPU tests
demand exact iteration counts, which kernel takes each family, and that the rule moves no instance of the families on which
rule on and rule off must agree bit for bit.  The table in DESIGN.md section 19 is what test_the_table prints."""
import numpy as np
import pytest

import osqp_jl_amd as oq
import batch_entry_families as fam
import batch_gap_cases as cases

# K_off -> K_on per instance
TABLE = {
    "pf16": [(75, 75), (50, 50), (50, 50), (50, 50), (50, 75), (50, 50), (50, 50), (50, 75)],
    "pf24": [(50, 50), (75, 100), (50, 50), (75, 75), (50, 75), (50, 50)],
    "pf60": [(75, 100), (75, 75), (50, 75), (75, 75), (50, 75), (75, 75)],
    "pf12": [(50, 50), (50, 75), (50, 50), (50, 75)],
}


def _print(name, tr):
    for i, row in enumerate(tr):
        line = ", ".join("%d: %.3f %.3f %.3f" % (k, c["pri"], c["dua"], c["gap"]) for k, c in sorted(row["checks"].items()))
        print(f"{name} inst {i}: {row['status']} K_off {row['K_off']} K_on {row['K_on']} | k: pri dua gap | {line}")


@pytest.mark.parametrize("name", list(cases.PF))
def test_the_table(oracle_lib, name):
    tr = cases.rule_trace_batch(oq, oracle_lib, name)
    _print(name, tr)
    assert [(r["K_off"], r["K_on"]) for r in tr] == TABLE[name]


# every family under the settings of test 1; pf(24, 3) also under the two variants of the life-cycle test
RUNS = [(name, dict()) for name in cases.PF] + [("pf24", dict(scaling=0)), ("pf24", dict(scaled_termination=1))]


@pytest.mark.parametrize("name,extra", RUNS, ids=["%s%s" % (n, "".join("-%s%d" % kv for kv in e.items())) for n, e in RUNS])
def test_conditions_on_the_portfolio_families(oracle_lib, name, extra):
    tr = cases.rule_trace_batch(oq, oracle_lib, name, **extra)
    _print(name, tr)
    moved = 0
    for i, row in enumerate(tr):
        assert row["status"] == "Solved" and row["K_off"] % cases.CHECK == 0, (i, row["status"], row["K_off"])
        assert row["K_on"] is not None, i
        for k, c in row["checks"].items():
            for key in ("pri", "dua", "gap"):
                assert abs(c[key] - 1.0) > cases.MARGIN, (i, k, key, c[key])
            if k < row["K_off"]:  # the residuals alone keep it going: K_off is where the kernels' own checks end too
                assert max(c["pri"], c["dua"]) > 1.0, (i, k)
            else:
                assert c["pri"] < 1.0 and c["dua"] < 1.0, (i, k, c["pri"], c["dua"])
                assert (c["gap"] < 1.0) == (k == row["K_on"]), (i, k, c["gap"])
        moved += row["K_on"] > row["K_off"]
    if not extra:
        assert moved >= 2 and len(tr) - moved >= 2, moved
    else:
        assert moved >= 1 and len(tr) - moved >= 1, moved


def test_which_kernel_takes_each_family():
    for name, (n, k, count, entry) in cases.PF.items():
        args, probs = cases.pf_instances(name)
        assert len(probs) == count and args[4].shape == (count, n + k) and args[5].shape == (count, n + k + 1)
        assert fam.predict(cases.pattern_of(args))["entry"] == entry, name
    # the entries test 2 forces: the run-time-shaped narrow entries and entry 4 for pf(16, 2) (entry 10 does not take it: the
    # sum row has 16 entries, its bound is 12 -- pf(12, 2) is there for entry 10), the wide ones for pf(24, 3)
    assert cases.forced_entries("pf16") == [1, 2, 3, 4, 5] and cases.forced_entries("pf24") == [6, 7, 8, 9]
    assert cases.forced_entries("pf12") == [10]


@pytest.mark.parametrize("name", cases.FIXED)
def test_the_rule_moves_no_instance_of_the_fixed_families(oracle_lib, name):
    tr = cases.rule_trace_batch(oq, oracle_lib, name)
    _print(name, tr)
    for i, row in enumerate(tr):
        assert row["status"] == "Solved" and row["K_on"] == row["K_off"], (i, row["status"], row["K_off"], row["K_on"])
        assert row["checks"][row["K_off"]]["gap"] < 0.5, (i, row["checks"][row["K_off"]]["gap"])


def test_the_approximate_pass_cases(oracle_lib):
    """The first limit (one iteration before K_on) is the issue's; the CPU procedure finds the gap already below its bound
    there.  The second (one iteration after K_off) is where the approximate pass decides."""
    name, inst = cases.APPROX
    row = cases.rule_trace_batch(oq, oracle_lib, name)[inst]
    assert row["K_on"] > row["K_off"]
    verdicts = []
    for limit in cases.approximate_limits(row):
        status, exact, approx = cases.approximate_verdict(oq, oracle_lib, name, inst, limit)
        print(limit, status, "ratios at eps", exact, "at 10 eps", approx)
        for v in exact + approx:
            assert abs(v - 1.0) > cases.MARGIN, (limit, exact, approx)
        verdicts.append(status)
    assert verdicts[1] in ("Solved_inaccurate", "Max_iter_reached"), verdicts
