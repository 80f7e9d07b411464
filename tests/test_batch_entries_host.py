"""The case list of the entry tests of the batched path (tests/batch_entry_families.py), checked on the host: every
run-time-shaped row of the kernel table has its cases, every pattern has the structural property its case is named for, and
every instance meets the conditions the GPU test (tests/test_batch_entries_gpu.py) builds its bounds on -- the oracle ends
Solved well inside its iteration limit, the exact optimum certifies, the oracle's own point meets the stopping rule as the
test re-evaluates it, and the oracle's own error against the optimum is far above rounding level."""
import numpy as np
import pytest
import scipy.sparse as sp

import batch_entry_families as F


def _pattern(case, oracle_lib):
    if case["kind"] == "mpc":
        P0, A0 = F.case_problems(case, oracle_lib)[0][:2]
        return F._finish(P0, A0)
    return F.pattern(case["kind"], case["args"])


def test_table_parses_to_the_rows_of_the_header():
    rows = F.table()
    assert len(rows) == len({r[0] for r in rows}) >= 11
    assert rows[0] == (0, 50, 9, 11, 16, True, "k_batch_quad") and sum(r[5] for r in rows) == 1
    order = [r[0] for r in rows]
    assert order.index(10) < order.index(4)  # the three-per-unit layout of the MPC sizes is tried before the two-per-unit one
    for num, NH, KC, KE, CH, fixed, kernel in rows:
        assert 1 <= NH <= 64 and KC <= 32 and KE <= 32 and CH == 16 and kernel in ("k_batch_quad", "k_batch_quad2")


def test_every_run_time_shaped_row_has_cases():
    """A row added to the table without cases fails here."""
    for num, NH, KC, KE, CH, fixed, _ in F.table():
        mine = [c for c in F.CASES if c["expect"] == num]
        assert mine, "table row %d has no cases" % num
        assert sum(c["tight"] for c in mine) >= 1, num
        if fixed:
            continue
        assert num in F.FAMILY, "table row %d has no family of shapes" % num
        forced = [c for c in mine if c["force"] == num]
        assert {c["n"] for c in forced} >= {2 * NH, 2 * NH - 1, NH + 1, NH}, num
        tight = [c for c in mine if c["tight"]]
        assert all(c["n"] == 2 * NH and c["opts"]["eps_abs"] == 1e-8 and c["opts"]["max_iter"] == 8000 for c in tight)
        assert any(c["phase"] == "on" and c["n"] >= NH + 8 for c in forced), num  # both ends of the first phase, at this quadrant size
        if F.FAMILY[num] == "narrow":
            assert any(c["kind"] == "random" and c["phase"] == "off" for c in forced), num
        elif F.FAMILY[num] == "wide":
            assert any(c["exceeds"] >= 16 and c["n"] == n for n in (2 * NH, 2 * NH - 1, NH + 1, NH) for c in forced), num
    assert {c["count"] for c in F.CASES} >= {1, 6, 7}
    assert all(c["count"] == 6 for c in F.CASES if not c["id"].startswith("count"))


@pytest.mark.parametrize("cid", F.CASE_IDS)
def test_case_pattern_has_the_property_it_is_named_for(oracle_lib, cid):
    case = F.CASES[F.CASE_IDS.index(cid)]
    pat = _pattern(case, oracle_lib)
    pat_P, pat_A = pat
    n, m = pat_A.shape[1], pat_A.shape[0]
    assert (n, m) == (case["n"], case["m"])
    assert np.all(pat_P.diagonal() == 1.0) and sp.tril(pat_P, -1).nnz == 0  # an upper triangle with a full diagonal
    col, row = F.longest(pat_A)
    if case["exceeds"]:
        assert max(col, row) > case["exceeds"], (col, row)
    pred = F.predict(pat, -1 if case["force"] is None else case["force"])
    if case["expect"] < 0:
        assert n > 128 or m > 256 or max(col, row) > 32, (n, m, col, row)
        assert pred["entry"] == -1, pred
        return
    num, NH, KC, KE, CH, fixed, _ = F.entry(case["expect"])
    assert col <= KC and row <= KE and n <= 2 * NH and m <= 256, (col, row, n, m)
    if case["kind"] == "spiked":
        want_row, want_col = case["args"][3], case["args"][4]
        assert (row == min(want_row, n) if want_row else row <= 5) and (col == min(want_col, m) if want_col else col <= 8), (col, row)
    # the transcribed schedule takes the entry the case is for: unforced cases rest on the try order
    assert pred["entry"] == case["expect"], pred
    assert pred["lds_bytes"] <= F.LDS_LIMIT
    if case["phase"] == "on":
        assert pred["p1_top"] + pred["p1_bot"] >= 8, pred
        if n >= NH + 8:
            assert pred["p1_bot"] > 0, pred
    elif case["phase"] == "off":
        assert pred["p1_top"] == 0 and pred["p1_bot"] == 0, pred
    if case["full_lanes"]:
        assert m == 256 and min(pred["kew"]) > 0, pred


def test_first_phases_the_transcription_gives():
    """The first phases of the first n = 2 NH case of each entry: both ends, and the caps (nb - 1) * 16 at quadrants of 32,
    48 and 64."""
    want = {1: (13, 13), 2: (16, 16), 7: (16, 16), 3: (32, 32), 8: (32, 32), 10: (47, 47), 4: (44, 44), 5: (48, 48), 9: (48, 48)}
    for num, p1 in want.items():
        case = next(c for c in F.CASES if c["expect"] == num and c["n"] == 2 * F.entry(num)[1] and not c["tight"])
        pred = F.predict(F.pattern(case["kind"], case["args"]), -1 if case["force"] is None else case["force"])
        assert (pred["p1_top"], pred["p1_bot"]) == p1, (num, pred)


def test_lds_limit_inside_the_nominal_range():
    """Where the 80 KB limit bites although n, m, columns and rows are within an entry's bounds: the wide entries refuse
    n = 2 NH with m = 256 and rows of 6, 9 and 12 entries at quadrants of 32, 48 and 64 (85 to 105 KB), and entry 9 holds
    the banded n = 128, m = 192 with 304 bytes to spare (the case e9-banded-n128-m192 runs it).  A change of the layout moves
    these edges and fails here."""
    for num, w, total in ((7, 6, 85776), (8, 9, 95504), (9, 12, 105232)):
        NH = F.entry(num)[1]
        pat = F.banded(2 * NH, 256, w)
        assert max(F.longest(pat[1])) <= 32
        pred = F.predict(pat, num)
        assert pred["entry"] == -1 and pred["refused"][num] == "LDS bytes (%d)" % total, pred
    pred = F.predict(F.banded(128, 192, 4), 9)
    assert pred["entry"] == 9 and F.LDS_LIMIT - pred["lds_bytes"] == 304, pred


@pytest.mark.parametrize("cid", F.CASE_IDS)
def test_conditions_on_the_inputs(oracle_lib, cid):
    """What the bounds of the GPU test rest on, on every instance of the case, with nothing left out."""
    case = F.CASES[F.CASE_IDS.index(cid)]
    ref = F.reference(case, oracle_lib)
    opts = case["opts"]
    assert len(ref["rows"]) == case["count"]
    for i, row in enumerate(ref["rows"]):
        assert row["status"] == "Solved" and row["iter"] <= opts["max_iter"] // 2, (i, row["status"], row["iter"])
        assert row["certified"], i
        assert max(row["ratios"]) <= 1.0, (i, row["ratios"])
        # the bound e_K <= 2 max(e_O, e_O') never degenerates to rounding level: at eps 1e-5 the oracle's own error is at least
        # 1e-9; at 1e-8 the larger of the two the bound takes is
        floor = [max(row["e_O"][k], row["e_O1"][k]) for k in (0, 1)] if case["tight"] else row["e_O"]
        assert min(floor) >= 1e-9, (i, row["e_O"], row["e_O1"])
