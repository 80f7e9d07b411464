"""The opt-in batched path for 128 < n <= 256 (osqp_amd_batch_large), on the host: the plan of the
kernel (osqp_amd_batch_large_plan touches no device) against a Python transcription of its LDS layout, the refusals, the
switch, and -- with the oracle alone -- the conditions tests/test_batch_large_gpu.py rests on."""
import numpy as np
import pytest

import osqp_jl_amd as oq
from osqp_jl_amd import batch
import batch_cert_cases as cert
import batch_entry_families as F
import batch_gap_cases as G
import batch_large_cases as L


@pytest.mark.parametrize("i", range(len(L.SHAPES)), ids=L.SHAPE_IDS)
def test_plan_of_the_six_shapes(product_lib, i):
    kind, args, _ = L.SHAPES[i]
    pat = F.pattern(kind, args)
    n, m, nnzA, nnzF = L.pattern_counts(pat)
    plan = batch.large_plan(product_lib, *pat)
    print(L.SHAPE_IDS[i], plan, "nnzA", nnzA, "nnzF", nnzF)
    assert plan["lds_bytes"] <= L.LDS_LIMIT
    assert plan["lds_bytes"] == L.lds_bytes(n, m, nnzA, nnzF)
    assert plan["scratch_bytes"] == 8 * n * n
    assert plan["tiles_per_wave"] == L.tiles_per_wave(n) <= 17


def test_the_cap_needs_seventeen_tiles_and_the_largest_case_145_kb(product_lib):
    assert batch.large_plan(product_lib, *F.pattern("random", (256, 384, 7)))["tiles_per_wave"] == 17
    assert batch.large_plan(product_lib, *F.pattern("banded", (129, 193, 4)))["tiles_per_wave"] == 6
    assert 140 * 1024 < batch.large_plan(product_lib, *F.pattern("banded", (256, 512, 6)))["lds_bytes"] < 150 * 1024


def test_refusals_of_the_plan(product_lib):
    out = np.full(3, -1, dtype=np.int64)
    assert product_lib.osqp_amd_batch_large_plan(257, 300, 1000, 700, out.ctypes.data) != 0
    assert b"256" in product_lib.osqp_amd_last_error()
    assert np.array_equal(out, [-1, -1, -1])
    with pytest.raises(oq.OSQPError, match="256"):
        batch.large_plan(product_lib, *F.banded(257, 385, 4))
    # a dense P at n = 200: 40000 entries of the full P alone are 320 KB
    pat = L.dense_p_pattern(200, 300, 7)
    n, m, nnzA, nnzF = L.pattern_counts(pat)
    assert nnzF == 200 * 200 and L.lds_bytes(n, m, nnzA, nnzF) > L.LDS_LIMIT
    with pytest.raises(oq.OSQPError, match=r"too large for the LDS-resident batched path \(needs %d bytes of LDS\)" % L.lds_bytes(n, m, nnzA, nnzF)):
        batch.large_plan(product_lib, *pat)
    # n <= 128 is not this kernel's
    with pytest.raises(oq.OSQPError, match="128 < n <= 256"):
        batch.large_plan(product_lib, *F.banded(128, 192, 4))


def test_switch_off_refuses_as_before_and_the_switch_returns_the_previous_value(product_lib):
    lib = product_lib
    assert lib.osqp_amd_batch_large(0) == 0  # the default
    args, _ = F.instances(F.pattern("banded", (129, 193, 4)), 2, 3000)
    with pytest.raises(oq.OSQPError, match="the batched path supports n <= 128 and fewer than 65536 rows / non-zeros"):
        batch.solve_batch(lib, *args, **F.OPTS)  # validated on the host: no device is touched
    assert lib.osqp_amd_batch_large(1) == 0
    assert lib.osqp_amd_batch_large(5) == 1
    assert lib.osqp_amd_batch_large(0) == 1
    assert lib.osqp_amd_batch_large(0) == 0
    # solve_batch(large=True) puts the switch back, also when the call is refused (n = 257: on the host, naming 256)
    args, _ = F.instances(F.banded(257, 385, 4), 1, 1)
    with pytest.raises(oq.OSQPError, match="n <= 256"):
        batch.solve_batch(lib, *args, large=True, **F.OPTS)
    assert lib.osqp_amd_batch_large(0) == 0


# ---- the conditions the GPU tests rest on, with the oracle alone -------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(L.SHAPES)), ids=L.SHAPE_IDS)
def test_references_are_solved_and_certified(oracle_lib, i):
    rows = F.reference(L.case(i), oracle_lib)["rows"]
    assert len(rows) == L.COUNT
    print(L.SHAPE_IDS[i], "iterations", [r["iter"] for r in rows])
    for r in rows:
        assert r["status"] == "Solved" and r["certified"], (r["status"], r["certified"])


def test_some_case_refactorises(oracle_lib):
    """A re-factorisation is what the visibility argument of the kernel is about: the references must contain one."""
    updates = {}
    for i in range(len(L.SHAPES)):
        _, probs = F.case_problems(L.case(i), oracle_lib)
        updates[L.SHAPE_IDS[i]] = [int(F.oracle_solve(oracle_lib, p, **F.OPTS).info.rho_updates) for p in probs]
    print(updates)
    assert sum(1 for v in updates.values() if max(v) >= 1) >= 1
    assert max(updates[L.SHAPE_IDS[3]]) >= 1  # at the cap, where the inverse is largest


@pytest.mark.parametrize("n,extra", L.CHAINS)
def test_chain_families_give_the_three_statuses(oracle_lib, n, extra):
    _, probs = L.chain_family(n, extra)
    for opts in cert.VARIANTS:
        res = [F.oracle_solve(oracle_lib, p, **dict(cert.OPTS, **opts)) for p in probs]
        print(n, opts, [(r.info.status_val, r.info.iter) for r in res])
        assert [r.info.status_val for r in res] == [1, -3, -4, 1, -3, -4]
    r = F.oracle_solve(oracle_lib, L.indefinite(n, extra)[0], **L.INDEFINITE_OPTS)
    assert r.info.status_val == -7 and r.info.iter == 50, (r.info.status, r.info.iter)


def test_gap_family_moves_with_a_margin(oracle_lib):
    tr = L.pf_trace(oq, oracle_lib)
    print([(row["K_off"], row["K_on"]) for row in tr])
    assert [(row["K_off"], row["K_on"]) for row in tr] == [(50, 100), (125, 200), (100, 150), (75, 125), (100, 150)]
    for row in tr:
        assert row["status"] == "Solved"
        for k, c in row["checks"].items():
            for name in ("pri", "dua", "gap"):
                assert abs(c[name] - 1.0) > G.MARGIN, (k, name, c[name])
