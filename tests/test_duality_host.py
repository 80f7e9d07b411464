"""Dual objective, duality gap and the gap stopping rule without a GPU: the numpy statement of the
definitions (duality_ref.py) on hand-built rows, strong duality at the oracle's accurate solutions, and the conditions on
the cases the GPU test of the rule runs on -- where the residual tests pass, where the gap first passes, and that no gap
ratio sits close enough to 1 for rounding to move a decision.  The oracle and numpy only."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_jl_amd as oq
from osqp_jl_amd import batch, interface
from osqp_jl_amd import types as T
import duality_cases
import duality_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = (("osqp_amd_duality_gap_check", 2), ("osqp_amd_duality", 3), ("osqp_amd_batch_duality", 3), ("osqp_amd_batch_duality_rows", 5))


def test_the_header_declares_and_the_library_exports_the_symbols(product_lib):
    text = open(os.path.join(ROOT, "include", "osqp_amd.h")).read()
    for name, nargs in SYMBOLS:
        assert re.search(r"c_int\s+" + name + r"\s*\(", text), name
        res, args = T.EXT_SYMBOLS[name]
        assert res is T.c_int and len(args) == nargs
        fn = getattr(product_lib, name)  # AttributeError: not exported
        assert fn.restype is T.c_int and list(fn.argtypes or []) == list(args)
    assert re.search(r"#define\s+OSQP_AMD_DUALITY_COUNT\s+6\b", text)
    assert interface.DUALITY_FIELDS == ("prim_obj", "dual_obj", "gap", "eps_gap", "rule", "gap_refusals")
    assert oq.duality is interface.duality and oq.duality_gap_check is interface.duality_gap_check
    assert callable(batch.ResidentBatch.duality)
    import ctypes as C  # both struct layouts stay frozen
    assert C.sizeof(T.Settings) == 176 and C.sizeof(T.CInfo) == 136


def test_null_handles_without_a_device(product_lib):
    buf = np.full(6, np.nan)
    assert product_lib.osqp_amd_duality_gap_check(None, 1) == 7 and b"workspace" in product_lib.osqp_amd_last_error()
    assert product_lib.osqp_amd_duality(None, buf.ctypes.data_as(T.c_float_p), 6) == 7 and np.all(np.isnan(buf))
    assert product_lib.osqp_amd_batch_duality(None, buf.ctypes.data, 0) == 1
    assert product_lib.osqp_amd_batch_duality_rows(None, None, 1, buf.ctypes.data, 0) == 1


def test_a_library_without_the_symbols_raises(oracle_lib):
    prob = duality_cases.VALUE_CASES["unconstrained"]()
    m = oq.Model(oracle_lib)
    oq.setup(m, **prob, verbose=False)
    for call in (lambda: oq.duality_gap_check(m), lambda: oq.duality(m)):
        with pytest.raises(oq.OSQPError, match="does not export"):
            call()
    with pytest.raises(ValueError, match="on"):
        oq.duality_gap_check(m, 1)
    oq.clean(m)


def test_projection_on_each_bound_kind():
    inf = np.inf
    l = np.array([-inf, -inf, -1.0, -2.0, -1e30, -1e30, -3.0])
    u = np.array([inf, 2.0, inf, 3.0, 1e30, 5.0, 1e30])
    for y in (np.array([1.5, 1.5, 1.5, 1.5, 1.5, 1.5, 1.5]), -np.array([1.5, 1.5, 1.5, 1.5, 1.5, 1.5, 1.5])):
        keep = y.copy()
        yh = duality_ref.project(y, l, u)
        assert np.array_equal(y, keep)  # y itself is not modified
        pos = y[0] > 0
        # both infinite: 0; only l infinite: max(y, 0); only u infinite: min(y, 0); both finite: y
        assert yh[0] == 0.0 and yh[4] == 0.0
        assert yh[1] == (1.5 if pos else 0.0) and yh[5] == (1.5 if pos else 0.0)
        assert yh[2] == (0.0 if pos else -1.5) and yh[6] == (0.0 if pos else -1.5)
        assert yh[3] == y[3]
    # SC: u yh+ + l yh-, an infinite bound contributes 0
    P, q, A = sp.csc_matrix((1, 1)), np.zeros(1), sp.csc_matrix((7, 1))
    y = np.array([4.0, 2.0, -2.0, -0.5, -7.0, 3.0, 1.0])
    d = duality_ref.duality(P, q, A, l, u, np.zeros(1), y)
    assert d["SC"] == 2.0 * 2.0 + (-1.0) * (-2.0) + (-2.0) * (-0.5) + 5.0 * 3.0 + 0.0
    assert d["S"] == 4.0 + 2.0 + 1.0 + 15.0 and d["N"] == 1 + 0 + 14
    assert d["dual_obj"] == -d["SC"] and d["gap"] == d["SC"] and d["prim_obj"] == 0.0
    # m = 0
    d0 = duality_ref.duality(sp.csc_matrix(np.array([[2.0]])), np.array([1.0]), sp.csc_matrix((0, 1)), np.zeros(0), np.zeros(0), np.array([3.0]), np.zeros(0))
    assert d0["SC"] == 0.0 and d0["prim_obj"] == 12.0 and d0["dual_obj"] == -9.0 and d0["gap"] == 21.0


@pytest.mark.parametrize("name", duality_cases.ZOO_VALUE_CASES)
def test_strong_duality_at_the_oracle_solution(oracle_lib, name):
    """|gap| <= eps_gap at the oracle's solution, solved to eps = 1e-8, eps_gap at the same eps: the check that the numpy
    statement is the dual of this QP (a wrong sign or a missing term is off by O(S)).

    The solve runs with polish on and the test requires the polish to be accepted.  Strong duality is a property of the
    optimum; a pair that only meets the residual tests at eps is not bound by it:
        gap = x'(Px + q + A'y) - y'(Ax - z) + (SC - y'z),    z = clip(Ax, l, u),
    so |gap| <= |x|_1 |r_dual|_inf + |y|_1 |r_prim|_inf + the complementarity slack -- the residuals weighted by the 1-norms of
    x and y (hundreds of entries here), not eps_gap.  FIGURES (the CPU oracle, adaptive_rho_interval = 25): the ADMM pair
    WITHOUT polish has |gap| / eps_gap = 12.9 on portfolio (stop at iteration 625, gap -5.08e-07, eps_gap 3.95e-08; 16.8 with
    adaptive_rho_interval 50 or 100), 1.4e-3 on huber, 6.7e-3 on svm, 2.4e-2 on control -- the lag of the gap behind the
    residuals that the stopping rule exists for, at a tighter eps.  The polished pairs: 3.4e-08, 2.5e-08, 0, 0."""
    prob = duality_cases.VALUE_CASES[name]()
    eps = 1e-8
    m = oq.Model(oracle_lib)
    oq.setup(m, **prob, verbose=False, eps_abs=eps, eps_rel=eps, max_iter=200000, adaptive_rho_interval=25, polish=True)
    r = oq.solve(m)
    assert r.info.status == "Solved" and r.info.status_polish == 1, (r.info.status, r.info.status_polish)
    d = duality_ref.duality(prob["P"], prob["q"], prob["A"], prob["l"], prob["u"], r.x, r.y, eps, eps)
    oq.clean(m)
    print(f"{name}: iter {r.info.iter} prim {d['prim_obj']:.12g} dual {d['dual_obj']:.12g} gap {d['gap']:.3e} eps_gap {d['eps_gap']:.3e}")
    assert abs(d["gap"]) <= d["eps_gap"], (d["gap"], d["eps_gap"])


@pytest.mark.parametrize("name", list(duality_cases.RULE_CASES))
def test_rule_cases_meet_their_conditions(oracle_lib, name):
    t = duality_cases.rule_trace(oq, oracle_lib, name)
    for k, c in t["checks"].items():
        print(f"{name}: k {k} pri {c['pri']:.3f} dua {c['dua']:.3f} gap {c['gap']:.3f}")
    assert t["K_on"] is not None and t["K_on"] > t["K_off"], (t["K_off"], t["K_on"])
    for k, c in t["checks"].items():
        assert c["pri"] < 1.0 and c["dua"] < 1.0, (k, c["pri"], c["dua"])   # the residual tests hold throughout
        assert (c["gap"] < 1.0) == (k == t["K_on"]), (k, c["gap"])          # the gap refuses before K_on and passes there
        assert abs(c["gap"] - 1.0) > 0.01, (k, c["gap"])                    # no decision within rounding of the bound
