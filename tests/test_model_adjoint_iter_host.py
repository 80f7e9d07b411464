"""The iterative derivatives of a single model without a GPU (osqp_amd_derivative_method; tests/model_adjoint_iter_ref.py):
(a) the numpy statement of the iterative KKT solve -- Jacobi-preconditioned CG on the condensed operator, the library's
    constants and stopping rule -- on all eight model_adjoint_ref.CASES from the oracle's solutions (scaling 10) against
    `exact` (dense solve of the unregularised K), adjoint and JVP, and the duality of the two;
(b) the header, the symbols, the NULL workspace, the argument checks of `interface.derivative_method`, a library without
    the symbols.

Figures are `rel_err` of batch_adjoint_ref / batch_jvp_ref (relative to max(1, |reference|)) and `duality_gap`; every test
prints before it asserts.  The solve stops on a DROP of the residual of 1e-10, not at rounding: its distance from `exact`
is that drop times cond K times the size of the first residual, orders above the direct model's figure.  Measured (worst
instance; adjoint / JVP / duality gap / outer steps, all cases meet the stopping rule within 40 steps):
  tiny 1.6e-12 / 1.4e-12 / 1.5e-13 / 6      grid2d 1.4e-11 / 1.2e-11 / 3.3e-14 / 6    control 3.6e-8 / 9.1e-9 / 2.7e-10 / 15
  svm 4.3e-10 / 1.7e-9 / 1.7e-11 / 9        lasso_data 1.1e-11 / 5.2e-12 / 4.6e-15 / 5  equality_qp 1.6e-11 / 6.6e-12 / 1.9e-15 / 6
  spd7 1.3e-15 / 3.4e-15 / 5.6e-17 / 5      control6_unsorted 2.6e-10 / 8.4e-11 / 1.4e-11 / 10
The bound of a case is 100 times the recorded figure (the rule of tests/test_model_adjoint_host.py: another BLAS sums in
another order and the CG takes a slightly different path); the GPU tests derive their bounds from the same tables."""
import os
import re

import numpy as np
import pytest

import osqp_jl_amd as oq
from osqp_jl_amd import interface
from osqp_jl_amd import types as T
import batch_adjoint_ref as adj
import batch_jvp_ref as jv
import model_adjoint_ref as mar
import model_adjoint_iter_ref as mir
import model_jvp_ref as mjr
from test_model_adjoint_host import _fake_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.2e-16

# the larger of the adjoint's and the JVP's figure against `exact`: the GPU test's bounds derive from these
MEASURED_ITER = dict(tiny=1.6e-12, grid2d=1.4e-11, control=3.7e-8, svm=1.7e-9, lasso_data=1.1e-11, equality_qp=1.7e-11, spd7=3.5e-15,
                     control6_unsorted=2.6e-10)
MEASURED_ITER_DUALITY = dict(tiny=1.6e-13, grid2d=3.3e-14, control=2.7e-10, svm=1.7e-11, lasso_data=4.6e-15, equality_qp=2.0e-15, spd7=5.6e-17,
                             control6_unsorted=1.4e-11)
OUTER_STEPS = dict(tiny=6, grid2d=6, control=15, svm=9, lasso_data=5, equality_qp=6, spd7=5, control6_unsorted=10)  # worst of adjoint and JVP
NOT_CONVERGED = {}  # case -> reached drop: none; at most three may be listed, never "tiny" or "control"

_runs = {}


def runs(oracle_lib, case):
    """Per instance of a case: (problem, incoming gradients, direction, adjoint model, JVP model); computed once, never modified."""
    if case not in _runs:
        out = []
        for k, p in enumerate(mar.problems(oracle_lib, case)):
            s = mar.oracle_solution(oracle_lib, case, k, 10)
            assert s["status"] == 1 and s["polish"] == 1, (case, k)
            n, m = len(p["q"]), len(p["l"])
            gx, gy = (g[0] for g in mar.incoming(case, k, n, m))
            d = mjr.reference_direction(p, mjr.direction(mjr.tangents(case, k, p), 0))
            data = (p["P"], p["q"], p["A"], p["l"], p["u"])
            out.append((p, gx, gy, d, mir.adjoint_model(*data, *s["state"], gx, gy), mir.jvp_model(*data, *s["state"], d)))
        _runs[case] = out
    return _runs[case]


def test_the_tables_are_complete():
    assert set(MEASURED_ITER) == set(MEASURED_ITER_DUALITY) == set(OUTER_STEPS) == set(mar.CASES)
    assert len(NOT_CONVERGED) <= 3 and "tiny" not in NOT_CONVERGED and "control" not in NOT_CONVERGED


@pytest.mark.parametrize("case", mar.CASES)
def test_model_agrees_with_exact(oracle_lib, case):
    worst_a, worst_j, outer, drop = 0.0, 0.0, 0, 0.0
    for p, gx, gy, d, ga, gj in runs(oracle_lib, case):
        assert np.array_equal(ga["act"], gj["act"])
        for info in (ga["info"], gj["info"]):
            outer, drop = max(outer, info["outer"]), max(drop, info["drop"])
            assert info["converged"] == (case not in NOT_CONVERGED), (case, info)
        worst_a = max(worst_a, adj.rel_err(ga, adj.exact(p["P"], p["A"], ga["x"], ga["y"], ga["act"], gx, gy)))
        tx, ty = jv.exact(p["P"], p["A"], gj["x"], gj["y"], gj["act"], d)
        worst_j = max(worst_j, jv.rel_err(gj["tx"], gj["ty"], tx, ty))
    print(f"(a) {case}: adjoint vs exact {worst_a:.2e}  jvp vs exact {worst_j:.2e}  outer steps {outer}  drop {drop:.2e}")
    assert max(worst_a, worst_j) <= 100 * MEASURED_ITER[case]
    assert outer <= mir.MAX_OUTER and drop <= mir.REL_DROP
    assert ga["info"]["outer"] > 3  # more than polish_refine_iter steps


@pytest.mark.parametrize("case", mar.CASES)
def test_duality_of_the_two_models(oracle_lib, case):
    """gx . tx + gy . ty = sum_k <g_k, d_k>: two solves with the same symmetric K (the rule and the floor of
    tests/test_model_jvp_host.py: 10 eps cond_2 K, or 100 x the recorded figure)."""
    worst, floor = 0.0, np.inf
    for p, gx, gy, d, ga, gj in runs(oracle_lib, case):
        floor = min(floor, 10 * EPS * np.linalg.cond(mar.dense_K(p["P"], p["A"], ga["act"])))
        worst = max(worst, jv.duality_gap(gx, gy, gj["tx"], gj["ty"], ga, d))
    print(f"(a) {case}: duality gap model/model {worst:.2e}  (10 eps cond K >= {floor:.2e})")
    assert worst <= max(floor, 100 * MEASURED_ITER_DUALITY[case])


def test_a_cap_of_one_step_is_reported(oracle_lib):
    p, gx, gy, d, ga, gj = runs(oracle_lib, "control")[0]
    s = mar.oracle_solution(oracle_lib, "control", 0, 10)
    got = mir.adjoint_model(p["P"], p["q"], p["A"], p["l"], p["u"], *s["state"], gx, gy, refine=0, max_outer=1)
    assert not got["info"]["converged"] and got["info"]["outer"] == 1 and got["info"]["drop"] == 1.0


SYMBOLS = (("osqp_amd_derivative_method", 4), ("osqp_amd_derivative_iter_stats", 3))


def test_the_header_declares_and_the_library_exports_the_symbols(product_lib):
    text = open(os.path.join(ROOT, "include", "osqp_amd.h")).read()
    for name, nargs in SYMBOLS:
        assert re.search(r"c_int\s+" + name + r"\s*\(", text), name
        assert name in T.EXT_SYMBOLS, name
        res, args = T.EXT_SYMBOLS[name]
        assert res is T.c_int and len(args) == nargs
        fn = getattr(product_lib, name)  # AttributeError: not exported
        assert fn.restype is T.c_int and list(fn.argtypes or []) == list(args)
    assert re.search(r"#define\s+OSQP_AMD_DERIVATIVE_ITER_STATS_COUNT\s+7\b", text)
    assert len(interface.DERIVATIVE_ITER_STATS_FIELDS) == 7


def test_a_null_workspace(product_lib):
    buf = np.full(8, np.nan)
    p = buf.ctypes.data_as(T.c_float_p)
    assert product_lib.osqp_amd_derivative_method(None, 2, 0, 0.0) == 7
    assert b"workspace" in product_lib.osqp_amd_last_error()
    assert product_lib.osqp_amd_derivative_iter_stats(None, p, 7) == 0 and np.all(np.isnan(buf))


class _NoCall:
    class _Fn:
        argtypes = ()

        def __call__(self, *a):
            raise AssertionError("the library was called")

    osqp_amd_derivative_method = _Fn()
    osqp_amd_derivative_iter_stats = _Fn()


def test_derivative_method_checks_its_arguments_in_python():
    mdl = _fake_model(3, 2)
    mdl.lib = _NoCall()
    try:
        with pytest.raises(ValueError, match="method"):
            interface.derivative_method(mdl, "cg")
        with pytest.raises(ValueError, match="method"):
            interface.derivative_method(mdl, 2)
        for bad in (0, -1, 1.5, True, "3"):
            with pytest.raises(ValueError, match="max_outer"):
                interface.derivative_method(mdl, "iterative", max_outer=bad)
        for bad in (0.0, 1.0, -1e-3, 1, "1e-8"):
            with pytest.raises(ValueError, match="rel_drop"):
                interface.derivative_method(mdl, "auto", rel_drop=bad)
    finally:
        mdl.workspace = T.Workspace_p()  # nothing for __del__ to clean


def test_a_library_without_the_symbols_raises(oracle_lib):
    p = mar.problems(oracle_lib, "spd7")[0]
    mdl = oq.Model(oracle_lib)
    oq.setup(mdl, **mar.setup_args(p), verbose=False)
    for call in (lambda: oq.derivative_method(mdl, "auto"), lambda: oq.derivative_iter_stats(mdl)):
        with pytest.raises(oq.OSQPError, match="does not export"):
            call()
    oq.clean(mdl)
