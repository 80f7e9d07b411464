"""Adjoint of a single model without a GPU (tests/model_adjoint_ref.py):
(a) `model` -- the library's algorithm from the oracle's scaled state -- against `exact` on every case, scaling 10 and 0, with
    3 refinement steps and with none;
(b) `exact` against central finite differences of the active-set solution on control(T=6), all five arrays moved at once;
(c) the header, the symbols, the NULL workspace, the argument checks of `interface.adjoint`, a library without the symbol.

Figures are `rel_err` (relative to max(1, |reference|)); every test prints before it asserts.  (a): the bound of a case is
100 times MEASURED below (the residue is rounding times cond K; cond_2 K <= 5.3e3 on these cases), as in
test_batch_adjoint_host.py; the GPU test derives its bounds from MEASURED.  Measured (worst of
scaling 10 and 0; in brackets the same with 0 refinement steps, which must stay above 1e-8: whether refinement runs is
observable):
  tiny 7.8e-16 [1.7e-5]   grid2d 1.4e-15 [9.0e-6]   control 1.7e-14 [1.5e-4]   svm 8.2e-16 [1.1e-4]
  lasso_data 1.5e-14 [5.5e-5]   equality_qp 1.1e-14 [1.2e-5]   spd7 2.8e-17 [2.2e-7]   control6_unsorted 3.2e-15 [1.2e-4]
(b): |fd - analytic| = 1.5e-8 on a loss derivative of -197.8 at h = 1e-7, against a bound of 5.9e-4 (cond K = 1.3e3; below)."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_jl_amd as oq
from osqp_jl_amd import interface
from osqp_jl_amd import types as T
import batch_adjoint_ref as adj
import model_adjoint_ref as mar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MEASURED = dict(tiny=7.8e-16, grid2d=1.4e-15, control=1.7e-14, svm=8.2e-16, lasso_data=1.5e-14, equality_qp=1.1e-14, spd7=2.8e-17,
                control6_unsorted=3.2e-15)  # the GPU test's bounds derive from these


@pytest.mark.parametrize("case", mar.CASES)
def test_model_agrees_with_exact(oracle_lib, case):
    worst, worst0 = 0.0, 0.0
    probs = mar.problems(oracle_lib, case)
    for scaling in (10, 0):
        for k, p in enumerate(probs):
            s = mar.oracle_solution(oracle_lib, case, k, scaling)
            assert s["status"] == 1 and s["polish"] == 1, (case, k, scaling, s["status"], s["polish"])
            n, m = len(p["q"]), len(p["l"])
            assert adj.nondegenerate(p["A"], s["act"], n)
            sign = np.where(s["y"] < 0, -1, np.where(s["y"] > 0, 1, 0))
            assert np.array_equal(s["act"], np.where(p["l"] == p["u"], -1, sign)), (case, k, scaling)
            gx, gy = mar.incoming(case, k, n, m)
            want = None
            for refine in (3, 0):
                got = mar.model(p["P"], p["q"], p["A"], p["l"], p["u"], *s["state"], gx[0], gy[0], refine=refine)
                assert np.array_equal(got["act"], s["act"])
                if want is None:
                    want = adj.exact(p["P"], p["A"], got["x"], got["y"], got["act"], gx[0], gy[0])
                err = adj.rel_err(got, want)
                if refine:
                    worst = max(worst, err)
                else:
                    worst0 = max(worst0, err)
    print(f"(a) {case}: {len(probs)} problem(s) x 2 scalings, model vs exact worst rel {worst:.2e}; without refinement {worst0:.2e}")
    assert worst <= 100 * MEASURED[case], worst
    assert worst0 > 1e-8, worst0  # the regularised answer alone is visibly not the exact one


def test_exact_agrees_with_finite_differences_of_the_active_set_solution(oracle_lib):
    """control(T=6): loss = g_x . x + g_y . y of the solution of the fixed active set, data moved by +-h d along a random
    direction in Px, Ax, q, l, u together.  Bound, reasoned: the two solves carry a rounding error of eps cond(K) |loss| each,
    divided by 2h; the loss is not affine in Px, Ax and the central difference truncates at h^2 times the third derivative,
    ~cond(K)^2 |loss|.  With h = 1e-7 and cond(K) ~ 1e2 .. 5e3 the first term leads (<= 1.2e-5)."""
    case, h = "control6_unsorted", 1e-7
    p = mar.problems(oracle_lib, case)[0]
    s = mar.oracle_solution(oracle_lib, case, 0)
    P, q, A, l, u, act = p["P"], p["q"], p["A"], p["l"], p["u"], s["act"]
    n, m = len(q), len(l)
    gx, gy = (g[0] for g in mar.incoming(case, 0, n, m))
    x, y = adj.active_set_solution(P, q, A, l, u, act)
    g = adj.exact(P, A, x, y, act, gx, gy)
    U = sp.triu(P, format="csc"); U.sort_indices()
    rng = np.random.default_rng(5)
    d = {k: rng.standard_normal(len(g[k])) for k in adj.GRADS}
    d["u"] = np.where(l == u, d["l"], d["u"])  # an equality row moves as one
    loss = []
    for sign in (1.0, -1.0):
        Ud, Ad = U.copy(), A.copy()
        Ud.data = U.data + sign * h * d["Px"]; Ad.data = A.data + sign * h * d["Ax"]
        xp, yp = adj.active_set_solution(Ud, q + sign * h * d["q"], Ad, l + sign * h * d["l"], u + sign * h * d["u"], act)
        loss.append(gx @ xp + gy @ yp)
    fd, an = (loss[0] - loss[1]) / (2 * h), sum(float(g[k] @ d[k]) for k in adj.GRADS)
    cond = np.linalg.cond(mar.dense_K(P, A, act))
    bound = (np.finfo(float).eps * cond / h + h * h * cond * cond) * max(1.0, abs(loss[0]), abs(an))
    print(f"(b) control(T=6): fd {fd:.12e} analytic {an:.12e} |diff| {abs(fd - an):.2e} bound {bound:.2e} (cond K {cond:.2e})")
    assert abs(fd - an) <= bound


def test_the_header_declares_and_the_library_exports_the_symbols(product_lib):
    text = open(os.path.join(ROOT, "include", "osqp_amd.h")).read()
    for name, nargs in (("osqp_amd_adjoint", 10), ("osqp_amd_adjoint_release", 1), ("osqp_amd_adjoint_stats", 3)):
        assert re.search(r"c_int\s+" + name + r"\s*\(", text), name
        assert name in T.EXT_SYMBOLS, name
        res, args = T.EXT_SYMBOLS[name]
        assert res is T.c_int and len(args) == nargs
        fn = getattr(product_lib, name)  # AttributeError: not exported
        assert fn.restype is T.c_int and list(fn.argtypes or []) == list(args)


def test_adjoint_refuses_a_null_workspace(product_lib):
    buf = np.full(4, np.nan)
    p = buf.ctypes.data_as(T.c_float_p)
    assert product_lib.osqp_amd_adjoint(None, 1, p, None, p, None, None, None, None, None) != 0
    assert b"workspace" in product_lib.osqp_amd_last_error()
    assert np.all(np.isnan(buf))
    assert product_lib.osqp_amd_adjoint_release(None) != 0
    assert product_lib.osqp_amd_adjoint_stats(None, p, 4) == 0 and np.all(np.isnan(buf))


class _NoCall:
    """A library whose adjoint entry must not be reached: the checks of `interface.adjoint` come first."""

    class _Fn:
        argtypes = ()

        def __call__(self, *a):
            raise AssertionError("the library was called")

    osqp_amd_adjoint = _Fn()
    osqp_amd_adjoint_release = _Fn()
    osqp_amd_adjoint_stats = _Fn()
    osqp_amd_get_stats = _Fn()


def _fake_model(n, m):
    mdl = interface.Model.__new__(interface.Model)
    mdl.lib = _NoCall()
    data = T.Data(n, m, None, None, None, None, None)
    ws = T.Workspace()
    ws.data = T.C.pointer(data)
    mdl._keep = (data, ws)
    mdl.workspace = T.C.pointer(ws)
    mdl.isempty = False
    return mdl


def test_adjoint_checks_its_arguments_in_python():
    mdl = _fake_model(3, 2)
    try:
        with pytest.raises(ValueError, match="dx and dy"):
            interface.adjoint(mdl)
        with pytest.raises(ValueError, match="dx"):
            interface.adjoint(mdl, dx=np.ones(4))
        with pytest.raises(ValueError, match="dy"):
            interface.adjoint(mdl, dy=np.ones((2, 3)))
        with pytest.raises(ValueError, match="dx"):
            interface.adjoint(mdl, dx=np.ones((2, 2, 3)))
        with pytest.raises(ValueError, match="dx"):
            interface.adjoint(mdl, dx=np.ones((0, 3)))
        with pytest.raises(ValueError, match="dx"):
            interface.adjoint(mdl, dx=np.array(["a", "b", "c"]))
        with pytest.raises(ValueError, match="dy"):
            interface.adjoint(mdl, dy=np.ones(2, dtype=complex))
        with pytest.raises(ValueError, match="unknown"):
            interface.adjoint(mdl, dx=np.ones(3), want=("q", "z"))
        with pytest.raises(ValueError, match="twice"):
            interface.adjoint(mdl, dx=np.ones(3), want=("q", "q"))
        with pytest.raises(ValueError, match="leading"):
            interface.adjoint(mdl, dx=np.ones(3), dy=np.ones((1, 2)))
        with pytest.raises(ValueError, match="number of cotangents"):
            interface.adjoint(mdl, dx=np.ones((2, 3)), dy=np.ones((3, 2)))
    finally:
        mdl.workspace = T.Workspace_p()  # nothing for __del__ to clean


def test_a_library_without_the_symbol_raises(oracle_lib):
    p = mar.problems(oracle_lib, "spd7")[0]
    mdl = oq.Model(oracle_lib)
    oq.setup(mdl, **mar.setup_args(p), verbose=False)
    oq.solve(mdl)
    for call in (lambda: oq.adjoint(mdl, dx=np.ones(7)), lambda: oq.adjoint_release(mdl), lambda: oq.adjoint_stats(mdl)):
        with pytest.raises(oq.OSQPError, match="does not export"):
            call()
    oq.clean(mdl)
