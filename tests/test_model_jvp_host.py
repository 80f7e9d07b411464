"""Forward sensitivities of a single model without a GPU (tests/model_jvp_ref.py):
(a) `model` -- the library's algorithm from the oracle's scaled state -- against `batch_jvp_ref.exact` on every case of
    model_adjoint_ref.CASES, scaling 10 and 0, with 3 refinement steps and with none;
(b) duality: gx . tx + gy . ty against sum_k <gradient_k, direction_k>, between `batch_adjoint_ref.exact` and
    `batch_jvp_ref.exact`, and between the two numpy models of the library (model_adjoint_ref.model, model_jvp_ref.model);
(c) `exact` against central finite differences of the active-set solution on control(T=6), all five arrays moved at once;
(d) the header, the symbol, the NULL workspace, the argument checks of `interface.jvp`, a library without the symbol.

Figures are `batch_jvp_ref.rel_err` (relative to max(1, |reference|)) and `duality_gap`; every test prints before it asserts.
(a): the bound of a case is 100 times MEASURED_JVP below (the rule of tests/test_model_adjoint_host.py: the residue is
rounding times cond K); the GPU test derives its bounds from MEASURED_JVP and MEASURED_DUALITY.  Measured (worst of scaling
10 and 0; in brackets the same with 0 refinement steps, which must stay above 1e-8: whether refinement runs is observable):
  tiny 9.1e-16 [1.7e-5]   grid2d 2.0e-15 [1.1e-5]   control 1.2e-14 [1.7e-4]   svm 1.6e-15 [5.4e-5]
  lasso_data 1.2e-14 [5.0e-5]   equality_qp 1.8e-14 [9.8e-6]   spd7 2.8e-17 [2.4e-7]   control6_unsorted 5.1e-15 [1.0e-4]
(b): exact against exact <= 3.7e-16 on every case (bound 10 eps cond_2 K >= 7.8e-15, below); model against model:
MEASURED_DUALITY, <= 1.3e-16.
(c): |fd - analytic| = 7.4e-9 (x) / 5.6e-8 (y) at h = 1e-7 against a bound of 6.2e-4 (cond K = 1.3e3; below)."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_jl_amd as oq
from osqp_jl_amd import interface
from osqp_jl_amd import types as T
import batch_adjoint_ref as adj
import batch_jvp_ref as jv
import model_adjoint_ref as mar
import model_jvp_ref as mjr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.2e-16

# `model` against `exact`, 3 refinement steps, worst of the scalings and instances: the GPU test's bounds derive from these
MEASURED_JVP = dict(tiny=9.1e-16, grid2d=2.0e-15, control=1.2e-14, svm=1.6e-15, lasso_data=1.2e-14, equality_qp=1.8e-14, spd7=2.8e-17,
                    control6_unsorted=5.1e-15)
# duality gap between model_adjoint_ref.model and model_jvp_ref.model, the same worst
MEASURED_DUALITY = dict(tiny=1.3e-16, grid2d=1.4e-17, control=3.8e-18, svm=1.1e-17, lasso_data=1.4e-17, equality_qp=3.6e-18, spd7=2.8e-17,
                        control6_unsorted=4.6e-17)


def _each(oracle_lib, case):
    """(k, problem, oracle solution, direction 0 in the sorted order, incoming gradients) per scaling and instance."""
    for scaling in (10, 0):
        for k, p in enumerate(mar.problems(oracle_lib, case)):
            s = mar.oracle_solution(oracle_lib, case, k, scaling)
            assert s["status"] == 1 and s["polish"] == 1, (case, k, scaling, s["status"], s["polish"])
            n, m = len(p["q"]), len(p["l"])
            assert adj.nondegenerate(p["A"], s["act"], n)
            d = mjr.reference_direction(p, mjr.direction(mjr.tangents(case, k, p), 0))
            gx, gy = mar.incoming(case, k, n, m)
            yield k, p, s, d, gx[0], gy[0]


@pytest.mark.parametrize("case", mar.CASES)
def test_model_agrees_with_exact(oracle_lib, case):
    worst, worst0 = 0.0, 0.0
    for k, p, s, d, _, _ in _each(oracle_lib, case):
        want = None
        for refine in (3, 0):
            got = mjr.model(p["P"], p["q"], p["A"], p["l"], p["u"], *s["state"], d, refine=refine)
            assert np.array_equal(got["act"], s["act"])
            if want is None:
                want = jv.exact(p["P"], p["A"], got["x"], got["y"], got["act"], d)
            err = jv.rel_err(got["tx"], got["ty"], *want)
            if refine:
                worst = max(worst, err)
            else:
                worst0 = max(worst0, err)
    print(f"(a) {case}: model vs exact worst rel {worst:.2e}; without refinement {worst0:.2e}")
    assert worst <= 100 * MEASURED_JVP[case], worst
    assert worst0 > 1e-8, worst0  # the regularised answer alone is visibly not the exact one


@pytest.mark.parametrize("case", mar.CASES)
def test_duality_with_the_adjoint(oracle_lib, case):
    """Forward and reverse mode are two solves with the same symmetric K: gx . tx + gy . ty = sum_k <g_k, d_k> up to the
    rounding of the two solves.  Bound of exact against exact, reasoned: each solve carries a relative error of eps cond_2 K
    in norm; `duality_gap` divides by the sum of the |terms|, which for these random vectors is (2 / pi) of the product of the
    norms; the two sums add a few eps: 10 eps cond_2 K covers 2 (pi / 2) eps cond K + the sums.  The two models solve the scaled
    matrix with refinement, to the same accuracy: the larger of that bound and 100 x MEASURED_DUALITY (the rule of (a))."""
    worst_exact, worst_model, floor = 0.0, 0.0, np.inf
    for k, p, s, d, gx, gy in _each(oracle_lib, case):
        P, A = p["P"], p["A"]
        ma = mar.model(P, p["q"], A, p["l"], p["u"], *s["state"], gx, gy)
        mj = mjr.model(P, p["q"], A, p["l"], p["u"], *s["state"], d)
        x, y, act = mj["x"], mj["y"], mj["act"]
        ge = adj.exact(P, A, x, y, act, gx, gy)
        tx, ty = jv.exact(P, A, x, y, act, d)
        floor = min(floor, 10 * EPS * np.linalg.cond(mar.dense_K(P, A, act)))
        worst_exact = max(worst_exact, jv.duality_gap(gx, gy, tx, ty, ge, d))
        worst_model = max(worst_model, jv.duality_gap(gx, gy, mj["tx"], mj["ty"], ma, d))
    print(f"(b) {case}: duality gap exact/exact {worst_exact:.2e}  model/model {worst_model:.2e}  (10 eps cond K >= {floor:.2e})")
    assert worst_exact <= floor
    assert worst_model <= max(floor, 100 * MEASURED_DUALITY[case])


def test_exact_agrees_with_finite_differences_of_the_active_set_solution(oracle_lib):
    """control(T=6): (x, y) of the fixed active set with the data moved by +-h d along one random direction in q, l, u, Px, Ax
    together, h = 1e-7.  Bound: the expression of tests/test_model_adjoint_host.py (b) -- rounding eps cond(K) of each solve
    divided by h, truncation h^2 cond(K)^2 -- on the scale of the solution and of its tangent."""
    case, h = "control6_unsorted", 1e-7
    p = mar.problems(oracle_lib, case)[0]
    s = mar.oracle_solution(oracle_lib, case, 0)
    P, q, A, l, u, act = p["P"], p["q"], p["A"], p["l"], p["u"], s["act"]
    x, y = adj.active_set_solution(P, q, A, l, u, act)
    U = sp.triu(P, format="csc"); U.sort_indices()
    rng = np.random.default_rng(5)
    d = {k: rng.standard_normal(w) for k, w in zip(jv.TANGENTS, (len(q), len(l), len(l), U.nnz, A.nnz))}
    d["u"] = np.where(l == u, d["l"], d["u"])  # an equality row moves as one
    tx, ty = jv.exact(P, A, x, y, act, d)
    moved = []
    for sign in (1.0, -1.0):
        Ud, Ad = U.copy(), A.copy()
        Ud.data = U.data + sign * h * d["Px"]; Ad.data = A.data + sign * h * d["Ax"]
        moved.append(adj.active_set_solution(Ud, q + sign * h * d["q"], Ad, l + sign * h * d["l"], u + sign * h * d["u"], act))
    fx, fy = (moved[0][0] - moved[1][0]) / (2 * h), (moved[0][1] - moved[1][1]) / (2 * h)
    cond = np.linalg.cond(mar.dense_K(P, A, act))
    scale = max(1.0, *(float(np.max(np.abs(v))) for v in (moved[0][0], moved[0][1], tx, ty)))
    bound = (np.finfo(float).eps * cond / h + h * h * cond * cond) * scale
    ex, ey = float(np.max(np.abs(fx - tx))), float(np.max(np.abs(fy - ty)))
    print(f"(c) control(T=6): |fd - analytic| x {ex:.2e} y {ey:.2e} bound {bound:.2e} (cond K {cond:.2e}, scale {scale:.2e})")
    assert ex <= bound and ey <= bound


def test_the_header_declares_and_the_library_exports_the_symbol(product_lib):
    text = open(os.path.join(ROOT, "include", "osqp_amd.h")).read()
    name = "osqp_amd_jvp"
    assert re.search(r"c_int\s+" + name + r"\s*\(", text)
    assert name in T.EXT_SYMBOLS
    res, args = T.EXT_SYMBOLS[name]
    assert res is T.c_int and len(args) == 10
    fn = getattr(product_lib, name)  # AttributeError: not exported
    assert fn.restype is T.c_int and list(fn.argtypes or []) == list(args)


def test_jvp_refuses_a_null_workspace(product_lib):
    buf = np.full(4, np.nan)
    p = buf.ctypes.data_as(T.c_float_p)
    assert product_lib.osqp_amd_jvp(None, 1, p, None, None, None, None, p, p, p) == 7
    assert b"osqp_amd_jvp" in product_lib.osqp_amd_last_error() and b"workspace" in product_lib.osqp_amd_last_error()
    assert np.all(np.isnan(buf))


class _NoCall:
    """A library whose jvp entry must not be reached: the checks of `interface.jvp` come first.  Its stats say nnz(A) = 4 and
    nnz(P upper) = 5 (the widths of Ax and Px)."""

    class _Fn:
        argtypes = ()

        def __call__(self, *a):
            raise AssertionError("the library was called")

    class _Stats:
        argtypes = ()

        def __call__(self, ws, out, count):
            for i, v in enumerate((0.0, 4.0, 0.0, 5.0)[:count]):
                out[i] = v
            return min(count, 4)

    osqp_amd_jvp = _Fn()
    osqp_amd_adjoint = _Fn()
    osqp_amd_get_stats = _Stats()


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


def test_jvp_checks_its_arguments_in_python():
    mdl = _fake_model(3, 2)
    try:
        with pytest.raises(ValueError, match="all None"):
            interface.jvp(mdl)
        with pytest.raises(TypeError):
            interface.jvp(mdl, z=np.ones(3))  # an unknown tangent
        with pytest.raises(ValueError, match="q"):
            interface.jvp(mdl, q=np.ones(4))
        with pytest.raises(ValueError, match="l"):
            interface.jvp(mdl, l=np.ones((2, 3)))
        with pytest.raises(ValueError, match="u"):
            interface.jvp(mdl, u=np.ones((2, 2, 2)))
        with pytest.raises(ValueError, match="q"):
            interface.jvp(mdl, q=np.ones((0, 3)))
        with pytest.raises(ValueError, match="Px"):
            interface.jvp(mdl, Px=np.ones(4))  # nnz(P upper) is 5
        with pytest.raises(ValueError, match="Ax"):
            interface.jvp(mdl, q=np.ones(3), Ax=np.ones(5))  # nnz(A) is 4
        with pytest.raises(ValueError, match="q"):
            interface.jvp(mdl, q=np.array(["a", "b", "c"]))
        with pytest.raises(ValueError, match="l"):
            interface.jvp(mdl, l=np.ones(2, dtype=complex))
        with pytest.raises(ValueError, match="leading"):
            interface.jvp(mdl, q=np.ones(3), l=np.ones((1, 2)))
        with pytest.raises(ValueError, match="number of directions"):
            interface.jvp(mdl, q=np.ones((2, 3)), Ax=np.ones((3, 4)))
        for bad in (dict(of=("z",)), dict(of=()), dict(wrt=("q", "q")), dict(mode="both"), dict(chunk=0), dict(out_rows=dict(y=[0])),
                    dict(out_rows=dict(x=[3])), dict(out_rows=dict(x=[0.5]))):
            with pytest.raises(ValueError):
                interface.jacobian(mdl, **bad)
    finally:
        mdl.workspace = T.Workspace_p()  # nothing for __del__ to clean


def test_a_library_without_the_symbol_raises(oracle_lib):
    p = mar.problems(oracle_lib, "spd7")[0]
    mdl = oq.Model(oracle_lib)
    oq.setup(mdl, **mar.setup_args(p), verbose=False)
    oq.solve(mdl)
    with pytest.raises(oq.OSQPError, match="does not export"):
        oq.jvp(mdl, q=np.ones(7))
    with pytest.raises(oq.OSQPError, match="does not export"):
        oq.jacobian(mdl, mode="forward", wrt=("q",))
    oq.clean(mdl)
