"""Numpy reference of the adjoint of a single model (osqp_amd_adjoint, osqp.jl_amd/csrc/direct_adjoint.hpp).

`model`  the library's algorithm on one problem from the oracle's scaled state (batch_polish_ref.oracle_state / scale_data):
         the classification of the rows, the FULL regularised matrix [P~ + delta I, A~a'; A~a, -delta I] solved densely (the
         library factorises exactly this matrix; the batch kernel's condensed form is another algorithm), `refine` steps
         against the unregularised matrix, back to the caller's units, and the table of batch_adjoint_ref.table.
`exact`  is batch_adjoint_ref.exact: the mathematics in the caller's units.

The cases of the tests, their oracle solutions (computed once per session, never modified) and their incoming gradients are
here too.  No GPU needed; tests/test_model_adjoint_host.py holds `model` to `exact`."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

import batch_adjoint_ref as adj
import batch_polish_ref as pol
import qp_zoo

CASES = ("tiny", "grid2d", "control", "svm", "lasso_data", "equality_qp", "spd7", "control6_unsorted")


def dense_K(P, A, act):
    """K = [P, Aa'; Aa, 0] of the active set, dense, in the caller's units."""
    rows = np.flatnonzero(act)
    Aa = sp.csr_matrix(A)[rows].toarray().reshape(len(rows), P.shape[0])
    return np.block([[adj.full_P(P), Aa.T], [Aa, np.zeros((len(rows), len(rows)))]])


def model(P, q, A, l, u, D, E, c, xs, zs, ys, gx, gy, delta=1e-6, refine=3):
    """The library's algorithm.  Returns the five gradients, "act" and the caller-unit "x", "y" of the state."""
    n, m = len(q), len(l)
    Ps, _, As, ls, us = pol.scale_data(P, q, A, l, u, D, E, c)
    act = adj.classify(zs, ys, ls, us)
    rows = np.concatenate([np.flatnonzero(act < 0), np.flatnonzero(act > 0)])  # lower rows first: the order of the reduced matrix
    mr = len(rows)
    Aa = As[rows].toarray().reshape(mr, n)
    K0 = np.block([[Ps.toarray(), Aa.T], [Aa, np.zeros((mr, mr))]])
    Kreg = K0 + np.diag(np.concatenate([delta * np.ones(n), -delta * np.ones(mr)]))
    lu = sla.lu_factor(Kreg)
    rhs = np.concatenate([c * (D * gx), (E * gy)[rows]])
    sol = sla.lu_solve(lu, rhs)
    for _ in range(refine):
        sol = sol + sla.lu_solve(lu, rhs - K0 @ sol)
    ry = np.zeros(m)
    ry[rows] = sol[n:]
    x, y = D * xs, E * ys / c
    out = adj.table(P, A, x, y, act, D * sol[:n], E * ry / c)
    out.update(act=act, x=x, y=y)
    return out


# ---- the cases ----
def _unsorted_control():
    """control(T=6) and the same A with the rows of one column stored descending: (problem, arrays of the caller's A,
    caller nnz index -> index in the sorted CSC arrays)."""
    p = qp_zoo.control(T=6)
    A = sp.csc_matrix(p["A"]); A.sort_indices()
    lens = np.diff(A.indptr)
    j = int(np.flatnonzero(lens >= 3)[0])
    a, b = A.indptr[j], A.indptr[j + 1]
    data, idx = A.data.copy(), A.indices.copy()
    data[a:b], idx[a:b] = A.data[a:b][::-1], A.indices[a:b][::-1]
    to_sorted = np.arange(A.nnz)
    to_sorted[a:b] = np.arange(a, b)[::-1]
    given = sp.csc_matrix((data, idx, A.indptr.copy()), shape=A.shape)
    assert not given.has_sorted_indices
    return dict(p, A=A), given, to_sorted


_cache = {}


def problems(oracle_lib, case):
    """[dict(P, q, A, l, u)] of a case ("tiny": one per instance of the batch family); A sorted CSC.  The unsorted case also
    carries "A_given" (what the caller hands to setup with keep_A_order=True) and "to_sorted"."""
    if case not in _cache:
        if case == "tiny":
            out = [dict(P=sp.csc_matrix(P), q=q, A=sp.csc_matrix(A), l=l, u=u) for P, q, A, l, u in adj.problems(oracle_lib, "tiny")]
        elif case == "grid2d":
            out = [qp_zoo.grid2d(g=24)]
        elif case == "control":
            out = [qp_zoo.control()]
        elif case == "svm":
            out = [qp_zoo.svm(n=20, m=300)]
        elif case == "lasso_data":
            out = [qp_zoo.lasso_data(n=30, m=300)]
        elif case == "equality_qp":
            out = [qp_zoo.equality_qp(n=300)]
        elif case == "spd7":
            rng = np.random.default_rng(77)
            M = rng.standard_normal((7, 7))
            out = [dict(P=sp.csc_matrix(M @ M.T + 7 * np.eye(7)), q=rng.standard_normal(7), A=sp.csc_matrix((0, 7)), l=np.zeros(0), u=np.zeros(0))]
        elif case == "control6_unsorted":
            p, given, to_sorted = _unsorted_control()
            out = [dict(p, A_given=given, to_sorted=to_sorted)]
        else:
            raise KeyError(case)
        for p in out:
            p["P"] = sp.csc_matrix(p["P"]); p["A"] = sp.csc_matrix(p["A"]); p["A"].sort_indices()
        _cache[case] = out
    return _cache[case]


def setup_args(p):
    """The keyword arguments of oq.setup for a problem of `problems` (the caller's own A where the case has one)."""
    if p["A"].shape[0] == 0:
        return dict(P=p["P"], q=p["q"])
    if "A_given" in p:
        return dict(P=p["P"], q=p["q"], A=p["A_given"], l=p["l"], u=p["u"], keep_A_order=True)
    return dict(P=p["P"], q=p["q"], A=p["A"], l=p["l"], u=p["u"])


def caller_order(p, g):
    """The gradients of `table` (sorted CSC order of A) in the caller's nnz order."""
    if "to_sorted" not in p:
        return g
    return dict(g, Ax=np.asarray(g["Ax"])[..., p["to_sorted"]])


def incoming(case, k, n, m, ncot=1):
    """The random incoming gradients of instance k of a case: (g_x [ncot x n], g_y [ncot x m]); cotangent 0 is the one the
    single-cotangent tests use."""
    rng = np.random.default_rng(sum(map(ord, case)) * 131 + k)
    return rng.standard_normal((ncot, n)), rng.standard_normal((ncot, m))


def oracle_solution(oracle_lib, case, k, scaling=10, **opts):
    """The oracle's polished solve of instance k of a case: dict(status, polish, x, y, state = (D, E, c, xs, zs, ys), act)."""
    import osqp_jl_amd as oq
    import batch_resident_ref as ref

    key = ("sol", case, k, scaling, tuple(sorted(opts.items())))
    if key not in _cache:
        p = problems(oracle_lib, case)[k]
        mdl = oq.Model(oracle_lib)
        args = setup_args(dict((a, b) for a, b in p.items() if a not in ("A_given", "to_sorted")))
        oq.setup(mdl, **args, **dict(ref.OPTS, polish=True, scaling=scaling, **opts))
        r = oq.solve(mdl)
        n, m = len(p["q"]), len(p["l"])
        st = pol.oracle_state(mdl, n, m, scaling)
        D, E, c, xs, zs, ys = st
        _, _, _, ls, us = pol.scale_data(p["P"], p["q"], p["A"], p["l"], p["u"], D, E, c)
        _cache[key] = dict(status=r.info.status_val, polish=r.info.status_polish, x=np.array(r.x), y=np.array(r.y), state=st,
                           act=adj.classify(zs, ys, ls, us))
        oq.clean(mdl)
    return _cache[key]
