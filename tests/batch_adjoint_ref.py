"""Numpy reference of the adjoint of the resident batch (k_batch_adjoint in osqp.jl_amd/csrc/batch_adjoint.hpp), in two parts:

`exact`  the mathematics in the caller's units: the dense KKT matrix of the active set K = [P, Aa'; Aa, 0], np.linalg.solve
         and the table of include/osqp_amd.h;
`model`  the kernel's algorithm on ONE instance from the scaled record (batch_polish_ref.oracle_state): the scaled data,
         the classification of the rows, the condensed regularised matrix, Cholesky, refinement against the unregularised
         system, back to the caller's units.

Gradients of the matrices are in the order of the value arrays `ResidentBatch` takes: the upper triangle of P as sorted CSC,
A as sorted CSC.  No GPU needed; tests/test_batch_adjoint_host.py holds `exact` to finite differences and `model` to `exact`."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

import batch_polish_ref as pol

GRADS = ("q", "l", "u", "Px", "Ax")


def patterns(P, A):
    """(rows, cols) of the stored upper triangle of P and of A, in CSC order."""
    U = sp.triu(sp.csc_matrix(P), format="csc"); U.sort_indices()
    Ac = sp.csc_matrix(A); Ac.sort_indices()
    colsP = np.repeat(np.arange(U.shape[1]), np.diff(U.indptr))
    colsA = np.repeat(np.arange(Ac.shape[1]), np.diff(Ac.indptr))
    return (U.indices.copy(), colsP), (Ac.indices.copy(), colsA)


def full_P(P):
    U = sp.triu(sp.csc_matrix(P), format="csc")
    return (U + sp.triu(U, 1).T).toarray()


def classify(z, y, l, u):
    """-1 lower, 1 upper, 0 inactive: the rule of the polish step, and a row with l == u is always active (lower)."""
    low = ((z - l) < -y) | (l == u)
    upp = ~low & ((u - z) < y)
    return np.where(low, -1, np.where(upp, 1, 0))


def nondegenerate(A, act, n):
    """K of this active set is non-singular (P positive definite): no more active rows than variables, full row rank."""
    rows = np.flatnonzero(act)
    if len(rows) > n:
        return False
    return len(rows) == 0 or np.linalg.matrix_rank(sp.csr_matrix(A)[rows].toarray()) == len(rows)


def active_set_solution(P, q, A, l, u, act):
    """(x, y) of the equality-constrained QP of a fixed active set: K [x; y_a] = [-q; b_a]."""
    n, rows = len(q), np.flatnonzero(act)
    Aa = sp.csr_matrix(A)[rows].toarray()
    K = np.block([[full_P(P), Aa.T], [Aa, np.zeros((len(rows), len(rows)))]])
    b = np.where(act < 0, l, u)[rows]
    s = np.linalg.solve(K, np.concatenate([-q, b]))
    y = np.zeros(len(l))
    y[rows] = s[n:]
    return s[:n], y


def table(P, A, x, y, act, rx, ry):
    """The five gradients from r_x, r_y (zero on inactive rows)."""
    (pi, pj), (ai, aj) = patterns(P, A)
    dP = np.where(pi == pj, -rx[pi] * x[pi], -(rx[pi] * x[pj] + rx[pj] * x[pi]))
    dA = -(y[ai] * rx[aj] + ry[ai] * x[aj])
    return dict(q=-rx, l=np.where(act < 0, ry, 0.0), u=np.where(act > 0, ry, 0.0), Px=dP, Ax=dA)


def exact(P, A, x, y, act, gx, gy):
    n, rows = len(x), np.flatnonzero(act)
    Aa = sp.csr_matrix(A)[rows].toarray()
    K = np.block([[full_P(P), Aa.T], [Aa, np.zeros((len(rows), len(rows)))]])
    s = np.linalg.solve(K, np.concatenate([gx, gy[rows]]))
    ry = np.zeros(len(y))
    ry[rows] = s[n:]
    return table(P, A, x, y, act, s[:n], ry)


def model(P, q, A, l, u, D, E, c, xs, zs, ys, gx, gy, delta=1e-6, refine=3):
    """The kernel's algorithm.  (D, E, c, xs, zs, ys): batch_polish_ref.oracle_state.  Returns the five gradients, "act",
    "status" (1, or -1 on a failed Cholesky: zeros) and the caller-unit "x", "y" of the record."""
    n, m = len(q), len(l)
    Ps, _, As, ls, us = pol.scale_data(P, q, A, l, u, D, E, c)
    act = classify(zs, ys, ls, us)
    rows = np.flatnonzero(act)
    Aa = As[rows]
    x, y = D * xs, E * ys / c
    M = (Ps + delta * sp.identity(n) + (Aa.T @ Aa) / delta).toarray()
    try:
        L = np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        (pi, _), (ai, _) = patterns(P, A)
        return dict(q=np.zeros(n), l=np.zeros(m), u=np.zeros(m), Px=np.zeros(len(pi)), Ax=np.zeros(len(ai)), act=np.zeros(m, int),
                    status=-1, x=x, y=y)

    def kkt_solve(rx, ry):
        t = rx + Aa.T @ ry / delta
        dx = sla.solve_triangular(L, sla.solve_triangular(L, t, lower=True), lower=True, trans="T")
        return dx, (Aa @ dx - ry) / delta

    g, b = c * (D * gx), (E * gy)[rows]
    r, s = kkt_solve(g, b)
    for _ in range(refine):
        dr, ds = kkt_solve(g - Ps @ r - Aa.T @ s, b - Aa @ r)
        r, s = r + dr, s + ds
    ry = np.zeros(m)
    ry[rows] = s
    out = table(P, A, x, y, act, D * r, E * ry / c)
    out.update(act=act, status=1, x=x, y=y)
    return out


def rel_err(got, want):
    """Largest difference over the five gradients, each relative to max(1, max|want|)."""
    worst = 0.0
    for k in GRADS:
        if len(want[k]):
            worst = max(worst, float(np.max(np.abs(np.asarray(got[k]) - want[k]))) / max(1.0, float(np.max(np.abs(want[k])))))
    return worst


# ---- the problem families of the adjoint tests and their oracle solutions (computed once per session, never modified) ----
FAMILIES = ("tiny", "ineq", "wide300", "tri128", "eq100", "mpc")
MIN_NONDEGENERATE = dict(tiny=8, ineq=6, wide300=6, tri128=3, eq100=3, mpc=20)  # instances a comparison must cover
_cache = {}


def problems(oracle_lib, family):
    """The per-instance (P, q, A, l, u) of a family."""
    import batch_resident_ref as ref
    from test_batch_gpu import _family

    key = ("probs", family)
    if key not in _cache:
        if family == "mpc":
            _cache[key] = ref.mpc_instances(oracle_lib, 0, 64, 2)
        else:
            n, m, count, seed, kw = dict(tiny=(5, 3, 8, 503, {}), ineq=(40, 120, 6, 40120, dict(equalities=False)),
                                         wide300=(20, 300, 6, 20300, dict(equalities=False)),
                                         tri128=(128, 256, 3, 128256, dict(tridiagonal_P=True, equalities=False)),
                                         eq100=(100, 60, 6, 10060, {}))[family]
            _cache[key] = _family(n, m, count, seed, **kw)[1]
    return _cache[key]


def oracle_solve(oracle_lib, probs, q=None, l=None, u=None, **opts):
    """One oracle model per instance, polish on: [dict(status, polish, x, y, state = (D, E, c, xs, zs, ys), act)]; the
    state is what the solve left (the polished iterate where the polish was accepted), act its classification."""
    import osqp_jl_amd as oq
    import batch_resident_ref as ref

    out = []
    for i, (P, pq, A, pl, pu) in enumerate(probs):
        pq, pl, pu = (pq if q is None else q[i]), (pl if l is None else l[i]), (pu if u is None else u[i])
        mdl = oq.Model(oracle_lib)
        oq.setup(mdl, P=P, q=pq, A=A, l=pl, u=pu, **dict(ref.OPTS, polish=True, **opts))
        r = oq.solve(mdl)
        st = pol.oracle_state(mdl, len(pq), len(pl), dict(ref.OPTS, **opts).get("scaling", 10))
        D, E, c, xs, zs, ys = st
        _, _, _, ls, us = pol.scale_data(P, pq, A, pl, pu, D, E, c)
        out.append(dict(status=r.info.status_val, polish=r.info.status_polish, x=np.array(r.x), y=np.array(r.y), state=st,
                        act=classify(zs, ys, ls, us)))
        oq.clean(mdl)
    return out


def oracle_solutions(oracle_lib, family):
    key = ("sols", family)
    if key not in _cache:
        _cache[key] = oracle_solve(oracle_lib, problems(oracle_lib, family))
    return _cache[key]


def incoming(family, count, n, m):
    """The random incoming gradients (g_x [count x n], g_y [count x m]) the tests of a family share."""
    rng = np.random.default_rng(sum(map(ord, family)))
    return rng.standard_normal((count, n)), rng.standard_normal((count, m))
