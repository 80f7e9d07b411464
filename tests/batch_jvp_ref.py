"""Numpy reference of the forward sensitivities of the resident batch (k_batch_jvp in osqp.jl_amd/csrc/batch_jvp.hpp), in two
parts, as tests/batch_adjoint_ref.py has them for the adjoint:

`exact`  the mathematics in the caller's units: with the active rows a and K = [P, Aa'; Aa, 0],
         K [tx; ty_a] = [-(tq + tP x + tA' y); (tb - tA x)_a], tb = tl on the lower rows, tu on the upper ones;
`model`  the kernel's algorithm on ONE instance from the scaled record (batch_polish_ref.oracle_state): the right-hand side
         in the caller's units, scaled; the condensed regularised matrix, Cholesky, refinement against the unregularised
         system, back to the caller's units.

A direction d is a dict q [n], l, u [m], Px [nnz(P upper)], Ax [nnz(A)] in the order of the value arrays `ResidentBatch`
takes; a missing entry is zero.  Problems, oracle solutions and the non-degeneracy rule are those of batch_adjoint_ref.  No GPU
needed; tests/test_batch_jvp_host.py holds `exact` to finite differences and to the adjoint, and `model` to `exact`."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

import batch_adjoint_ref as adj
import batch_polish_ref as pol
from batch_adjoint_ref import FAMILIES, MIN_NONDEGENERATE, nondegenerate, oracle_solutions, problems  # noqa: F401  (shared with the tests)

TANGENTS = adj.GRADS  # ("q", "l", "u", "Px", "Ax")


def tangent_matrices(P, A, d):
    """(tP symmetric [n x n], tA [m x n]) dense, of the value tangents d["Px"], d["Ax"] (missing: zero)."""
    (pi, pj), (ai, aj) = adj.patterns(P, A)
    n, m = sp.csc_matrix(P).shape[0], sp.csc_matrix(A).shape[0]
    tP, tA = np.zeros((n, n)), np.zeros((m, n))
    if d.get("Px") is not None:
        tP[pi, pj] = d["Px"]
        tP[pj, pi] = d["Px"]
    if d.get("Ax") is not None:
        tA[ai, aj] = d["Ax"]
    return tP, tA


def rhs(P, A, x, y, act, d):
    """(rhs_x [n], rhs_a [m], zero on the inactive rows) in the caller's units."""
    n, m = len(x), len(y)
    tP, tA = tangent_matrices(P, A, d)
    zero = lambda k, w: np.zeros(w) if d.get(k) is None else np.asarray(d[k], dtype=float)
    tb = np.where(act < 0, zero("l", m), zero("u", m))
    return -(zero("q", n) + tP @ x + tA.T @ y), np.where(act != 0, tb - tA @ x, 0.0)


def exact(P, A, x, y, act, d):
    """(tx [n], ty [m]) by the dense K solve."""
    n, rows = len(x), np.flatnonzero(act)
    Aa = sp.csr_matrix(A)[rows].toarray()
    K = np.block([[adj.full_P(P), Aa.T], [Aa, np.zeros((len(rows), len(rows)))]])
    rx, ra = rhs(P, A, x, y, act, d)
    s = np.linalg.solve(K, np.concatenate([rx, ra[rows]]))
    ty = np.zeros(len(y))
    ty[rows] = s[n:]
    return s[:n], ty


def model(P, q, A, l, u, D, E, c, xs, zs, ys, d, delta=1e-6, refine=3):
    """The kernel's algorithm.  (D, E, c, xs, zs, ys): batch_polish_ref.oracle_state.  Returns dict(tx, ty, act, status (1, or -1
    on a failed Cholesky: zeros), and the caller-unit x, y of the record)."""
    n, m = len(q), len(l)
    Ps, _, As, ls, us = pol.scale_data(P, q, A, l, u, D, E, c)
    act = adj.classify(zs, ys, ls, us)
    rows = np.flatnonzero(act)
    Aa = As[rows]
    x, y = D * xs, E * ys / c
    M = (Ps + delta * sp.identity(n) + (Aa.T @ Aa) / delta).toarray()
    try:
        L = np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        return dict(tx=np.zeros(n), ty=np.zeros(m), act=np.zeros(m, int), status=-1, x=x, y=y)

    def kkt_solve(rx, ry):
        t = rx + Aa.T @ ry / delta
        dx = sla.solve_triangular(L, sla.solve_triangular(L, t, lower=True), lower=True, trans="T")
        return dx, (Aa @ dx - ry) / delta

    rx, ra = rhs(P, A, x, y, act, d)
    g, b = c * (D * rx), (E * ra)[rows]
    r, s = kkt_solve(g, b)
    for _ in range(refine):
        dr, ds = kkt_solve(g - Ps @ r - Aa.T @ s, b - Aa @ r)
        r, s = r + dr, s + ds
    ty = np.zeros(m)
    ty[rows] = s
    return dict(tx=D * r, ty=E * ty / c, act=act, status=1, x=x, y=y)


def tangents(family, ndir, probs):
    """Seeded random directions of a family: dict of [ndir x count x cols] arrays for q, l, u, Px, Ax, with tu = tl on the rows
    with l == u (an equality row moves as one).  probs: the (P, q, A, l, u) of the instances."""
    count, n, m = len(probs), len(probs[0][1]), len(probs[0][3])
    (pi, _), (ai, _) = adj.patterns(probs[0][0], probs[0][2])
    rng = np.random.default_rng(1000 + sum(map(ord, family)))
    d = {k: rng.standard_normal((ndir, count, w)) for k, w in zip(TANGENTS, (n, m, m, len(pi), len(ai)))}
    eq = np.array([p[3] == p[4] for p in probs]).reshape(count, m)
    d["u"] = np.where(eq[None], d["l"], d["u"])
    return d


def direction(d, k, i):
    """Direction k of instance i of `tangents`."""
    return {name: a[k, i] for name, a in d.items()}


def rel_err(got_x, got_y, want_x, want_y):
    """Largest difference of (tx, ty), each relative to max(1, max|want|)."""
    worst = float(np.max(np.abs(got_x - want_x))) / max(1.0, float(np.max(np.abs(want_x))))
    if len(want_y):
        worst = max(worst, float(np.max(np.abs(got_y - want_y))) / max(1.0, float(np.max(np.abs(want_y)))))
    return worst


def duality_gap(gx, gy, tx, ty, g, d):
    """|gx . tx + gy . ty - sum_k <g_k, d_k>| relative to max(1, sum |terms|): g the five adjoint gradients of (gx, gy), d the
    direction whose sensitivities are (tx, ty)."""
    lhs = np.concatenate([gx * tx, gy * ty])
    rhs_terms = np.concatenate([np.asarray(g[k]) * np.asarray(d[k]) for k in TANGENTS if d.get(k) is not None])
    return abs(float(lhs.sum()) - float(rhs_terms.sum())) / max(1.0, float(np.abs(lhs).sum() + np.abs(rhs_terms).sum()))
