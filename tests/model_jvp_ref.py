"""Numpy reference of the forward sensitivities of a single model (osqp_amd_jvp, osqp.jl_amd/csrc/direct_jvp.hpp).

`model`  the library's algorithm on one problem from the oracle's scaled state, as model_adjoint_ref.model has it for the
         adjoint: the classification of the rows, lower rows first, the FULL regularised matrix
         [P~ + delta I, A~a'; A~a, -delta I] solved densely, `refine` steps against the unregularised matrix, back to the
         caller's units.  The right-hand side is batch_jvp_ref.rhs (the caller's units), scaled: [c D rhs_x; (E rhs_a)_a].
`exact`  is batch_jvp_ref.exact: the mathematics in the caller's units.

The cases, their problems and their oracle solutions are model_adjoint_ref's; the seeded directions are here.  A direction
is a dict q [n], l, u [m], Px [nnz(P upper)], Ax [nnz(A)] in the CALLER's nnz order; `reference_direction` translates Ax into
the sorted CSC order the references work in (control6_unsorted).  No GPU needed; tests/test_model_jvp_host.py holds `model`
to `exact`."""
import numpy as np
import scipy.linalg as sla

import batch_adjoint_ref as adj
import batch_jvp_ref as jv
import batch_polish_ref as pol
import model_adjoint_ref as mar

TANGENTS = jv.TANGENTS


def model(P, q, A, l, u, D, E, c, xs, zs, ys, d, delta=1e-6, refine=3):
    """The library's algorithm.  d: a direction in the sorted order.  Returns dict(tx, ty, act, x, y)."""
    n, m = len(q), len(l)
    Ps, _, As, ls, us = pol.scale_data(P, q, A, l, u, D, E, c)
    act = adj.classify(zs, ys, ls, us)
    rows = np.concatenate([np.flatnonzero(act < 0), np.flatnonzero(act > 0)])  # lower rows first: the order of the reduced matrix
    mr = len(rows)
    Aa = As[rows].toarray().reshape(mr, n)
    K0 = np.block([[Ps.toarray(), Aa.T], [Aa, np.zeros((mr, mr))]])
    Kreg = K0 + np.diag(np.concatenate([delta * np.ones(n), -delta * np.ones(mr)]))
    lu = sla.lu_factor(Kreg)
    x, y = D * xs, E * ys / c
    rx, ra = jv.rhs(P, A, x, y, act, d)
    rhs = np.concatenate([c * (D * rx), (E * ra)[rows]])
    sol = sla.lu_solve(lu, rhs)
    for _ in range(refine):
        sol = sol + sla.lu_solve(lu, rhs - K0 @ sol)
    ty = np.zeros(m)
    ty[rows] = sol[n:]
    return dict(tx=D * sol[:n], ty=E * ty / c, act=act, x=x, y=y)


def tangents(case, k, p, ndir=1):
    """The seeded random directions of instance k of a case: dict of [ndir x cols] arrays in the caller's nnz order, with
    tu = tl on the rows with l == u (an equality row moves as one); direction 0 is the one the single-direction tests use."""
    n, m = len(p["q"]), len(p["l"])
    (pi, _), (ai, _) = adj.patterns(p["P"], p["A"])
    rng = np.random.default_rng(sum(map(ord, case)) * 137 + 1000 + k)
    d = {name: rng.standard_normal((ndir, w)) for name, w in zip(TANGENTS, (n, m, m, len(pi), len(ai)))}
    d["u"] = np.where((p["l"] == p["u"])[None], d["l"], d["u"])
    return d


def direction(d, i):
    """Direction i of `tangents`."""
    return {name: a[i] for name, a in d.items()}


def reference_direction(p, d):
    """A direction of the caller (Ax in the caller's nnz order) in the sorted CSC order of the references."""
    if "to_sorted" not in p or d.get("Ax") is None:
        return d
    ax = np.empty_like(np.asarray(d["Ax"], dtype=float))
    ax[..., p["to_sorted"]] = d["Ax"]
    return dict(d, Ax=ax)
