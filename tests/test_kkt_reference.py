"""The host reference of the direct back-end's KKT solve (kkt_reference.py) on its own, no GPU: a correct solve passes the
bounds the GPU tests hold every form to, and a solve of a matrix that differs from the reference's in one place -- rho 1 %
off on one row, one entry of P changed by 1e-6 relative, an A that an update did not reach -- fails them."""
import numpy as np
import pytest
import scipy.sparse as sp

import kkt_reference as kr


def _problem():
    """Inequality, equality and free rows; P with off-diagonal entries."""
    rng = np.random.default_rng(3)
    n, m = 40, 50
    M = sp.random(n, n, density=0.1, random_state=rng, data_rvs=rng.standard_normal)
    P = sp.triu((M @ M.T + 0.1 * sp.eye(n)).tocsc(), format="csc")
    A = sp.random(m, n, density=0.15, random_state=rng, data_rvs=rng.standard_normal, format="csc")
    l = -rng.random(m) - 0.1
    u = rng.random(m) + 0.1
    u[:10] = l[:10]
    l[10:15], u[10:15] = -np.inf, np.inf
    return P, A, l, u, rng.standard_normal(n + m)


def _solve(ref, b):
    """What op 3 returns for the reference's matrix, by a dense solve (not the reference's own SuperLU)."""
    w = np.linalg.solve(ref.K.toarray(), b)
    return np.concatenate([w[:ref.n], b[ref.n:] + w[ref.n:] / ref.rho])


def test_rho_vector_follows_the_engine_rule():
    l = np.array([-1.0, 2.0, -np.inf, -np.inf, -2e26, 0.0, 1.0])
    u = np.array([1.0, 2.0 + 5e-5, np.inf, 3.0, 2e26, 1e-4, np.inf])
    assert list(kr.row_classes(l, u)) == [0, 1, -1, 0, -1, 0, 0]
    assert np.array_equal(kr.rho_vector(l, u, 0.5), [0.5, 500.0, 1e-6, 0.5, 1e-6, 0.5, 0.5])
    assert np.array_equal(kr.rho_vector(l, u, 1e9), [1e6, 1e9, 1e-6, 1e6, 1e-6, 1e6, 1e6])  # (rho clipped to RHO_MAX)


def test_a_correct_solve_passes():
    P, A, l, u, b = _problem()
    ref = kr.Reference(P, A, kr.rho_vector(l, u, 0.731))
    e = ref.check(b, _solve(ref, b), kr.BACKWARD, kr.IDENTITY, kr.FORWARD)
    assert e["backward"] < 1e-13 and e["identity"] < 1e-13 and e["forward"] < 1e-12, e
    Pf = (P + sp.triu(P, 1).T).toarray()
    assert np.array_equal(ref.Pf.toarray(), Pf)  # the full P from the upper triangle, also when given in full
    assert np.array_equal(kr.Reference(sp.csc_matrix(Pf), A, ref.rho).K.toarray(), ref.K.toarray())


def test_condition_estimate_is_the_componentwise_condition():
    """cond(K, w) of (a') against its dense definition || |K^-1| (|K| |w| + |b|) ||_inf / ||w||_inf; a correct solve passes (a')."""
    P, A, l, u, b = _problem()
    ref = kr.Reference(P, A, kr.rho_vector(l, u, 0.731))
    out = _solve(ref, b)
    w = ref.w(b, out)
    Kd = ref.K.toarray()
    exact = np.max(np.abs(np.linalg.inv(Kd)) @ (np.abs(Kd) @ np.abs(w) + np.abs(b))) / np.max(np.abs(w))
    est = ref.condition(b, out)
    assert exact / 3 <= est <= exact * (1 + 1e-9), (est, exact)
    e = ref.check(b, out, kr.BACKWARD, kr.IDENTITY, kr.FORWARD, by_condition=True)
    assert e["forward_w"] <= 1e-3 * e["condition"] * kr.BACKWARD, e


def test_no_constraints():
    P, _, _, _, b = _problem()
    n = P.shape[0]
    ref = kr.Reference(P, sp.csc_matrix((0, n)), np.zeros(0))
    ref.check(b[:n], _solve(ref, b[:n]), kr.BACKWARD, kr.IDENTITY, kr.FORWARD)


@pytest.mark.parametrize("fault", ["rho-off-on-one-row", "P-entry-off-by-1e-6", "stale-A"])
def test_a_solve_of_another_matrix_fails(fault):
    """The solve is of the problem's K; the reference is built from data that differ in one place."""
    P, A, l, u, b = _problem()
    rho = kr.rho_vector(l, u, 0.731)
    out = _solve(kr.Reference(P, A, rho), b)
    if fault == "rho-off-on-one-row":
        rho2 = rho.copy()
        rho2[20] *= 1.01
        ref = kr.Reference(P, A, rho2)
    elif fault == "P-entry-off-by-1e-6":
        P2 = P.copy()
        off = np.flatnonzero(P2.indices != np.repeat(np.arange(P2.shape[1]), np.diff(P2.indptr)))
        P2.data[off[np.argmax(np.abs(P2.data[off]))]] *= 1.0 + 1e-6
        ref = kr.Reference(P2, A, rho)
    else:
        A2 = A.copy()
        A2.data *= 1.0 + 0.3 * np.random.default_rng(4).uniform(-1.0, 1.0, A2.nnz)
        ref = kr.Reference(P, A2, rho)
    e = ref.errors(b, out, conditioned=True)
    assert e["backward"] > 1e3 * kr.BACKWARD, e  # far beyond the bound, not just over it
    assert e["forward_w"] > 10 * e["condition"] * kr.BACKWARD, e  # (a') too
    if fault == "stale-A":
        assert e["identity"] > 1e3 * kr.IDENTITY, e
    for by_condition in (False, True):
        with pytest.raises(AssertionError):
            ref.check(b, out, kr.BACKWARD, kr.IDENTITY, kr.FORWARD, by_condition=by_condition)
