"""Inputs of the duality tests (test_duality_host.py, test_duality_gpu.py; not a test module): the value cases, and the
cases on which the gap stopping rule changes where a solve ends, with the CPU procedure that finds where -- the oracle's
iterates and the numpy statement of the gap (duality_ref.py), never the engine under test."""
import functools

import numpy as np
import scipy.sparse as sp

import duality_ref
import qp_zoo

RULE_EPS = 1e-3
RULE_SETTINGS = dict(verbose=False, eps_abs=RULE_EPS, eps_rel=RULE_EPS, adaptive_rho_interval=25)
CHECK = 25        # check_termination of the default settings
MAX_CHECKS = 16   # how far past K_off the procedure looks for K_on


def small_free():
    """12 variables, 10 rows of every bound kind: free rows (both infinite, as +-inf and as +-1e30), rows with only the upper or
    only the lower bound infinite (again both spellings), an equality, two-sided rows.  P positive definite: bounded."""
    rng = np.random.default_rng(41)
    n, m = 12, 10
    M = rng.standard_normal((n, n))
    P = sp.csc_matrix(sp.triu(M @ M.T / n + 0.5 * np.eye(n)))
    q = rng.standard_normal(n)
    A = sp.random(m, n, density=0.4, random_state=rng, data_rvs=rng.standard_normal, format="csc")
    A = (A + sp.csc_matrix((np.ones(m), (np.arange(m), np.arange(m))), shape=(m, n))).tocsc()  # no empty row
    inf = np.inf
    l = np.array([-inf, -1e30, -inf, -1e30, -0.3, 0.1, 0.2, -0.5, -0.2, -1.0])
    u = np.array([inf, 1e30, 0.2, -0.1, inf, 1e30, 0.2, 0.5, 0.1, 1.0])
    return dict(P=P, q=q, A=A, l=l, u=u)


def unconstrained():
    """7 variables, m = 0."""
    rng = np.random.default_rng(42)
    n = 7
    M = rng.standard_normal((n, n))
    P = sp.csc_matrix(sp.triu(M @ M.T / n + 0.3 * np.eye(n)))
    return dict(P=P, q=rng.standard_normal(n), A=sp.csc_matrix((0, n)), l=np.zeros(0), u=np.zeros(0))


VALUE_CASES = {
    "portfolio": lambda: qp_zoo.portfolio(n=300, k=10),
    "huber": lambda: qp_zoo.huber(n=20, m=200),
    "svm": lambda: qp_zoo.svm(n=20, m=200),
    "control": lambda: qp_zoo.control(nx=4, nu=2, T=10),
    "small_free": small_free,
    "unconstrained": unconstrained,
}
ZOO_VALUE_CASES = ("portfolio", "huber", "svm", "control")
POLISHED = ("portfolio", "control")

# name -> (problem, extra settings)
RULE_CASES = {
    "portfolio_scaled": (VALUE_CASES["portfolio"], dict(scaling=10)),
    "portfolio_unscaled": (VALUE_CASES["portfolio"], dict(scaling=0)),
    "huber": (VALUE_CASES["huber"], dict()),
}


def upper(prob):
    """The problem with P as its upper triangle (what setup takes)."""
    return dict(prob, P=sp.triu(prob["P"], format="csc"))


def oracle_solve(oq, oracle_lib, prob, **settings):
    m = oq.Model(oracle_lib)
    oq.setup(m, **upper(prob), **settings)
    r = oq.solve(m)
    out = (r.info.status, int(r.info.iter), np.array(r.x, dtype=float), np.array(r.y, dtype=float))
    oq.clean(m)
    return out


_traces = {}


def rule_trace(oq, oracle_lib, name):
    """The CPU procedure: K_off = where the oracle stops on the residuals alone; for every check k from K_off on, the oracle's
    iterate after exactly k iterations (max_iter = k, eps = 1e-14: nothing stops it, adaptive rho does not look at eps) and its
    ratios at RULE_EPS in numpy; K_on = the first k whose gap ratio is below 1.  Returns dict(K_off, K_on, checks = {k:
    dict(pri, dua, gap, x, y)}).  Computed once per session."""
    if name in _traces:
        return _traces[name]
    make, extra = RULE_CASES[name]
    prob = make()
    status, K_off, _, _ = oracle_solve(oq, oracle_lib, prob, **RULE_SETTINGS, **extra)
    assert status == "Solved" and K_off % CHECK == 0, (status, K_off)
    checks, K_on = {}, None
    for k in range(K_off, K_off + CHECK * MAX_CHECKS, CHECK):
        settings = dict(RULE_SETTINGS, eps_abs=1e-14, eps_rel=1e-14, max_iter=k, **extra)
        st, it, x, y = oracle_solve(oq, oracle_lib, prob, **settings)
        assert st == "Max_iter_reached" and it == k, (st, it, k)
        pri, eps_pri, dua, eps_dua = qp_zoo.kkt_check(prob, x, y, RULE_EPS)
        checks[k] = dict(pri=pri / eps_pri, dua=dua / eps_dua, gap=duality_ref.gap_ratio(prob, x, y, RULE_EPS), x=x, y=y)
        if checks[k]["gap"] < 1.0:
            K_on = k
            break
    _traces[name] = dict(prob=prob, extra=extra, K_off=K_off, K_on=K_on, checks=checks)
    return _traces[name]
