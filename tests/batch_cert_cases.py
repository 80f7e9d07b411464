"""Infeasible instances for the certificate tests of the resident batch, and the checker of a certificate against the
definitions.  Two families; in both every group of three consecutive instances is solvable, primal infeasible, dual
infeasible, in that order (`kind(i)` = i % 3).

chain(n, extra, dense), instance i from default_rng(100 + i):
  A: rows 0 .. n-1 the identity (box rows, value 1), row n + k (k < extra) entries in columns {k, k+1, k+2} mod n, with
     `dense` one more row with an entry in every column; the other values N(0, 1), drawn row by row.
  P: tridiagonal on a FIXED pattern (explicit zeros stay): diagonal 1 + U(0, 1), off-diagonal 0.1 N(0, 1).
  q: N(0, 1); l = -1, u = 1.   (draw order: A, diagonal, off-diagonal, q)
  primal infeasible: l[n] = sum |A[n, :]| + 1, u[n] = l[n] + 1 -- out of reach of the box |x| <= 1;
  dual infeasible:   P[0, 0] = P[0, 1] = 0, q[0] = -1, bounds -+1e30 on every row that touches variable 0 -- e_0 is a
                     direction of unbounded descent.
mpc: batch_resident_ref.mpc_instances(oracle_lib, 0, count, 2);
  primal infeasible: l[60] = u[60] = 1000 (the first box row; the recipe of test_batch_polish_gpu.py);
  dual infeasible:   Px = 0 and q = 0 at variables 90 .. 96, q[96] = -1, bounds -+1e30 on their box rows 150 .. 156 and on
                     rate row 196 -- the first input of the last stage, and the state it moves, cost nothing and are free.
No GPU needed: tests/test_batch_cert_host.py holds both families and the checker to the oracle."""
import numpy as np
import scipy.sparse as sp

import batch_resident_ref as ref

OPTS = ref.OPTS
VARIANTS = [dict(), dict(scaling=0), dict(scaled_termination=1)]
INF = 1e30
EPS = float(np.finfo(float).eps)
PRIM, DUAL = (-3, 3), (-4, 4)


def kind(i):
    """0 solvable, 1 primal infeasible, 2 dual infeasible."""
    return i % 3


def chain_patterns(n, extra, dense=False):
    """(pattern of triu(P), pattern of A) as CSC matrices of ones with sorted indices."""
    rows = list(range(n)) + [n + k for k in range(extra) for _ in range(3)] + ([n + extra] * n if dense else [])
    cols = list(range(n)) + [(k + d) % n for k in range(extra) for d in range(3)] + (list(range(n)) if dense else [])
    A = sp.csc_matrix((np.ones(len(rows)), (rows, cols)), shape=(n + extra + (1 if dense else 0), n))
    P = sp.csc_matrix(sp.triu(sp.diags([np.ones(n), np.ones(n - 1)], [0, 1]), format="csc"))
    A.sort_indices(); P.sort_indices()
    return P, A


def chain(n, extra, dense=False, count=6, first_seed=100):
    """[(P upper triangle, q, A, l, u)] of `count` instances, seeds first_seed, first_seed + 1, ..."""
    patP, patA = chain_patterns(n, extra, dense)
    m = patA.shape[0]
    probs = []
    for i in range(count):
        rng = np.random.default_rng(first_seed + i)
        D = np.zeros((m, n))
        D[np.arange(n), np.arange(n)] = 1.0
        for k in range(extra):
            D[n + k, [(k + d) % n for d in range(3)]] = rng.standard_normal(3)
        if dense:
            D[n + extra, :] = rng.standard_normal(n)
        diag, off = 1.0 + rng.random(n), 0.1 * rng.standard_normal(n - 1)
        q = rng.standard_normal(n)
        l, u = -np.ones(m), np.ones(m)
        if kind(i) == 1:
            l[n] = float(np.sum(np.abs(D[n]))) + 1.0
            u[n] = l[n] + 1.0
        if kind(i) == 2:
            diag[0] = 0.0; off[0] = 0.0; q[0] = -1.0
            touch = np.flatnonzero(patA.tocsr()[:, 0].toarray().ravel())
            l[touch], u[touch] = -INF, INF
        A = patA.copy()
        A.data = D[patA.indices, np.repeat(np.arange(n), np.diff(patA.indptr))]
        Pd = np.zeros((n, n))
        Pd[np.arange(n), np.arange(n)] = diag
        Pd[np.arange(n - 1), np.arange(1, n)] = off
        P = patP.copy()
        P.data = Pd[patP.indices, np.repeat(np.arange(n), np.diff(patP.indptr))]  # explicit zeros kept
        probs.append((P, q, A, l, u))
    return probs


def mpc(oracle_lib, count=8):
    probs = []
    for i, (P, q, A, l, u) in enumerate(ref.mpc_instances(oracle_lib, 0, count, 2)):
        P = sp.csc_matrix(P); q, l, u = q.copy(), l.copy(), u.copy()
        assert P.nnz == 100 and np.array_equal(P.indices, np.arange(100))  # diagonal: data[j] is P[j, j]
        if kind(i) == 1:
            l[60] = u[60] = 1000.0
        if kind(i) == 2:
            P.data[90:97] = 0.0  # explicit zeros kept
            q[90:97] = 0.0; q[96] = -1.0
            free = list(range(150, 157)) + [196]
            l[free], u[free] = -INF, INF
        probs.append((P, q, A, l, u))
    return probs


def stack(probs):
    """`batch_resident_ref.stack` for these families: their P is the upper triangle on a fixed pattern that may hold
    explicit zeros, so the values are taken as stored."""
    P0, _, A0, _, _ = probs[0]
    for P, _, A, _, _ in probs:
        assert np.array_equal(P.indices, P0.indices) and np.array_equal(P.indptr, P0.indptr)
        assert np.array_equal(A.indices, A0.indices) and np.array_equal(A.indptr, A0.indptr)
    patP, patA = P0.copy(), A0.copy()
    patP.data = np.ones(patP.nnz); patA.data = np.ones(patA.nnz)
    return (patP, patA, np.array([p[0].data for p in probs]), np.array([p[2].data for p in probs]),
            np.array([p[1] for p in probs]), np.array([p[3] for p in probs]), np.array([p[4] for p in probs]))


def slack(k, S):
    """Rounding bound of a sum of k products of magnitude <= S evaluated on scaled data and undone by factors that cancel up
    to a rounding each: the form of test_batch_polish_gpu.py, 16 (k + 8) eps S."""
    return 16 * (k + 8) * EPS * S


def check_primal(v, prob, eps, tag=""):
    """The criteria of a certificate of primal infeasibility, from the raw data: normalised, signs where a bound is missing,
    |A'v|_inf < eps, u'v+ + l'v- < -eps (|v|_inf = 1).  Returns the two figures."""
    P, q, A, l, u = prob
    A = sp.csc_matrix(A)
    assert np.all(np.isfinite(v)) and float(np.max(np.abs(v))) == 1.0, (tag, float(np.max(np.abs(v))))
    assert np.all(v[u >= INF] <= 0.0) and np.all(v[l <= -INF] >= 0.0), tag
    atv = float(np.max(np.abs(A.T @ v)))
    b = slack(int(np.max(np.diff(A.indptr))), float(np.max(np.abs(A.data))))
    fu, fl = u < INF, l > -INF
    support = float(np.sum(u[fu] * np.maximum(v[fu], 0.0)) + np.sum(l[fl] * np.minimum(v[fl], 0.0)))
    bounds = np.concatenate([np.abs(u[fu]), np.abs(l[fl])])
    b2 = slack(len(v), float(np.max(bounds)) if len(bounds) else 0.0)
    print(f"{tag} primal: |A'v| {atv:.3e} (< {eps:.1e} + {b:.1e})  support {support:.3e} (< -{eps:.1e} + {b2:.1e})")
    assert atv < eps + b, (tag, atv)
    assert support < -eps + b2, (tag, support)
    return atv, support


def check_dual(v, prob, eps, tag=""):
    """The criteria of a certificate of dual infeasibility: normalised, q'v < -eps, |Pv|_inf < eps, (Av)_i < eps where u_i
    is finite and > -eps where l_i is finite."""
    P, q, A, l, u = prob
    U = sp.triu(sp.csc_matrix(P), format="csc")
    Pf, A = (U + sp.triu(U, 1).T).tocsr(), sp.csr_matrix(A)
    assert np.all(np.isfinite(v)) and float(np.max(np.abs(v))) == 1.0, (tag, float(np.max(np.abs(v))))
    qv = float(q @ v)
    pv = float(np.max(np.abs(Pf @ v)))
    av = A @ v
    bq = slack(len(q), float(np.max(np.abs(q))))
    bp = slack(int(np.max(np.diff(Pf.indptr))), float(np.max(np.abs(Pf.data))) if Pf.nnz else 0.0)
    ba = slack(int(np.max(np.diff(A.indptr))), float(np.max(np.abs(A.data))))
    hi = float(np.max(av[u < INF], initial=-np.inf)); lo = float(np.min(av[l > -INF], initial=np.inf))
    print(f"{tag} dual: q'v {qv:.3e} (< -{eps:.1e} + {bq:.1e})  |Pv| {pv:.3e} (< {eps:.1e} + {bp:.1e})  Av in [{lo:.3e}, {hi:.3e}]")
    assert qv < -eps + bq, (tag, qv)
    assert pv < eps + bp, (tag, pv)
    assert hi < eps + ba and lo > -eps - ba, (tag, lo, hi)
    return qv, pv


def check_certificate(status, pcert, dcert, prob, opts, tag=""):
    """The certificate that belongs to `status` against the criteria, with the eps of `opts` (settings defaults 1e-4), ten
    times that for an inaccurate status."""
    relax = 10.0 if status in (3, 4) else 1.0
    if status in PRIM:
        return check_primal(pcert, prob, relax * opts.get("eps_prim_inf", 1e-4), tag)
    assert status in DUAL, status
    return check_dual(dcert, prob, relax * opts.get("eps_dual_inf", 1e-4), tag)
