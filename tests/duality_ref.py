"""The numpy statement of the dual objective and the duality gap (the definitions the engine, the batch
kernel and the header share), from the caller's data and a pair (x, y):

  yh       = y projected onto the polar of the recession cone of [l, u]: 0 where both bounds are infinite, min(y, 0) where
             only u is, max(y, 0) where only l is, y otherwise
  SC       = sum_i u_i max(yh_i, 0) + l_i min(yh_i, 0)        (an infinite bound contributes 0; 0 when m = 0)
  prim_obj = 1/2 x'Px + q'x      dual_obj = -1/2 x'Px - SC      gap = x'Px + q'x + SC
  eps_gap  = eps_abs + eps_rel max(|x'Px|, |q'x|, |SC|)

The kernels call a bound infinite when the SCALED bound passes OSQP_INFTY * MIN_SCALING = 1e26 in magnitude (the row factors
of the equilibration lie in [1e-4, 1e4]).  Here the test is on the caller's bound against the same 1e26: the two agree
for every finite bound below 1e22 in magnitude and every bound at +-1e30 or beyond, which is all the tests use.

Sums are taken in extended precision (math.fsum), so the rounding of this side is one ulp of the result."""
import math

import numpy as np
import scipy.sparse as sp

INF_BOUND = 1e30 * 1e-4


def full_P(P):
    """The full symmetric matrix from either form (upper triangle or full), as qp_zoo.kkt_check reads it."""
    P = sp.csc_matrix(P)
    return P if sp.tril(P, -1).nnz > 0 else (P + sp.triu(P, 1).T).tocsc()


def project(y, l, u):
    """yh: y on the polar of the recession cone of [l, u]; y is not modified."""
    y, l, u = (np.asarray(a, dtype=float) for a in (y, l, u))
    u_inf, l_inf = u > INF_BOUND, l < -INF_BOUND
    yh = y.copy()
    yh[u_inf & l_inf] = 0.0
    only_u = u_inf & ~l_inf
    yh[only_u] = np.minimum(y[only_u], 0.0)
    only_l = l_inf & ~u_inf
    yh[only_l] = np.maximum(y[only_l], 0.0)
    return yh


def duality(P, q, A, l, u, x, y, eps_abs=0.0, eps_rel=0.0):
    """dict(prim_obj, dual_obj, gap, xPx, qx, SC, eps_gap, S): S = the sum of the absolute values of every term of the three
    sums (|x_i P_ij x_j|, |q_i x_i|, |u_i yh_i+|, |l_i yh_i-|), the scale of their rounding errors; N = n + nnz(P full) + 2 m
    the number of terms."""
    Pf = full_P(P).tocoo()
    x, q = np.asarray(x, dtype=float), np.asarray(q, dtype=float)
    l, u, y = (np.asarray(a, dtype=float).ravel() for a in (l, u, y))
    m = len(l)
    t_p = x[Pf.row] * Pf.data * x[Pf.col]
    t_q = q * x
    if m:
        yh = project(y, l, u)
        up, lo = np.maximum(yh, 0.0), np.minimum(yh, 0.0)
        t_u = np.where(u > INF_BOUND, 0.0, u) * up  # an infinite bound contributes 0 (yh is 0 on its side anyway)
        t_l = np.where(l < -INF_BOUND, 0.0, l) * lo
    else:
        t_u = t_l = np.zeros(0)
    xPx, qx = math.fsum(t_p), math.fsum(t_q)
    SC = math.fsum(np.concatenate([t_u, t_l]))
    S = math.fsum(np.abs(np.concatenate([t_p, t_q, t_u, t_l])))
    return dict(prim_obj=0.5 * xPx + qx, dual_obj=-0.5 * xPx - SC, gap=xPx + qx + SC, xPx=xPx, qx=qx, SC=SC,
                eps_gap=eps_abs + eps_rel * max(abs(xPx), abs(qx), abs(SC)), S=S, N=len(x) + Pf.nnz + 2 * m)


def tolerance(d):
    """4 (N + 8) 2^-53 S: the dot-product rounding bound of both sides (N terms summed in some order on the device, one
    rounding here) plus the handful of roundings the scaling factors put on every term (x = D x~, y = E y~ / c, the stored
    c D P D, the final 1 / c).  Derived, not measured."""
    return 4.0 * (d["N"] + 8) * 2.0 ** -53 * d["S"]


def gap_ratio(prob, x, y, eps):
    """|gap| / eps_gap at eps_abs = eps_rel = eps."""
    d = duality(prob["P"], prob["q"], prob["A"], prob["l"], prob["u"], x, y, eps, eps)
    return abs(d["gap"]) / d["eps_gap"]
