"""Numpy model of the polish step of the resident batch (k_batch_polish in osqp.jl_amd/csrc/batch_polish.hpp): the
oracle's polish() on ONE instance in the scaled space, with the regularised KKT system in its condensed form

    M = P + delta I + (1 / delta) A_act' A_act          (n x n, symmetric positive definite, Cholesky)
    d_x = M^-1 (r_x + A_act' r_y / delta),   d_y = (A_act d_x - r_y) / delta

which is the exact elimination of the constraint block of [P + delta I, A_act'; A_act, -delta I].  The refinement steps run
against the unregularised matrix [P, A_act'; A_act, 0], as the oracle's do.  Multipliers are kept as a full m-vector (zero on
inactive rows) instead of the oracle's packed [lower; upper] order: the order only permutes the system.

No GPU needed; tests/test_batch_polish_host.py holds this model to the oracle, the GPU tests hold the kernel to the oracle."""
import ctypes as C

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

OSQP_INFTY = 1e30


class _Scaling(C.Structure):  # oracle/osqp_oracle.c scaling_t
    _fields_ = [("c", C.c_double), ("cinv", C.c_double), ("D", C.POINTER(C.c_double)), ("Dinv", C.POINTER(C.c_double)),
                ("E", C.POINTER(C.c_double)), ("Einv", C.POINTER(C.c_double))]


def oracle_state(model, n, m, scaling):
    """(D, E, c, x, z, y) of an oracle model after a solve: its scaling factors and its SCALED iterate."""
    w = model.workspace.contents
    vec = lambda p, k: np.array([p[i] for i in range(k)], dtype=float)
    if scaling:
        s = C.cast(w.scaling, C.POINTER(_Scaling)).contents
        D, E, c = vec(s.D, n), vec(s.E, m), float(s.c)
    else:
        D, E, c = np.ones(n), np.ones(m), 1.0
    return D, E, c, vec(w.x, n), vec(w.z, m), vec(w.y, m)


def scale_data(P, q, A, l, u, D, E, c):
    """The raw data of an instance under the stored factors, as the solve kernels' prologue applies them: P <- c D P D
    (full symmetric), A <- E A D, q <- c D q, bounds clipped at +-OSQP_INFTY and then times E."""
    U = sp.triu(sp.csc_matrix(P), format="csc")
    F = (U + sp.triu(U, 1).T).tocsr()
    Ps = sp.diags(D) @ F @ sp.diags(D) * c
    As = sp.diags(E) @ sp.csr_matrix(A) @ sp.diags(D)
    return Ps.tocsr(), c * (D * q), As.tocsr(), np.maximum(l, -OSQP_INFTY) * E, np.minimum(u, OSQP_INFTY) * E


def residuals(Ps, qs, As, x, z, y, D, E, c, unscaled):
    """pri_res, dua_res, obj_val of a scaled iterate by the definitions of the termination check (`unscaled`: scaling on and
    scaled_termination off)."""
    rp = As @ x - z
    rd = Ps @ x + qs + As.T @ y
    if unscaled:
        pri = float(np.max(np.abs(rp / E))) if len(rp) else 0.0
        dua = float(np.max(np.abs(rd / D))) / c
    else:
        pri = float(np.max(np.abs(rp))) if len(rp) else 0.0
        dua = float(np.max(np.abs(rd)))
    obj = float(0.5 * x @ (Ps @ x) + qs @ x) / c
    return pri, dua, obj


def polish(P, q, A, l, u, D, E, c, x, z, y, pri_res, dua_res, delta=1e-6, refine=3, unscaled=True):
    """Polish one Solved instance.  (x, z, y): the scaled ADMM iterate; pri_res / dua_res: what the solve reported.
    Returns dict(status = 1 | -1, x, y (caller's units), xs, zs, ys (scaled), pri_res, dua_res, obj_val); on status -1
    the iterate entries are the inputs."""
    n, m = len(q), len(l)
    Ps, qs, As, ls, us = scale_data(P, q, A, l, u, D, E, c)
    low = (z - ls) < -y
    upp = ~low & ((us - z) < y)
    act = low | upp
    b = np.where(low, ls, us)[act]
    Aa = As[np.flatnonzero(act)]
    refused = dict(status=-1, x=D * x, y=E * y / c, xs=x, zs=z, ys=y, pri_res=pri_res, dua_res=dua_res, obj_val=None)
    M = (Ps + delta * sp.identity(n) + (Aa.T @ Aa) / delta).toarray()
    try:
        L = np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        return refused

    def kkt_solve(rx, ry):
        t = rx + Aa.T @ ry / delta
        dx = sla.solve_triangular(L, sla.solve_triangular(L, t, lower=True), lower=True, trans="T")
        return dx, (Aa @ dx - ry) / delta

    xp, ya = kkt_solve(-qs, b)
    for _ in range(refine):
        dx, dy = kkt_solve(-qs - Ps @ xp - Aa.T @ ya, b - Aa @ xp)
        xp, ya = xp + dx, ya + dy
    yp = np.zeros(m)
    yp[act] = ya
    s = As @ xp + yp
    zp = np.minimum(np.maximum(s, ls), us)
    yp = s - zp
    pri, dua, obj = residuals(Ps, qs, As, xp, zp, yp, D, E, c, unscaled)
    ok = (pri < pri_res and dua < dua_res) or (pri < pri_res and dua_res < 1e-10) or (dua < dua_res and pri_res < 1e-10)
    if not ok:
        return refused
    return dict(status=1, x=D * xp, y=E * yp / c, xs=xp, zs=zp, ys=yp, pri_res=pri, dua_res=dua, obj_val=obj)
