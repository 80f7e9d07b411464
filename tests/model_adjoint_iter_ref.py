"""Numpy / scipy statement of the iterative KKT solve behind osqp_amd_adjoint / osqp_amd_jvp under
osqp_amd_derivative_method (csrc/pcg.hip: kkt_iter_solve).

`kkt_iter`       [P~, A~a'; A~a, 0] [s_x; s_a] = [b1; b2] on scaled data: Jacobi-preconditioned conjugate gradients on the
                 condensed operator P~ + d I + A~' diag(mask / d) A~ with d = max(delta, 1e-3), relative tolerance 1e-6 on
                 ||residual||inf, start vector zero, at most 2000 iterations; s_a = mask (A~ s_x - r2) / d; outer steps on the
                 residual of the UNREGULARISED system, stopped when rn = ||r1 + A~' (mask / d) r2||inf has dropped by rel_drop
                 against the first step's, after more than `refine` steps, at most `max_outer`.  The constants and the stopping
                 rule are the library's.
`adjoint_model`  the five gradients, caller units, from the oracle's scaled state (the arguments of model_adjoint_ref.model).
`jvp_model`      (tx, ty) likewise (the arguments of model_jvp_ref.model).

No GPU needed; tests/test_model_adjoint_iter_host.py holds both to the dense solves `exact`."""
import numpy as np
import scipy.sparse as sp

import batch_adjoint_ref as adj
import batch_jvp_ref as jv
import batch_polish_ref as pol

DELTA_IN_MIN, CG_REL_TOL, CG_MAX_ITER, MAX_OUTER, REL_DROP = 1e-3, 1e-6, 2000, 40, 1e-10


def kkt_iter(Ps, As, side, b1, b2, delta=1e-6, refine=3, max_outer=MAX_OUTER, rel_drop=REL_DROP):
    """Returns (s_x [n], s_y [m], dict(converged, outer, cg, drop)).  side [m]: non-zero on the active rows."""
    Ps, As = sp.csr_matrix(Ps), sp.csr_matrix(As)
    n, m = len(b1), len(b2)
    d = max(delta, DELTA_IN_MIN)
    mask = np.asarray(side) != 0
    rho = np.where(mask, 1.0 / d, 0.0)
    At = As.T.tocsr()
    dinv = 1.0 / (d + Ps.diagonal() + (At.multiply(At) @ rho if m else 0.0))

    def apply_M(v):
        return Ps @ v + d * v + At @ (rho * (As @ v))

    sx, sy = np.zeros(n), np.zeros(m)
    first, rn, steps, cg_total, ok = -1.0, 0.0, 0, 0, False
    for step in range(max_outer):
        r1 = b1 - (Ps @ sx + At @ sy) if step else np.array(b1, dtype=float)
        r2 = np.where(mask, b2 - As @ sx if step else b2, 0.0)
        rhs = r1 + At @ (rho * r2)
        rn = float(np.max(np.abs(rhs))) if n else 0.0
        tol = CG_REL_TOL * rn + 1e-300
        x, r = np.zeros(n), rhs.copy()
        z = dinv * r
        p, rz, it = z.copy(), float(r @ z), 0
        failed = False
        while it < CG_MAX_ITER and float(np.max(np.abs(r))) > tol:
            w = apply_M(p)
            pw = float(p @ w)
            if not pw > 0.0:
                failed = True
                break
            alpha = rz / pw
            x += alpha * p
            r -= alpha * w
            z = dinv * r
            rz_new = float(r @ z)
            p = z + (rz_new / rz) * p
            rz = rz_new
            it += 1
        cg_total += it
        if failed:
            break
        sx = sx + x
        sy = sy + np.where(mask, (As @ x - r2) / d, 0.0)
        steps += 1
        if first < 0.0:
            first = rn
        if step >= refine and rn <= rel_drop * first:
            ok = True
            break
    drop = rn / first if first > 0.0 else (0.0 if first == 0.0 else 1.0)
    return sx, sy, dict(converged=ok, outer=steps, cg=cg_total, drop=drop)


def adjoint_model(P, q, A, l, u, D, E, c, xs, zs, ys, gx, gy, delta=1e-6, refine=3, **kw):
    """The library's iterative adjoint.  Returns the five gradients, "act", the caller-unit "x", "y" and "info" of kkt_iter."""
    Ps, _, As, ls, us = pol.scale_data(P, q, A, l, u, D, E, c)
    act = adj.classify(zs, ys, ls, us)
    sx, sy, info = kkt_iter(Ps, As, act, c * (D * gx), E * gy, delta, refine, **kw)
    x, y = D * xs, E * ys / c
    out = adj.table(P, A, x, y, act, D * sx, E * sy / c)
    out.update(act=act, x=x, y=y, info=info)
    return out


def jvp_model(P, q, A, l, u, D, E, c, xs, zs, ys, d, delta=1e-6, refine=3, **kw):
    """The library's iterative JVP.  d: a direction in the sorted order.  Returns dict(tx, ty, act, x, y, info)."""
    Ps, _, As, ls, us = pol.scale_data(P, q, A, l, u, D, E, c)
    act = adj.classify(zs, ys, ls, us)
    x, y = D * xs, E * ys / c
    rx, ra = jv.rhs(P, A, x, y, act, d)
    sx, sy, info = kkt_iter(Ps, As, act, c * (D * rx), E * ra, delta, refine, **kw)
    return dict(tx=D * sx, ty=E * sy / c, act=act, x=x, y=y, info=info)
