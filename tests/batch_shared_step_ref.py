"""The K-step reference of the shared batch (k_batch_solve_shared in osqp.jl_amd/csrc/batch_shared.hpp): K ADMM iterations
from a KNOWN state in numpy.longdouble.  After `warm_start(x0, y0)` a solve with max_iter = K and check_termination = 0 runs
exactly K iterations, stops with Max_iter_reached and returns D x_K and E y_K / c, so the whole iteration -- the matrix-core
product x~ = M^-1 b, the row phase, the un-scaling and the figures of the last check -- is compared with this model directly,
with no ADMM convergence in between.

The model of an instance (q, l, u) of a batch on the base (P, q0, A, l0, u0), from the oracle's (D, E, c) of the BASE data:
  scaled data   batch_polish_ref.scale_data;  rho per row: kkt_reference.rho_vector on the scaled BASE bounds;
  M             Ps + sigma I + As' diag(rho) As;
  start         x = x0 / D, z = E (A_raw x0), y = c y0 / E; a missing vector is zero, and z is zero when x is missing;
  iteration     b = sigma x - qs + As' (rho z - y);  x~ = M^-1 b (float64 LU, five refinement steps on longdouble residuals);
                x <- alpha x~ + (1 - alpha) x;  zh = alpha As x~ + (1 - alpha) z;  z <- clip(zh + y / rho, ls, us);
                y <- y + rho (zh - z);
  returns       D x, E y / c, pri_res, dua_res, obj_val of the last iterate by the definitions of batch_polish_ref.residuals,
                the scale of each of the three, kappa_2(M) and tau.

THE BOUND.  tau = 32 K n 2^-53 kappa_2(M): the forward error c n u kappa of a product with an explicitly inverted symmetric
positive definite matrix (the kernel's dense step), c = 32, once per iteration.  Derived, not fitted.  x and y are compared
relative to max(1, |ref|_inf), the three figures absolutely against tau times their scale:
  pri_res   max(1, |A x / E|_inf, |z / E|_inf)
  dua_res   max(1, max(|P x / D|_inf, |q / D|_inf, |A' y / D|_inf) / c)
  obj_val   max(1, (1/2 |x|' |P| |x| + |q|' |x|) / c)
(under scaled_termination the residuals and the scales of the first two lose their 1 / E, 1 / D and 1 / c).
NO MARGIN CONDITION: the clip is 1-Lipschitz, so the whole map is Lipschitz-continuous and a bound at rounding distance
from a clip needs no exclusion.  Every instance is compared.

`wrong=` builds the two deliberately wrong models of tests/test_batch_shared_steps_host.py: "plain_rho" gives equality rows
the rho of inequality rows, "z_without_alpha" relaxes x but not z.  No GPU needed."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

import batch_polish_ref as pol
import kkt_reference as kkt

LD = np.longdouble
C_BOUND = 32
UNIT = 2.0 ** -53
REFINE = 5


def _inf(v):
    return LD(np.max(np.abs(v))) if len(v) else LD(0)


class StepModel:
    """The shared part of the model -- scaled matrices, rho, M, its LU factor and kappa_2(M) -- of one base and one scaling."""

    def __init__(self, base, D, E, c, sigma=kkt.SIGMA, rho=1.0, wrong=None):
        assert wrong in (None, "plain_rho", "z_without_alpha")
        P, q0, A, l0, u0 = base
        self.n, self.m = A.shape[1], A.shape[0]
        self.D, self.E, self.c = np.asarray(D, dtype=LD), np.asarray(E, dtype=LD), LD(c)
        self.sigma, self.wrong = LD(sigma), wrong
        Ps, _, As, ls0, us0 = pol.scale_data(P, q0, A, l0, u0, D, E, c)
        self.Ps = Ps.toarray().astype(LD)
        self.As = As.toarray().astype(LD).reshape(self.m, self.n)
        self.A_raw = sp.csr_matrix(A).toarray().astype(LD).reshape(self.m, self.n)
        rv = kkt.rho_vector(ls0, us0, rho)
        if wrong == "plain_rho":
            rv = np.where(kkt.row_classes(ls0, us0) == 1, min(max(float(rho), kkt.RHO_MIN), kkt.RHO_MAX), rv)
        self.rho = np.asarray(rv, dtype=LD).reshape(self.m)
        self.equalities = int(np.sum(kkt.row_classes(ls0, us0) == 1))
        self.M = self.Ps + self.sigma * np.eye(self.n, dtype=LD) + self.As.T @ (self.rho[:, None] * self.As)
        M64 = self.M.astype(np.float64)
        self.lu = sla.lu_factor(M64)
        self.kappa = float(np.linalg.cond(M64, 2))

    def tau(self, K):
        return C_BOUND * K * self.n * UNIT * self.kappa

    def solve(self, b):
        w = sla.lu_solve(self.lu, b.astype(np.float64)).astype(LD)
        for _ in range(REFINE):
            w = w + sla.lu_solve(self.lu, (b - self.M @ w).astype(np.float64)).astype(LD)
        return w

    def run(self, q, l, u, x0, y0, K, alpha, scaled_termination=False):
        """K iterations of instance (q, l, u) from (x0, y0) in caller's units (either may be None) -> dict(x, y, pri_res,
        dua_res, obj_val, scale = (pri, dua, obj), kappa, tau); everything longdouble."""
        D, E, c, As, Ps, rho, m = self.D, self.E, self.c, self.As, self.Ps, self.rho, self.m
        alpha = LD(alpha)
        qs = c * (D * np.asarray(q, dtype=LD))
        ls = np.maximum(np.asarray(l, dtype=LD), -pol.OSQP_INFTY).reshape(m) * E
        us = np.minimum(np.asarray(u, dtype=LD), pol.OSQP_INFTY).reshape(m) * E
        if x0 is None:
            x, z = np.zeros(self.n, dtype=LD), np.zeros(m, dtype=LD)
        else:
            x0 = np.asarray(x0, dtype=LD)
            x, z = x0 / D, E * (self.A_raw @ x0)
        y = np.zeros(m, dtype=LD) if y0 is None or not m else c * np.asarray(y0, dtype=LD) / E
        for _ in range(K):
            xt = self.solve(self.sigma * x - qs + As.T @ (rho * z - y))
            x = alpha * xt + (1 - alpha) * x
            zh = As @ xt if self.wrong == "z_without_alpha" else alpha * (As @ xt) + (1 - alpha) * z
            z = np.minimum(np.maximum(zh + y / rho, ls), us)
            y = y + rho * (zh - z)
        ax, px, aty = As @ x, Ps @ x, As.T @ y
        rp, rd = ax - z, px + qs + aty
        obj = (LD(0.5) * (x @ px) + qs @ x) / c
        obj_scale = (LD(0.5) * (np.abs(x) @ (np.abs(Ps) @ np.abs(x))) + np.abs(qs) @ np.abs(x)) / c
        if scaled_termination:
            pri, dua = _inf(rp), _inf(rd)
            pri_scale, dua_scale = max(_inf(ax), _inf(z)), max(_inf(px), _inf(qs), _inf(aty))
        else:
            pri, dua = _inf(rp / E), _inf(rd / D) / c
            pri_scale, dua_scale = max(_inf(ax / E), _inf(z / E)), max(_inf(px / D), _inf(qs / D), _inf(aty / D)) / c
        one = LD(1)
        return dict(x=D * x, y=E * y / c, pri_res=pri, dua_res=dua, obj_val=obj,
                    scale=(max(one, pri_scale), max(one, dua_scale), max(one, obj_scale)), kappa=self.kappa, tau=self.tau(K))


def k_step(base, inst, scaling, x0, y0, K, alpha, sigma=kkt.SIGMA, rho=1.0, scaled_termination=False):
    """The model as one call: base (P, q0, A, l0, u0), inst (q, l, u), scaling (D, E, c) of the base data."""
    return StepModel(base, *scaling, sigma=sigma, rho=rho).run(*inst, x0, y0, K, alpha, scaled_termination)


def ratios(x, y, info3, want):
    """The errors of a result (x, y, (pri_res, dua_res, obj_val)) against the model's `want`, each as a multiple of the bound
    it is held to: (x, y, pri_res, dua_res, obj_val).  A result passes when every entry is at most 1."""
    tau = LD(want["tau"])
    out = [_inf(np.asarray(x, dtype=LD) - want["x"]) / (tau * max(LD(1), _inf(want["x"])))]
    out.append(_inf(np.asarray(y, dtype=LD) - want["y"]) / (tau * max(LD(1), _inf(want["y"]))))
    for got, key, scale in zip(info3, ("pri_res", "dua_res", "obj_val"), want["scale"]):
        out.append(abs(LD(got) - want[key]) / (tau * scale))
    out = [float(r) for r in out]
    return [r if r == r else float("inf") for r in out]  # a NaN in the result is outside every bound


# ---- the starts and the variants the host test and the GPU test share --------------------------------------------------------
# id -> (solves as a list of max_iter, alpha, start): K = sum of the list
VARIANTS = {
    "K1-alpha1.0": ([1], 1.0, "xy"),
    "K1-alpha1.6": ([1], 1.6, "xy"),
    "K3-alpha1.6": ([3], 1.6, "xy"),
    "K3-chained": ([1, 1, 1], 1.6, "xy"),
    "K1-x-only": ([1], 1.6, "x"),
    "K1-y-only": ([1], 1.6, "y"),
}


M0_COUNT = 35  # 2 T + 3 at the T = 16 of the shape without rows


def family(name):
    """(base, q, l, u) of a family of `batch_shared_cases.EDGES` (2 T + 3 instances) or of "m0", the shape without rows."""
    import batch_shared_cases as S

    return S.unconstrained(count=M0_COUNT) if name == "m0" else S.boxed(name)


def expected_status(name, variant):
    """Max_iter_reached (-2) after K iterations from a random start -- except for ONE iteration with alpha = 1 on the shape
    without rows: there x_1 = (P + sigma I)^-1 (sigma x0 - q) is the optimum up to sigma |x0 - x_1| ~ 1e-6, inside eps = 1e-5,
    and the check made at the iteration limit reports Solved (1), on the oracle too (the host test holds it to this)."""
    return 1 if (name, variant) == ("m0", "K1-alpha1.0") else -2


def starts(name, count, n, m):
    """(x0 [count x n], y0 [count x m]), standard normal, drawn instance by instance: instance i is the same in any batch."""
    x0, y0 = np.empty((count, n)), np.empty((count, m))
    for i in range(count):
        rng = np.random.default_rng([sum(map(ord, name)), i])
        x0[i], y0[i] = rng.standard_normal(n), rng.standard_normal(m)
    return x0, y0


_models, _wants, _scalings = {}, {}, {}


def base_scaling(oracle_lib, key, base, **opts):
    """(D, E, c) of the oracle for the base data: what every instance of a shared batch carries.  Once per key."""
    import osqp_jl_amd as oq

    if key not in _scalings:
        P, q0, A, l0, u0 = base
        mdl = oq.Model(oracle_lib)
        oq.setup(mdl, P=P, q=q0, A=A, l=l0, u=u0, **opts)
        _scalings[key] = pol.oracle_state(mdl, A.shape[1], A.shape[0], opts.get("scaling", 10))[:3]
        oq.clean(mdl)
    return _scalings[key]


def model_of(key, base, scaling, **kw):
    """One StepModel per key, built once per process."""
    if key not in _models:
        _models[key] = StepModel(base, *scaling, **kw)
    return _models[key]


def wants(key, mdl, q, l, u, x0, y0, K, alpha, start, scaled_termination=False):
    """[model result per instance] of one family and variant, computed once per process and left unchanged."""
    if key not in _wants:
        _wants[key] = [mdl.run(q[i], l[i], u[i], x0[i] if "x" in start else None, y0[i] if "y" in start else None, K, alpha,
                               scaled_termination) for i in range(q.shape[0])]
    return _wants[key]
