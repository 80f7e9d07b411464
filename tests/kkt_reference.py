"""An exact reference for the KKT solve of the direct back-end (op 3 of osqp_amd_apply), on the host.

Op 3 takes b = [b_x; b_z] (length n + m) and returns [x~; z~], where (csrc/direct.hip LdlFactor::solve, k_perm_out)

    [P + sigma I    A'            ] [x~]
    [A              -diag(rho)^-1 ] [nu]  =  b,        z~ = b_z + rho^-1 o nu.

`Reference` rebuilds that matrix from the problem data as it stands after an update -- the full symmetric P from its upper
triangle, sigma, and the rho vector by the engine's rule (csrc/kernels.hip k_rho_vec), re-derived here -- for a workspace set
up with scaling=0 and adaptive_rho=False (the matrix the engine factorises is then the caller's), and measures a solve three
ways, none of which goes through the engine:
  (a) the componentwise backward error of w = [x~; nu], nu = rho o (z~ - b_z):  max_i |b - K w|_i / (|K| |w| + |b|)_i;
  (b) the rho-free identity z~ = A x~ (the second block row with nu eliminated), relative to |A| |x~| + |b_z| (z~ is formed
      as b_z + rho^-1 nu: an empty row of A leaves a rounding of b_z behind);
  (c) the distance to an independent solution -- scipy's SuperLU on K and one step of refinement -- in the output's terms
      ([x~; z~]), relative to its largest entry.
A value the engine kept stale or put in the wrong place shows in (a) at about the relative size of the change it missed.

A solve through an explicitly inverted block can measure (a) above BACKWARD without being wrong: an explicit inverse's error
grows with the block's condition number.  Such a solve is held instead to the forward error that a backward error of BACKWARD
allows at the condition of the solve (`check(..., by_condition=True)`):
  (a') ||w - w_ref||_inf / ||w_ref||_inf <= cond(K, w) * BACKWARD,  cond(K, w) = || |K^-1| (|K| |w| + |b|) ||_inf / ||w||_inf
(the componentwise condition number that turns the backward error of (a) into a forward error), cond estimated by Higham's
1-norm estimator on the SuperLU factor (`condition`)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

SIGMA = 1e-6  # the default sigma
RHO_MIN, RHO_MAX = 1e-6, 1e6
RHO_EQ_OVER_RHO_INEQ = 1e3
RHO_TOL = 1e-4     # u - l below it: an equality row
OSQP_INFTY = 1e30
INF_BOUND = 1e26   # OSQP_INFTY * MIN_SCALING: a row beyond it on both sides is free

# The bounds every form of the factorisation is held to (test_kkt_reference_gpu.py gives what the GPU measured against them).
BACKWARD = 1e-10   # (a); (a') scales it by the condition
IDENTITY = 1e-9    # (b)
FORWARD = 1e-9     # (c)


def full_P(P):
    """The symmetric matrix that the upper triangle of P stands for (what the engine reads: setup keeps triu(P))."""
    U = sp.triu(sp.csc_matrix(P, dtype=np.float64), format="csc")
    return (U + sp.triu(U, 1).T).tocsc()


def row_classes(l, u):
    """-1 free, 1 equality, 0 inequality (k_rho_vec's constraint types), for bounds clipped to +-OSQP_INFTY."""
    l = np.maximum(np.asarray(l, dtype=np.float64), -OSQP_INFTY)
    u = np.minimum(np.asarray(u, dtype=np.float64), OSQP_INFTY)
    t = np.where(u - l < RHO_TOL, 1, 0)
    t[(l < -INF_BOUND) & (u > INF_BOUND)] = -1
    return t


def rho_vector(l, u, rho):
    """The engine's rho vector for bounds l, u and the scalar rho."""
    rho = min(max(float(rho), RHO_MIN), RHO_MAX)
    t = row_classes(l, u)
    return np.where(t == -1, RHO_MIN, np.where(t == 1, RHO_EQ_OVER_RHO_INEQ * rho, rho))


def ratio(num, den):
    """max_i num_i / den_i; a row whose scale is zero must have a zero numerator (else the ratio is infinite)."""
    if num.size == 0:
        return 0.0
    safe = np.where(den > 0, den, 1.0)
    q = np.where(den > 0, num / safe, np.where(num > 0, np.inf, 0.0))
    return float(np.max(q))


class Reference:
    """The KKT matrix of one state of the problem; `rho_vec` is the per-row rho (`rho_vector`)."""

    def __init__(self, P, A, rho_vec, sigma=SIGMA):
        self.Pf = full_P(P)
        self.n = self.Pf.shape[0]
        self.A = sp.csc_matrix(A, dtype=np.float64)
        self.m = self.A.shape[0]
        self.rho = np.asarray(rho_vec, dtype=np.float64)
        assert self.A.shape[1] == self.n and self.rho.shape == (self.m,)
        H = (self.Pf + sigma * sp.eye(self.n, format="csc")).tocsc()
        if self.m:
            self.K = sp.bmat([[H, self.A.T], [self.A, -sp.diags(1.0 / self.rho)]], format="csc")
        else:
            self.K = H
        self.absK = abs(self.K)
        self.absA = abs(self.A)
        self._lu = None

    def w(self, b, out):
        """[x~; nu] of an output [x~; z~]."""
        return np.concatenate([out[:self.n], self.rho * (out[self.n:] - b[self.n:])])

    def backward_error(self, b, out):
        """(a)"""
        w = self.w(b, out)
        return ratio(np.abs(b - self.K @ w), self.absK @ np.abs(w) + np.abs(b))

    def identity_error(self, b, out):
        """(b)"""
        x, z = out[:self.n], out[self.n:]
        return ratio(np.abs(z - self.A @ x), self.absA @ np.abs(x) + np.abs(b[self.n:]))

    def factor(self):
        if self._lu is None:
            self._lu = spla.splu(self.K)
        return self._lu

    def reference_w(self, b):
        """w of the independent solve (SuperLU with partial pivoting on K, one step of refinement)."""
        lu = self.factor()
        w = lu.solve(b)
        return w + lu.solve(b - self.K @ w)

    def solution(self, b):
        """[x; z] of the independent solve."""
        w = self.reference_w(b)
        return np.concatenate([w[:self.n], b[self.n:] + w[self.n:] / self.rho])

    def forward_error(self, b, out):
        """(c)"""
        ref = self.solution(b)
        return float(np.max(np.abs(out - ref)) / max(float(np.max(np.abs(ref))), np.finfo(float).tiny))

    def condition(self, b, out):
        """cond(K, w) of (a'): || K^-1 G ||_inf / ||w||_inf with G = diag(|K| |w| + |b|) -- the 1-norm of G K^-1, K being
        symmetric -- by scipy's onenormest (Higham's block estimator; a lower bound, exact or close in practice)."""
        w = self.w(b, out)
        g = self.absK @ np.abs(w) + np.abs(b)
        lu = self.factor()
        N = self.n + self.m
        op = spla.LinearOperator((N, N), matvec=lambda v: g * lu.solve(np.ravel(v)), rmatvec=lambda v: lu.solve(g * np.ravel(v)),
                                 dtype=np.float64)
        return float(spla.onenormest(op)) / max(float(np.max(np.abs(w))), np.finfo(float).tiny)

    def forward_error_w(self, b, out):
        """||w - w_ref||_inf / ||w_ref||_inf of (a')."""
        ref = self.reference_w(b)
        return float(np.max(np.abs(self.w(b, out) - ref)) / max(float(np.max(np.abs(ref))), np.finfo(float).tiny))

    def errors(self, b, out, conditioned=False):
        """(a), (b), (c); `conditioned`: also cond(K, w) and the forward error in w of (a')."""
        b, out = np.asarray(b, dtype=np.float64), np.asarray(out, dtype=np.float64)
        assert b.shape == out.shape == (self.n + self.m,)
        if not np.all(np.isfinite(out)):
            return dict(backward=np.inf, identity=np.inf, forward=np.inf, condition=np.inf, forward_w=np.inf)
        e = dict(backward=self.backward_error(b, out), identity=self.identity_error(b, out), forward=self.forward_error(b, out))
        if conditioned:
            e.update(condition=self.condition(b, out), forward_w=self.forward_error_w(b, out))
        return e

    def check(self, b, out, backward, identity, forward, what="", by_condition=False):
        """Asserts (a) -- or, `by_condition`, (a') -- (b) and (c); returns the measured errors."""
        e = self.errors(b, out, conditioned=by_condition)
        first = e["forward_w"] <= e["condition"] * backward if by_condition else e["backward"] <= backward
        assert first and e["identity"] <= identity and e["forward"] <= forward, (what, e)
        return e
