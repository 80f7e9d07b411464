"""An exact reference for the ADMM iterates of the indirect back-end (csrc/pcg.hip), on the host: numpy / scipy only, no engine
and no oracle in any number it gives (the values of R4's matrix and bounds events are drawn by the plain functions of kkt_events.py).

With OSQP_AMD_PCG_LAMBDA=0 every CG solve of the engine stops at the floor of its tolerance rule, ||r||inf <= 1e-13 ||b1||inf,
so with scaling=0 its iterates are those of an ADMM whose KKT systems are solved exactly, up to cond(M) * 1e-13 per step
(M = P + sigma I + A' diag(rho) A).  `ExactAdmm` is that ADMM:

    b = [sigma x - q ; z - y / rho],   (x~, z~) = kkt_reference.Reference(P, A, rho).solution(b)   (SuperLU + one refinement step),
    x+ = alpha x~ + (1 - alpha) x,   zr = alpha z~ + (1 - alpha) z,   z+ = clip(zr + y / rho, l, u),   y+ = y + rho (zr - z+),

with the engine's rules around it, re-derived here from their definitions and not called: the rho vector by row class
(kkt_reference.rho_vector), a warm start from the kept iterate, `warm_start(x, y)` (z = A x, not clipped: Engine::warm_start), the
events between solves (q, rho, values of P and A in full or by index, bounds, alpha), adaptive rho inside a solve
(Engine::compute_rho_estimate / adapt_rho: rho sqrt(pri / dua) on residuals relative to their norms, an update when it leaves
[rho / 5, 5 rho]; every decision is recorded with its two thresholds) and the progress monitor of the tolerance rule
(Engine::update_info): 25 iterations after its reference point without halving sqrt(pri dua) it would raise lambda from 0 to 1e-6
and the engine's solves would stop being exact -- `ExactAdmm` raises instead, so a run that passes never met it.

`CgAdmm` is the same iteration with the linear solve stated as pcg.hip states it, for iteration counts (and to show that such a
statement stays ten times closer to the exact one than the GPU is asked to): Jacobi preconditioner 1 / (sigma + diag P +
sum_i rho_i A_ij^2); start vector = the energy-optimal point on the line through the last two solutions, theta clamped to
[-1, 4], off for the first solve after M changed or the guess was set (every solve call sets it to x); the products A x~ and M x~
carried along the recurrences and recomputed every 25 solves and whenever rho or the matrices change; z~ = the carried A x~; stop
at ||r||inf <= 1e-13 ||b1||inf + 1e-300.  Two switches make it wrong on purpose (test_pcg_reference_host.py: the checks see both):
`keep_dinv` keeps the preconditioner across a rho change (more iterations, same iterates); `keep_Ax` keeps the carried pair -- one
refresh computes A x~ and M x~ together -- across a rho change (a converged recurrence around a wrong point).

CASES: the smallest problems at which the kernels of pcg.hip can go wrong (see `case`)."""
import numpy as np
import scipy.sparse as sp

import kkt_reference as kr

REFRESH = 25          # kRefresh of pcg.hip
MONITOR = 25          # distance of the progress monitor's reference points
RHO_TOLERANCE = 5.0   # adaptive_rho_tolerance (default)
FLOOR = 1e-13         # the floor of the tolerance rule, relative to ||b1||inf
EPS = 1e-12           # eps_abs = eps_rel of every run: no early stop


class MonitorFired(AssertionError):
    pass


def residuals(P_full, q, A, x, z, y):
    """pri, dua and the norms the rho estimate divides them by (unscaled: scaling=0)."""
    Ax, Px, Aty = A @ x, P_full @ x, A.T @ y
    m = A.shape[0]
    ninf = lambda v: float(np.max(np.abs(v))) if v.size else 0.0
    pri = ninf(Ax - z) if m else 0.0
    dua = ninf(Px + q + Aty)
    return pri, dua, (max(ninf(z), ninf(Ax)) if m else 0.0), max(ninf(q), ninf(Aty) if m else 0.0, ninf(Px))


class ExactAdmm:
    def __init__(self, P, q, A, l, u, rho=0.1, sigma=kr.SIGMA, alpha=1.6):
        self.P = sp.csc_matrix(sp.triu(sp.csc_matrix(P, dtype=np.float64), format="csc"))
        self.P.sum_duplicates(); self.P.sort_indices()
        self.n = self.P.shape[0]
        self.A = sp.csc_matrix(A, dtype=np.float64, copy=True) if A is not None else sp.csc_matrix((0, self.n))
        self.A.sum_duplicates(); self.A.sort_indices()
        self.m = self.A.shape[0]
        self.q = np.asarray(q, dtype=np.float64).copy()
        self.l = np.maximum(np.asarray(l, dtype=np.float64), -kr.OSQP_INFTY) if self.m else np.zeros(0)
        self.u = np.minimum(np.asarray(u, dtype=np.float64), kr.OSQP_INFTY) if self.m else np.zeros(0)
        self.rho, self.sigma, self.alpha = float(rho), float(sigma), float(alpha)
        self.x, self.z, self.y = np.zeros(self.n), np.zeros(self.m), np.zeros(self.m)
        self.decisions = []   # (iteration, estimate, rho * tol, rho / tol, updated) of every adaptive-rho decision
        self.rho_updates = 0
        self._matrix_changed()

    # ---- the state the linear solve depends on
    def _matrix_changed(self, rho_only=False):
        self.Pf = kr.full_P(self.P)
        self.rho_vec = kr.rho_vector(self.l, self.u, self.rho)
        self._ref = None
        self.matrix_changed_hook(rho_only)

    def matrix_changed_hook(self, rho_only):
        pass

    def guess_set_hook(self):
        pass

    def kkt(self, b):
        if self._ref is None:
            self._ref = kr.Reference(self.P, self.A, self.rho_vec, self.sigma)
        out = self._ref.solution(b)
        return out[:self.n], out[self.n:]

    def M(self):
        """The reduced matrix P + sigma I + A' diag(rho) A of the current state."""
        return (self.Pf + self.sigma * sp.eye(self.n, format="csc") + self.A.T @ sp.diags(self.rho_vec) @ self.A).tocsc()

    # ---- events between solves
    def update_q(self, q):
        self.q = np.asarray(q, dtype=np.float64).copy()

    def update_rho(self, rho):
        self.rho = min(max(float(rho), kr.RHO_MIN), kr.RHO_MAX)
        self._matrix_changed(rho_only=True)

    def update_alpha(self, alpha):
        self.alpha = float(alpha)

    def update_values(self, Px=None, Px_idx=None, Ax=None, Ax_idx=None):
        for M, vals, idx in ((self.P, Px, Px_idx), (self.A, Ax, Ax_idx)):
            if vals is not None and len(vals):
                M.data[slice(None) if idx is None else idx] = vals
        self._matrix_changed()

    def update_bounds(self, l, u):
        before = self.rho_vec
        self.l = np.maximum(np.asarray(l, dtype=np.float64), -kr.OSQP_INFTY)
        self.u = np.minimum(np.asarray(u, dtype=np.float64), kr.OSQP_INFTY)
        if not np.array_equal(kr.rho_vector(self.l, self.u, self.rho), before):
            self._matrix_changed(rho_only=True)  # (Engine::update_rho_vec_from_bounds: the back-end's update_rho)

    def warm_start(self, x, y):
        self.x = np.asarray(x, dtype=np.float64).copy()
        self.y = np.asarray(y, dtype=np.float64).copy()
        self.z = self.A @ self.x

    def cold_start(self):
        self.x, self.z, self.y = np.zeros(self.n), np.zeros(self.m), np.zeros(self.m)

    # ---- the stopping test at the end of a call (Engine::check_termination on unscaled data; the problems are feasible)
    def status_margin(self, r, eps):
        """(pri / eps_pri, dua / eps_dua): below 1 the residual passes."""
        pri, dua, pri_norm, dua_norm = r
        return (pri / (eps + eps * pri_norm) if self.m else 0.0), dua / (eps + eps * dua_norm)

    def status(self, r, eps):
        a, b = self.status_margin(r, eps)
        if a < 1.0 and b < 1.0:
            return "Solved"
        return "Solved_inaccurate" if a < 10.0 and b < 10.0 else "Max_iter_reached"

    # ---- one solve call
    def step(self):
        rho = self.rho_vec
        b = np.concatenate([self.sigma * self.x - self.q, self.z - self.y / rho])
        xt, zt = self.kkt(b)
        a = self.alpha
        self.x = a * xt + (1.0 - a) * self.x
        zr = a * zt + (1.0 - a) * self.z
        z_new = np.clip(zr + self.y / rho, self.l, self.u)
        self.y = self.y + rho * (zr - z_new)
        self.z = z_new

    def solve(self, max_iter, check_termination=0, adaptive_rho=False, adaptive_rho_interval=0, warm=True, trajectory=False):
        """`max_iter` iterations (no early stop: the tests run with eps = 1e-12 and assert Max_iter_reached).  Returns the
        final x, y, pri_res, dua_res, the number of rho updates of this call and -- `trajectory` -- every iterate (x, y)."""
        if not warm:
            self.cold_start()
        self.guess_set_hook()
        have_ref, g_ref, it_ref = False, 0.0, 0
        updates, path = 0, []
        last = None

        def evaluate(it):
            nonlocal have_ref, g_ref, it_ref
            r = residuals(self.Pf, self.q, self.A, self.x, self.z, self.y)
            g = np.sqrt(r[0] * r[1])
            if not have_ref:
                g_ref, it_ref, have_ref = g, it, True
            elif it - it_ref >= MONITOR:
                if g > 0.5 * g_ref:
                    raise MonitorFired(f"the progress monitor fires at iteration {it} (reference point {it_ref}): {g} > 0.5 * {g_ref}")
                g_ref, it_ref = g, it
            return r

        can_check = False
        for it in range(1, max_iter + 1):
            self.step()
            if trajectory:
                path.append((self.x.copy(), self.y.copy()))
            can_check = bool(check_termination) and it % check_termination == 0
            if can_check:
                last = evaluate(it)
                assert it == max_iter or self.status(last, EPS) == "Max_iter_reached", (it, last)  # (no early stop)
            if adaptive_rho and adaptive_rho_interval and it % adaptive_rho_interval == 0:
                if not can_check:
                    last = evaluate(it)
                pri, dua, pri_norm, dua_norm = last
                est = self.rho * np.sqrt((pri / (pri_norm + 1e-10)) / (dua / (dua_norm + 1e-10) + 1e-10))
                est = min(max(est, kr.RHO_MIN), kr.RHO_MAX)
                hi, lo = self.rho * RHO_TOLERANCE, self.rho / RHO_TOLERANCE
                update = est > hi or est < lo
                self.decisions.append((it, est, hi, lo, update))
                if update:
                    self.update_rho(est)
                    updates += 1
        if not can_check:
            last = evaluate(max_iter)
        self.rho_updates += updates
        out = dict(x=self.x.copy(), y=self.y.copy(), pri_res=last[0], dua_res=last[1], rho_updates=updates, iter=max_iter,
                   status=self.status(last, EPS), margin=self.status_margin(last, EPS))
        if trajectory:
            out["trajectory"] = path
        return out


class CgAdmm(ExactAdmm):
    """The same iteration with the linear solve as pcg.hip states it (module docstring); `cg_total` counts CG iterations,
    `cg_per_step` lists them per ADMM step."""

    def __init__(self, *a, keep_dinv=False, keep_Ax=False, extrapolate=True, **k):
        self.keep_dinv, self.keep_Ax, self.extrapolate = keep_dinv, keep_Ax, extrapolate
        self.cg_total, self.cg_per_step = 0, []
        self.xs = None
        self._M = self._dinv = None
        self.carried_valid = self.have_prev = False
        self.since_refresh = 0
        super().__init__(*a, **k)
        self.xs = np.zeros(self.n)

    def matrix_changed_hook(self, rho_only):
        """Pcg::update_rho / update_matrices: preconditioner rebuilt, carried products and extrapolation pair dropped (the two
        switches: not after a change of rho alone)."""
        first = self._M is None or not rho_only
        self._M = self.M()
        self._AtR = (self.A.T @ sp.diags(self.rho_vec)).tocsr()
        self._Acsr = self.A.tocsr()
        if first or not self.keep_dinv:
            A2 = self.A.copy(); A2.data = A2.data ** 2
            self._dinv = 1.0 / (self.sigma + self.Pf.diagonal() + (A2.T @ self.rho_vec if self.m else 0.0))
        if first or not self.keep_Ax:
            self.carried_valid = False
        self.have_prev = False

    def guess_set_hook(self):
        """Pcg::set_guess at the start of every solve call."""
        self.xs = self.x.copy()
        self.carried_valid = self.have_prev = False

    def kkt(self, b):
        n, M, dinv = self.n, self._M, self._dinv
        b1 = b[:n] + (self._AtR @ b[n:] if self.m else 0.0)
        bnorm = float(np.max(np.abs(b1)))
        self.since_refresh += 1
        if not self.carried_valid or self.since_refresh >= REFRESH:
            self.Axs, self.Mxs = self._Acsr @ self.xs, M @ self.xs
            self.carried_valid, self.since_refresh = True, 0
        xs, Axs, Mxs = self.xs, self.Axs, self.Mxs
        if self.extrapolate:
            if self.have_prev:
                e = xs - self.xs0
                num, den = float(e @ (b1 - Mxs)), float(e @ (Mxs - self.Mxs0))
                theta = num / den if den > 0.0 else 0.0
                theta = 0.0 if theta != theta else min(max(theta, -1.0), 4.0)
                new = (xs + theta * e, Axs + theta * (Axs - self.Axs0), Mxs + theta * (Mxs - self.Mxs0))
                self.xs0, self.Axs0, self.Mxs0 = xs, Axs, Mxs
                xs, Axs, Mxs = new
            else:
                self.xs0, self.Axs0, self.Mxs0 = xs.copy(), Axs.copy(), Mxs.copy()
                self.have_prev = True
        tol = FLOOR * bnorm + 1e-300
        r = b1 - Mxs
        zz = dinv * r
        p = zz.copy()
        rz = float(r @ zz)
        it = 0
        xs, Axs, Mxs = xs.copy(), Axs.copy(), Mxs.copy()
        while float(np.max(np.abs(r))) > tol and it < 20000:
            u = self._Acsr @ p
            w = M @ p
            alpha = rz / float(p @ w)
            xs += alpha * p; Axs += alpha * u; Mxs += alpha * w
            r -= alpha * w
            zz = dinv * r
            rz_new = float(r @ zz)
            p = zz + (rz_new / rz) * p
            rz = rz_new
            it += 1
        self.cg_total += it
        self.cg_per_step.append(it)
        self.xs, self.Axs, self.Mxs = xs, Axs, Mxs
        return xs.copy(), Axs.copy()


# ----------------------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------------------
def _bounds(rng, A, eq_share, free_share):
    """Two-sided rows around A x0 for a random x0 (the problem is feasible), a share of equalities and of free rows."""
    m = A.shape[0]
    c = A @ rng.standard_normal(A.shape[1])
    l, u = c - 0.2 - rng.random(m), c + 0.2 + rng.random(m)
    k = rng.permutation(m)
    ne, nf = int(round(eq_share * m)), int(round(free_share * m))
    l[k[:ne]] = u[k[:ne]] = c[k[:ne]]
    l[k[ne:ne + nf]], u[k[ne:ne + nf]] = -np.inf, np.inf
    return l, u


def _mixed(rng, n, m, density, eq_share, free_share, a_scale):
    B = sp.random(n, n, density=density, random_state=rng, data_rvs=rng.standard_normal, format="csc")
    P = sp.triu((B.T @ B + sp.eye(n)).tocsc(), format="csc")
    stripe = sp.csc_matrix((np.ones(m), (np.arange(m), np.arange(m) % n)), shape=(m, n))
    A = (a_scale * sp.random(m, n, density=density, random_state=rng, data_rvs=rng.standard_normal, format="csc") + stripe).tocsc()
    l, u = _bounds(rng, A, eq_share, free_share)
    return dict(P=P, q=rng.standard_normal(n), A=A, l=l, u=u, rho=0.1)


def case(name):
    """name -> dict(P (upper triangle), q, A, l, u, rho).  Fixed seeds.
      mixed    n = 300, m = 350, density 0.03; P = B'B + I, A = random + an identity stripe; 5 % equality rows, 10 % free rows, the
               rest two-sided: neither n nor m a multiple of 64 or 256, all three rho classes
      easy     n = 321, m = 290; P = I + 0.02 * sparse symmetric, rho = 0.01, no equalities: at most 6 CG iterations on every step
               after the third (the asynchronous form completes steps on the device without stalling)
      tiny     n = 70, m = 66: just above a 64-column panel (one full panel and a ragged one), one partial workgroup
      no-rows  n = 200, m = 0: the fused forms must fall back; the m > 0 branches
      wrap     n = 262144 + 257, m = 262144 + 300; P tridiagonal, strictly diagonally dominant, A with two entries per row: the
               first sizes at which the grid-stride loops of k_pcg_start / k_pcg_step / k_pcg_sr take a second pass"""
    if name == "mixed":
        return _mixed(np.random.default_rng(101), 300, 350, 0.03, 0.05, 0.10, 0.25)
    if name == "tiny":
        return _mixed(np.random.default_rng(193), 70, 66, 0.08, 0.05, 0.10, 0.2)
    if name == "easy":
        rng = np.random.default_rng(102)
        n, m = 321, 290
        S = sp.random(n, n, density=0.003, random_state=rng, data_rvs=lambda k: rng.uniform(-0.3, 0.3, k), format="csc")
        P = sp.triu((sp.eye(n) + 0.02 * (S + S.T)).tocsc(), format="csc")
        A = 0.2 * sp.random(m, n, density=0.02, random_state=rng, data_rvs=rng.standard_normal, format="csc")
        l, u = _bounds(rng, A, 0.0, 0.05)
        return dict(P=P, q=rng.standard_normal(n), A=A, l=l, u=u, rho=0.01)
    if name == "no-rows":
        rng = np.random.default_rng(104)
        n = 200
        B = sp.random(n, n, density=0.03, random_state=rng, data_rvs=rng.standard_normal, format="csc")
        P = sp.triu((B.T @ B + sp.eye(n)).tocsc(), format="csc")
        return dict(P=P, q=rng.standard_normal(n), A=sp.csc_matrix((0, n)), l=np.zeros(0), u=np.zeros(0), rho=0.1)
    if name == "wrap":
        rng = np.random.default_rng(105)
        n, m = 262144 + 257, 262144 + 300
        d = 2.0 + rng.random(n)
        o = 0.5 * rng.uniform(-1.0, 1.0, n - 1)
        P = sp.diags([d, o], [0, 1], format="csc")
        r = np.arange(m)
        A = sp.csc_matrix((np.concatenate([rng.uniform(0.5, 1.0, m), rng.uniform(-0.5, 0.5, m)]),
                           (np.concatenate([r, r]), np.concatenate([r % n, (r + 3) % n]))), shape=(m, n))
        l, u = _bounds(rng, A, 0.0, 0.05)
        return dict(P=P, q=rng.standard_normal(n), A=A, l=l, u=u, rho=0.1)
    raise KeyError(name)


CASES = ("mixed", "easy", "tiny", "no-rows", "wrap")
SMALL = ("mixed", "easy", "tiny", "no-rows")


def gershgorin_cond(M):
    """An upper bound on cond(M) of a symmetric, strictly diagonally dominant M with a positive diagonal."""
    M = sp.csr_matrix(M)
    d = M.diagonal()
    off = np.asarray(abs(M).sum(axis=1)).ravel() - np.abs(d)
    assert np.all(d - off > 0)
    return float(np.max(d + off) / np.min(d - off))


# ----------------------------------------------------------------------------------------------------------------------------
# the runs (test_pcg_reference_gpu.py drives the engine through the same; SETTINGS are the solver settings of each solve call)
# ----------------------------------------------------------------------------------------------------------------------------
RHO_EVENT = 2.0
RHO_DOWN = 1e-3  # the last event of R4: a stale preconditioner costs CG iterations after a decrease of rho (after an increase it saves some)
R4_ITER = 12


def run_settings(run, name):
    if run == "R1":
        return dict(adaptive_rho=False, check_termination=0, max_iter=8 if name == "wrap" else 60)
    if run == "R2":
        return dict(adaptive_rho=False, check_termination=7, max_iter=30)
    if run == "R3":
        return dict(adaptive_rho=True, adaptive_rho_interval=8, check_termination=0, max_iter=30)
    if run == "R4":
        return dict(adaptive_rho=False, check_termination=0, max_iter=R4_ITER)
    raise KeyError(run)


R4_EVENTS = ("setup", "update_q", "rho", "full", "subset", "to-equalities-and-free", "back", "warm_start", "alpha", "rho-down")


def r4_event(model, event, rng):
    """Draws the values of an event of R4 from the host model's data; returns (kind, payload) for whoever applies it (to an
    `ExactAdmm` through `apply_event`, to the engine in the GPU test)."""
    import kkt_events as ev

    if event == "setup":
        return "none", None
    if event == "update_q":
        return "q", rng.standard_normal(model.n)
    if event == "rho":
        return "rho", RHO_EVENT
    if event == "full":
        Px, Ax = ev.full_update_values(rng, model.P, model.A)
        return "values", (Px, None, Ax, None)
    if event == "subset":
        return "values", ev.subset_update_values(rng, model.P, model.A)
    if event == "to-equalities-and-free":
        if model.m == 0:
            return "none", None
        model._bounds_before = (model.l.copy(), model.u.copy())
        return "bounds", ev.bounds_update_values(rng, np.where(model.l <= -kr.OSQP_INFTY, -np.inf, model.l),
                                                 np.where(model.u >= kr.OSQP_INFTY, np.inf, model.u))
    if event == "back":
        if model.m == 0:
            return "none", None
        return "bounds", model._bounds_before
    if event == "warm_start":
        return "warm_start", (rng.standard_normal(model.n), rng.standard_normal(model.m))
    if event == "alpha":
        return "alpha", 1.0
    if event == "rho-down":
        return "rho", RHO_DOWN
    raise KeyError(event)


def apply_event(model, kind, payload):
    if kind == "q":
        model.update_q(payload)
    elif kind == "rho":
        model.update_rho(payload)
    elif kind == "values":
        Px, Px_idx, Ax, Ax_idx = payload
        model.update_values(Px, Px_idx, Ax, Ax_idx)
    elif kind == "bounds":
        model.update_bounds(*payload)
    elif kind == "warm_start":
        model.warm_start(*payload)
    elif kind == "alpha":
        model.update_alpha(payload)
    elif kind != "none":
        raise KeyError(kind)


def make(name, cls=ExactAdmm, **k):
    c = case(name)
    return cls(c["P"], c["q"], c["A"], c["l"], c["u"], rho=c["rho"], **k)


def reference_run(name, run, cls=ExactAdmm, trajectory=False, **k):
    """The host model's results of a run on a case: a list with one entry per solve call (one for R1 - R3; one per event for R4,
    with the event's kind and payload so that the GPU test applies the very same values), and the model."""
    model = make(name, cls, **k)
    s = run_settings(run, name)
    call = dict(max_iter=s["max_iter"], check_termination=s["check_termination"], adaptive_rho=s["adaptive_rho"],
                adaptive_rho_interval=s.get("adaptive_rho_interval", 0), trajectory=trajectory)
    if run != "R4":
        return [dict(model.solve(warm=False, **call), event="setup", kind="none", payload=None)], model
    rng = np.random.default_rng(7)
    out = []
    for event in R4_EVENTS:
        kind, payload = r4_event(model, event, rng)
        apply_event(model, kind, payload)
        out.append(dict(model.solve(warm=event != "setup", **call), event=event, kind=kind, payload=payload))
    return out, model


_RUNS = {}


def cached_run(name, run, cls=ExactAdmm):
    """`reference_run`, computed once per process and shared (nobody writes into a record); with every iterate, but for `wrap`."""
    key = (name, run, cls)
    if key not in _RUNS:
        _RUNS[key] = reference_run(name, run, cls, trajectory=name != "wrap")
    return _RUNS[key]


# ----------------------------------------------------------------------------------------------------------------------------
# the linear solve on its own (op 3 of osqp_amd_apply), through events 1 to 6 of kkt_events.py
# ----------------------------------------------------------------------------------------------------------------------------
COND_MAX = 1e4


def solve_structures():
    """name -> problem: the two cases with all three row classes, and small instances of the structures of qp_zoo.py."""
    import qp_zoo

    return {
        "mixed": lambda: case("mixed"), "tiny": lambda: case("tiny"),
        "grid2d": lambda: qp_zoo.grid2d(20), "grid3d": lambda: qp_zoo.grid3d(7), "control": lambda: qp_zoo.control(nx=8, nu=4, T=40),
        "portfolio": lambda: qp_zoo.portfolio(n=300, k=10), "svm": lambda: qp_zoo.svm(n=20, m=150),
        "equality": lambda: qp_zoo.equality_qp(300), "huber": lambda: qp_zoo.huber(n=20, m=150), "lasso": lambda: qp_zoo.lasso_data(n=20, m=150),
    }


# those whose cond(M) stays at most COND_MAX through the six events (test_pcg_reference_host.py computes the set and compares)
SOLVE_QUALIFIED = ("mixed", "tiny", "grid2d", "grid3d")


def reduced_matrix(ref, sigma=kr.SIGMA):
    """M of a kkt_reference.Reference."""
    return (ref.Pf + sigma * sp.eye(ref.n, format="csc") + ref.A.T @ sp.diags(ref.rho) @ ref.A).tocsc()


def reduced_residual(ref, b, out, sigma=kr.SIGMA):
    """||b1 - M x~||inf / ||b1||inf with b1 = b_x + A'(rho o b_z), formed on the host."""
    b1 = b[:ref.n] + ref.A.T @ (ref.rho * b[ref.n:])
    return float(np.max(np.abs(b1 - reduced_matrix(ref, sigma) @ out[:ref.n])) / np.max(np.abs(b1)))


def dense_cond(M):
    w = np.linalg.eigvalsh(M.toarray())
    return float(w[-1] / w[0])


class CgAdmmPlainStart(CgAdmm):
    """OSQP_AMD_PCG_EXTRAP=0: every solve starts from the last solution."""

    def __init__(self, *a, **k):
        super().__init__(*a, extrapolate=False, **k)
