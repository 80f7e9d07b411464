"""The events that rewrite a workspace's KKT matrix, shared by the tests that hold a back-end's solve to kkt_reference.py
(test_kkt_reference_gpu.py: the direct back-end; test_pcg_reference_gpu.py: the indirect one).

The values of an event are drawn by plain functions of the data and a generator (`full_update_values`, `subset_update_values`,
`bounds_update_values`): whoever applies an event to a workspace and to a host model of it draws them once.  `Workspace` is the
driver: one workspace and the data it must hold; every event updates both, then the solve (op 3 of osqp_amd_apply) is checked
against the data."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import kkt_reference as kr
import osqp_jl_amd as oq

RHO0, RHO1, RHO2 = 0.1, 0.731, 0.2
PRODUCTS = 1e-12  # ops 0 / 1 / 2, componentwise relative to |M| |v|


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def apply(m, op, v, nout):
    v = np.ascontiguousarray(v, dtype=np.float64)
    out = np.empty(nout)
    assert m.lib.osqp_amd_apply(m.workspace, op, fptr(v), fptr(out)) == 0
    return out


def canonical(M):
    M = sp.csc_matrix(M, dtype=np.float64, copy=True)
    M.sum_duplicates()
    M.sort_indices()
    return M


def entries(M):
    """Row and column of every stored entry, in storage order (the order of the nnz indices of an update)."""
    return M.indices, np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))


def full_update_values(rng, P, A):
    """P -> D P D, A -> A o (1 + 0.3 xi); explicitly stored zeros become non-zero (a diagonal one d_i^2, an off-diagonal one a
    quarter of the geometric mean of its two new diagonal entries, A's a value in +-[0.5, 1.5]).  Returns (Px, Ax) in full."""
    n = P.shape[0]
    r, c = entries(P)
    d = rng.uniform(0.5, 2.0, n)
    Px = d[r] * d[c] * P.data
    zero = P.data == 0
    Px[zero & (r == c)] = d[r[zero & (r == c)]] ** 2
    dpos = np.full(n, -1)
    dpos[c[r == c]] = np.flatnonzero(r == c)
    off = np.flatnonzero(zero & (r != c) & (dpos[r] >= 0) & (dpos[c] >= 0))
    Px[off] = 0.25 * np.sqrt(Px[dpos[r[off]]] * Px[dpos[c[off]]])
    Ax = A.data * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, A.nnz))
    za = A.data == 0
    Ax[za] = rng.choice([-1.0, 1.0], int(za.sum())) * rng.uniform(0.5, 1.5, int(za.sum()))
    return Px, Ax


def subset_update_values(rng, P, A):
    """The entries of P that touch a random tenth of the variables (scaled as in D P D), a random third of A's.  Returns
    (Px, Px_idx, Ax, Ax_idx)."""
    n = P.shape[0]
    S = rng.choice(n, max(1, n // 10), replace=False)
    d = np.ones(n)
    d[S] = rng.uniform(0.5, 2.0, len(S))
    r, c = entries(P)
    pidx = rng.permutation(np.flatnonzero(np.isin(r, S) | np.isin(c, S)))
    aidx = rng.choice(A.nnz, max(1, A.nnz // 3), replace=False) if A.nnz else np.zeros(0, dtype=np.int64)
    Px = d[r[pidx]] * d[c[pidx]] * P.data[pidx]
    Ax = A.data[aidx] * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, len(aidx)))
    return Px, pidx, Ax, aidx


def bounds_update_values(rng, l, u):
    """A tenth of the inequality rows become equalities, another tenth free; a third of the equality rows inequalities.
    Returns the new (l, u); the row classes are asserted to have changed as said."""
    t = kr.row_classes(l, u)
    l, u = l.copy(), u.copy()
    ineq, eq = rng.permutation(np.flatnonzero(t == 0)), rng.permutation(np.flatnonzero(t == 1))
    k = max(1, len(ineq) // 10) if len(ineq) >= 2 else 0
    to_eq, to_free, to_ineq = ineq[:k], ineq[k:2 * k], eq[:max(1, len(eq) // 3)] if len(eq) else eq
    v = np.where(np.isfinite(l[to_eq]), l[to_eq], np.where(np.isfinite(u[to_eq]), u[to_eq], 0.0))
    l[to_eq], u[to_eq] = v, v
    l[to_free], u[to_free] = -np.inf, np.inf
    l[to_ineq] -= 1.0
    u[to_ineq] += 1.0
    want = t.copy()
    want[to_eq], want[to_free], want[to_ineq] = 1, -1, 0
    assert np.array_equal(kr.row_classes(l, u), want) and not np.array_equal(want, t)
    return l, u


class Workspace:
    """One workspace and the data it must hold: every event updates both, then the solve is checked against the data.
    `linsys_solver` picks the back-end; `judge(ref, b, out, what)` replaces the default verdict on a solve (kkt_reference's
    three bounds, and the count of factorisations, which only the direct back-end keeps).  `lib=None` walks the data alone
    through the same events with the same draws (no workspace: `judge` gets out=None) -- what a host test looks at."""

    def __init__(self, lib, prob, what, seed, by_condition, linsys_solver="direct", judge=None):
        self.by_condition = by_condition
        self.judge = judge
        P = sp.csc_matrix(prob["P"])
        if sp.tril(P, -1).nnz:
            P = sp.triu(P, format="csc")
        self.P = canonical(P)
        n = self.P.shape[0]
        self.A = canonical(prob["A"]) if prob.get("A") is not None else sp.csc_matrix((0, n))
        self.l = np.asarray(prob.get("l", np.zeros(0)), dtype=np.float64).copy()
        self.u = np.asarray(prob.get("u", np.zeros(0)), dtype=np.float64).copy()
        self.rho = RHO0
        self.rng = np.random.default_rng(seed)
        self.factorizations = 1
        self.m = None
        self.what = what
        if lib is None:
            return
        self.m = oq.Model(lib)
        oq.setup(self.m, P=self.P, q=prob["q"], A=self.A, l=self.l, u=self.u, linsys_solver=linsys_solver, verbose=False, scaling=0,
                 adaptive_rho=False, rho=RHO0)
        st = self.stats()
        self.what = f"{what} (supernode levels {int(st[19])}, dense block {int(st[25])})"

    def stats(self):
        return oq.stats(self.m)

    def check(self, event):
        n, mm = self.A.shape[1], self.A.shape[0]
        ref = kr.Reference(self.P, self.A, kr.rho_vector(self.l, self.u, self.rho))
        b = self.rng.standard_normal(n + mm)
        out = None
        if self.m is not None:
            out = np.empty_like(b)
            assert self.m.lib.osqp_amd_apply(self.m.workspace, 3, fptr(b), fptr(out)) == 0
        if self.judge is not None:
            self.judge(ref, b, out, f"{self.what} / {event}")
            return
        ref.check(b, out, kr.BACKWARD, kr.IDENTITY, kr.FORWARD, what=f"{self.what} / {event}", by_condition=self.by_condition)
        assert self.stats()[8] == self.factorizations, (self.what, event, self.stats()[8], self.factorizations)

    def check_products(self, event):
        n, mm = self.A.shape[1], self.A.shape[0]
        x, y = self.rng.standard_normal(n), self.rng.standard_normal(mm)
        for op, M, v in ((0, self.A, x), (1, self.A.T.tocsc(), y), (2, kr.full_P(self.P), x)):
            if M.shape[0] == 0 or M.shape[1] == 0 or self.m is None:
                continue
            err = kr.ratio(np.abs(apply(self.m, op, v, M.shape[0]) - M @ v), abs(M) @ np.abs(v))
            assert err <= PRODUCTS, (self.what, event, op, err)

    def rho_update(self, rho, event):
        if self.m is not None:
            oq.update_settings(self.m, rho=rho)
        self.rho = rho
        self.factorizations += 1
        self.check(event)

    def _update(self, Px, Px_idx, Ax, Ax_idx, event):
        Px = None if Px is None or len(Px) == 0 else Px
        Ax = None if Ax is None or len(Ax) == 0 else Ax
        assert Px is not None or Ax is not None
        if self.m is not None:
            oq.update(self.m, Px=Px, Px_idx=None if Px is None else Px_idx, Ax=Ax, Ax_idx=None if Ax is None else Ax_idx)
        for M, vals, idx in ((self.P, Px, Px_idx), (self.A, Ax, Ax_idx)):
            if vals is not None:
                M.data[slice(None) if idx is None else idx] = vals
        self.factorizations += 1
        self.check(event)
        self.check_products(event)

    def full_update(self, event):
        Px, Ax = full_update_values(self.rng, self.P, self.A)
        self._update(Px, None, Ax, None, event)

    def subset_update(self, event):
        Px, pidx, Ax, aidx = subset_update_values(self.rng, self.P, self.A)
        self._update(Px, pidx, Ax, aidx, event)

    def bounds_update(self, event):
        l, u = bounds_update_values(self.rng, self.l, self.u)
        if self.m is not None:
            oq.update(self.m, l=l, u=u)
        self.l, self.u = l, u
        self.factorizations += 1
        self.check(event)

    def refuses_an_indefinite_P(self):
        """The last stored diagonal entry of P far below -(rho |A_j|^2 + |P_j|): the reduced matrix P + sigma I + A' R A is
        indefinite, and with it the KKT matrix's inertia is wrong."""
        r, c = entries(self.P)
        diag = np.flatnonzero(r == c)
        if len(diag) == 0:
            return False
        k = diag[np.argmax(c[diag])]
        j = c[k]
        Aj = self.A[:, [j]]
        rho = kr.rho_vector(self.l, self.u, self.rho)
        v = -1e3 * (1.0 + float(np.sum(rho[Aj.indices] * Aj.data ** 2)) + float(abs(kr.full_P(self.P)[:, [j]]).sum()))
        with pytest.raises(oq.OSQPError):
            oq.update(self.m, Px=np.array([v]), Px_idx=np.array([k]))
        return True

    def events(self):
        """Events 1 to 6."""
        self.check("setup")
        self.rho_update(RHO1, "rho update")
        self.full_update("P and A update")
        self.subset_update("update of an index subset")
        if self.A.shape[0]:
            self.bounds_update("bounds update (row classes)")
        self.rho_update(RHO2, "second rho update")

    def run(self):
        self.events()
        return self.refuses_an_indefinite_P()

    def close(self):
        if self.m is not None:
            oq.clean(self.m)
