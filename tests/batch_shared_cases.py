"""Families and the reference of the shared-batch tests (batch.SharedBatch: one model, many right-hand sides).

Boxed family: the base (P0, q0, A0, l0, u0) is `F.instances(F.pattern(kind, shape), 1, seed)`; instance i draws, in sequence from
default_rng(seed + 1000), x0 = N(0,1)^n, w = 0.05 + U(0,1)^m, q = N(0,1)^n (1 + 3 (i % 3)) and takes l, u = A0 x0 -+ w.  With
neq > 0 the first neq rows are equalities in the base (u0[:neq] = l0[:neq]) and in every instance (l = u = (A0 x0)[:neq]).
Chain family: P and A of the dual-infeasible recipe of batch_cert_cases.chain (variable 0 costs nothing and its rows are
loose, in the base and in every instance); instance i % 3 == 1 is primal infeasible, i % 3 == 2 dual infeasible.
The reference is `OracleShared`: one oracle model per instance, set up on the BASE data and then updated -- the definition of
an instance of a shared batch.  No GPU needed: tests/test_batch_shared_host.py holds the families to what the GPU tests rest on."""
import numpy as np
import scipy.sparse as sp

import osqp_jl_amd as oq
import batch_cert_cases as CC
import batch_entry_families as F

OPTS = dict(F.OPTS, adaptive_rho=0, rho=1.0)

# id -> (kind, shape, seed, neq, instances)
BOXED = {
    "banded-17": ("banded", (17, 23, 3), 11, 0, 7),
    "banded-100": ("banded", (100, 200, 4), 12, 0, 7),
    "random-144": ("random", (144, 200, 7), 13, 0, 7),
    "banded-256": ("banded", (256, 512, 6), 14, 0, 5),
    "banded-129-eq": ("banded", (129, 193, 4), 15, 20, 7),
    "banded-33-eq": ("banded", (33, 40, 3), 16, 5, 7),
}
# The edges of the dense step (tests/test_batch_shared_steps_*.py): id -> (kind, shape, seed, neq, T, ldm, ntile).  T is the
# number of instances per workgroup that batch.shared_plan gives the shape, ldm = 16 ceil(n / 16) and ntile = ldm / 16 what the
# matrix-core product branches on; each batch has 2 T + 3 instances: two full tiles and a partial one.
EDGES = {
    "banded-2": ("banded", (2, 2, 1), 51, 0, 16, 16, 1),             # smallest; 14 padding rows (the seed: max E <= 2 c, see
                                                                     # test_batch_shared_steps_host.py)
    "banded-15": ("banded", (15, 20, 3), 55, 0, 16, 16, 1),          # the tail chunk only; one padding row
    "banded-16": ("banded", (16, 24, 3), 56, 0, 16, 16, 1),          # one exact tile, no padding
    "banded-32-eq": ("banded", (32, 48, 3), 72, 4, 16, 32, 2),       # one full 32-column chunk, no tail; equalities
    "banded-128": ("banded", (128, 192, 4), 168, 0, 16, 128, 8),     # ntile = the number of wavefronts: no second tile
    "banded-130-m400": ("banded", (130, 400, 5), 170, 0, 8, 144, 9),  # T = 8; only wavefront 0 holds two tiles
    "banded-176-eq": ("banded", (176, 300, 5), 216, 8, 8, 176, 11),  # T = 8; a tail chunk with two tiles; equalities
    "banded-240": ("banded", (240, 360, 5), 280, 0, 8, 240, 15),     # T = 8; odd tile count
    "banded-241-eq": ("banded", (241, 400, 5), 281, 6, 8, 256, 16),  # T = 8; 15 padding rows in the last tile; LDS nearly full
    "banded-200-m460": ("banded", (200, 460, 5), 240, 0, 4, 208, 13),  # T = 4 away from n = 256; ldm an odd multiple of 16
}
BOXED.update({name: (kind, shape, seed, neq, 2 * T + 3) for name, (kind, shape, seed, neq, T, _, _) in EDGES.items()})
CHAINS = [(17, 5), (130, 20), (256, 40)]
CHAIN_STATUS = [1, -3, -4] * 3
CHAIN_STATUS_30 = [2, -3, -4, -2, -3, -4, 2, -3, -4]  # max_iter = 30, rho = 1.0


def boxed(name, count=None):
    """(base (P0, q0, A0, l0, u0), q [count x n], l, u [count x m])."""
    kind, shape, seed, neq, cnt = BOXED[name]
    return boxed_spec(kind, shape, seed, neq, cnt if count is None else count)


def boxed_spec(kind, shape, seed, neq, count):
    """The boxed family on any pattern of batch_entry_families (tools/batch_shared.py times it at 4096 instances)."""
    _, probs = F.instances(F.pattern(kind, shape), 1, seed)
    P0, q0, A0, l0, u0 = probs[0]
    l0, u0 = l0.copy(), u0.copy()
    u0[:neq] = l0[:neq]
    n, m = A0.shape[1], A0.shape[0]
    rng = np.random.default_rng(seed + 1000)
    q, l, u = np.empty((count, n)), np.empty((count, m)), np.empty((count, m))
    for i in range(count):
        x0 = rng.standard_normal(n)
        w = 0.05 + rng.random(m)
        q[i] = rng.standard_normal(n) * (1 + 3 * (i % 3))
        ax = A0 @ x0
        l[i], u[i] = ax - w, ax + w
        l[i, :neq] = u[i, :neq] = ax[:neq]
    return (P0, q0, A0, l0, u0), q, l, u


def unconstrained(n=33, count=5, seed=21):
    """The m = 0 shape: P from `banded`, no rows."""
    pat_P, _ = F.banded(n, 40, 3)
    _, probs = F.instances((pat_P, sp.csc_matrix((0, n))), 1, seed)
    P0, q0, A0, l0, u0 = probs[0]
    rng = np.random.default_rng(seed + 1000)
    q = rng.standard_normal((count, n))
    return (P0, q0, sp.csc_matrix((0, n)), np.zeros(0), np.zeros(0)), q, np.zeros((count, 0)), np.zeros((count, 0))


def chain(n, extra, count=9):
    P, _, A, l0, u0 = CC.chain(n, extra, count=3)[2]
    m = A.shape[0]
    q0 = np.random.default_rng(5).standard_normal(n)
    q0[0] = 0.0
    q, l, u = np.empty((count, n)), np.tile(l0, (count, 1)), np.tile(u0, (count, 1))
    Ad = A.toarray()
    for i in range(count):
        q[i] = np.random.default_rng(200 + i).standard_normal(n)
        q[i, 0] = 0.0
        if i % 3 == 1:
            l[i, n + 1] = float(np.sum(np.abs(Ad[n + 1]))) + 1.0
            u[i, n + 1] = l[i, n + 1] + 1.0
        if i % 3 == 2:
            q[i, 0] = -1.0
    return (P, q0, A, l0.copy(), u0.copy()), q, l, u


def perturbed(l, u, q, seed=7):
    """The recipe of batch_resident_ref.closed_loop_steps for one step, but the noise goes onto l AND u of each of the first six
    rows, so that u - l of every row -- and with it the kind of the row -- stays as it is."""
    rng = np.random.default_rng(seed)
    l, u, q = l.copy(), u.copy(), q.copy()
    k = min(6, l.shape[1])
    for i in range(l.shape[0]):
        d = 0.01 * rng.standard_normal(k)
        l[i, :k] += d; u[i, :k] += d
        q[i, :min(6, q.shape[1])] *= 1 + 0.02 * rng.standard_normal(min(6, q.shape[1]))
    return q, l, u


class OracleShared:
    """One oracle model per instance with the call surface of `batch.SharedBatch`: every model is set up on the base data."""

    def __init__(self, oracle_lib, base, count, **opts):
        P, q0, A, l0, u0 = base
        self.m = A.shape[0]
        self.models = []
        for _ in range(count):
            mdl = oq.Model(oracle_lib)
            oq.setup(mdl, P=P, q=q0, A=A, l=l0, u=u0, **opts)
            self.models.append(mdl)

    def update(self, q=None, l=None, u=None):
        for i, mdl in enumerate(self.models):
            if q is not None:
                oq.update(mdl, q=q[i])
            if l is not None and self.m:
                oq.update(mdl, l=l[i], u=u[i])

    def warm_start(self, x=None, y=None):
        for i, mdl in enumerate(self.models):
            oq.warm_start(mdl, x=None if x is None else x[i], y=None if y is None or not self.m else y[i])

    def update_settings(self, **kw):
        """`oq.update_settings`; scaled_termination, which that function does not list, goes to the oracle's own symbol."""
        kw = dict(kw)
        scaled = kw.pop("scaled_termination", None)
        for mdl in self.models:
            oq.update_settings(mdl, **kw)
            if scaled is not None:
                assert mdl.lib.osqp_update_scaled_termination(mdl.workspace, int(scaled)) == 0

    def solve(self):
        return [oq.solve(mdl) for mdl in self.models]

    def close(self):
        for mdl in self.models:
            oq.clean(mdl)
        self.models = []


_REF = {}


def reference(oracle_lib, key, base, q, l, u, **opts):
    """Setup on the base, update, solve: computed once per key and shared."""
    if key not in _REF:
        ob = OracleShared(oracle_lib, base, q.shape[0], **opts)
        ob.update(q=q, l=l, u=u)
        _REF[key] = ob.solve()
        ob.close()
    return _REF[key]
