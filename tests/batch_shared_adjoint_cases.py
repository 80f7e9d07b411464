"""Families, references and filters of the adjoint of the shared batch (`SharedBatch.adjoint`, osqp_amd_shared_batch_adjoint;
k_shared_adjoint and k_shared_reduce_rows in osqp.jl_amd/csrc/batch_shared_adjoint.hpp).

Families: `batch_shared_cases.boxed_spec(kind, shape, seed, neq, count)` with count = 2 T + 3 (T: the instances per workgroup of
the solve kernel for the shape), each the boundary of something in the adjoint kernel -- CASES below.  The existing
`banded-129-eq` is NOT used: its 20 equality rows are rank deficient (cond K ~ 1e17 on every instance).
Reference of the gradients: `batch_adjoint_ref.exact` (the dense KKT solve of the active set, caller's units) and
`batch_adjoint_ref.model` (the kernel's algorithm on the scaled state); an instance of a shared batch carries the scaling of
the BASE data, which `oracle_states` reads from oracle models set up on the base and then updated.
Reference of the summed matrix gradients: `block_sum`, the order of include/osqp_amd.h as a numpy loop.
No GPU needed; tests/test_batch_shared_adjoint_host.py holds this file to what the GPU tests rest on."""
import numpy as np
import scipy.sparse as sp

import osqp_jl_amd as oq
import batch_adjoint_ref as adj
import batch_polish_ref as pol
import batch_shared_cases as S

# id -> (kind, shape, seed, neq, T): what it is the boundary of
CASES = {
    "banded-17": ("banded", (17, 23, 3), 11, 0, 16),        # smallest; factor in LDS
    "banded-33-eq": ("banded", (33, 40, 3), 16, 5, 16),     # equalities; factor in LDS
    "banded-128": ("banded", (128, 192, 4), 18, 0, 16),     # last n of the LDS form
    "random-129-eq": ("random", (129, 160, 5), 17, 12, 16),  # first n of the scratch form, equalities, n no multiple of 32
    "banded-256": ("banded", (256, 512, 6), 14, 0, 4),      # the cap; T = 4
    "banded-240": ("banded", (240, 360, 5), 281, 0, 8),     # T = 8: the stride of the tile records; ldm = 240, 15 tiles of 16
}
COND_MAX = 1e8
BLOCK = 16


def count_of(name):
    return 2 * CASES[name][4] + 3


def family(name, count=None):
    """(base (P0, q0, A0, l0, u0), q [count x n], l, u [count x m]); instance i is the same whatever count is."""
    kind, shape, seed, neq, _ = CASES[name]
    return S.boxed_spec(kind, shape, seed, neq, count_of(name) if count is None else count)


def block_sum(rows):
    """The sum over axis 0 of rows [count x cols] in the order of the contract: s_b = ((r_16b + r_16b+1) + ...) over each block
    of 16 consecutive rows, then ((s_0 + s_1) + ...).  Plain IEEE additions, one at a time."""
    rows = np.asarray(rows, dtype=np.float64)
    total = None
    for b in range(0, rows.shape[0], BLOCK):
        s = rows[b].copy()
        for j in range(b + 1, min(b + BLOCK, rows.shape[0])):
            s = s + rows[j]
        total = s if total is None else total + s
    return total


def well_conditioned(P, A, act):
    """The derivative exists and `exact` can be trusted as a reference: no more active rows than variables, full row rank,
    and cond K <= 1e8 for K = [P, Aa'; Aa, 0] (np.linalg.solve then carries ~1e-8 of relative error at worst)."""
    n = A.shape[1]
    rows = np.flatnonzero(act)
    if len(rows) > n:
        return False
    Aa = sp.csr_matrix(A)[rows].toarray()
    if len(rows) and np.linalg.matrix_rank(Aa) < len(rows):
        return False
    K = np.block([[adj.full_P(P), Aa.T], [Aa, np.zeros((len(rows), len(rows)))]])
    return bool(np.linalg.cond(K) <= COND_MAX)


def cotangents(name, ncot, count, n, m):
    """The incoming gradients the tests of a family share: g_x [ncot x count x n], g_y [ncot x count x m].  Drawn instance by
    instance, so that instance i has the same cotangents whatever count is."""
    gx, gy = np.empty((ncot, count, n)), np.empty((ncot, count, m))
    for i in range(count):
        rng = np.random.default_rng([sum(map(ord, name)), i])
        gx[:, i], gy[:, i] = rng.standard_normal((ncot, n)), rng.standard_normal((ncot, m))
    return gx, gy


_states = {}


def oracle_states(oracle_lib, name):
    """[dict(status, x, y, state = (D, E, c, xs, zs, ys), act)] of the family's instances from oracle models set up on the BASE
    data and updated -- the definition of an instance of a shared batch (S.OracleShared).  Computed once per session."""
    if name not in _states:
        base, q, l, u = family(name)
        n, m = q.shape[1], l.shape[1]
        ob = S.OracleShared(oracle_lib, base, q.shape[0], **S.OPTS)
        ob.update(q=q, l=l, u=u)
        out = []
        for i, (mdl, r) in enumerate(zip(ob.models, ob.solve())):
            st = pol.oracle_state(mdl, n, m, S.OPTS.get("scaling", 10))
            D, E, c, xs, zs, ys = st
            ls, us = np.maximum(l[i], -pol.OSQP_INFTY) * E, np.minimum(u[i], pol.OSQP_INFTY) * E
            out.append(dict(status=r.info.status_val, x=np.array(r.x), y=np.array(r.y), state=st, act=adj.classify(zs, ys, ls, us)))
        ob.close()
        _states[name] = out
    return _states[name]
