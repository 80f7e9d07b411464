"""Families, tangents and references of the forward sensitivities of the shared batch (`SharedBatch.jvp`,
osqp_amd_shared_batch_jvp; k_shared_jvp in osqp.jl_amd/csrc/batch_shared_jvp.hpp).

Families: those of the adjoint of the shared batch (tests/batch_shared_adjoint_cases.py: CASES, `family`, `oracle_states`,
`well_conditioned`, `cotangents`), each the boundary of something in the kernel the two calls share.
Tangents: `tangents(name, ndir, count)` -- q, l, u per instance, drawn instance by instance (instance i has the same tangent
whatever count is), tu = tl on the rows with l == u; Px, Ax ONE row per direction for the whole batch, drawn from the name alone.
References: `batch_jvp_ref.exact` (the dense KKT solve of the active set, caller's units) and `batch_jvp_ref.model` (the
kernel's algorithm on the scaled state); both work unchanged on the base-scaled states of `oracle_states`, and an instance sees
the shared matrix tangent as its own.
No GPU needed; tests/test_batch_shared_jvp_host.py holds this file to what the GPU tests rest on."""
import numpy as np

import batch_adjoint_ref as adj
import batch_shared_adjoint_cases as SA

CASES = SA.CASES
count_of, family, oracle_states, well_conditioned, cotangents = SA.count_of, SA.family, SA.oracle_states, SA.well_conditioned, SA.cotangents
TANGENTS = ("q", "l", "u", "Px", "Ax")
SHARED = ("Px", "Ax")


def tangents(name, ndir, count=None):
    """dict of q [ndir x count x n], l, u [ndir x count x m], Px [ndir x nnzP], Ax [ndir x nnzA] of the family `name`."""
    base, q, l, u = family(name, count)
    count, n, m = q.shape[0], q.shape[1], l.shape[1]
    (pi, _), (ai, _) = adj.patterns(base[0], base[2])
    d = dict(q=np.empty((ndir, count, n)), l=np.empty((ndir, count, m)), u=np.empty((ndir, count, m)))
    for i in range(count):
        rng = np.random.default_rng([sum(map(ord, name)), i, 7])
        d["q"][:, i], d["l"][:, i], d["u"][:, i] = rng.standard_normal((ndir, n)), rng.standard_normal((ndir, m)), rng.standard_normal((ndir, m))
    d["u"] = np.where((l == u)[None], d["l"], d["u"])  # an equality row moves as one
    rng = np.random.default_rng([sum(map(ord, name)), 77])
    d["Px"], d["Ax"] = rng.standard_normal((ndir, len(pi))), rng.standard_normal((ndir, len(ai)))
    return d


def direction(d, k, i):
    """Direction k of `tangents` as instance i sees it: its own q, l, u and the shared Px, Ax."""
    return {name: (a[k] if name in SHARED else a[k, i]) for name, a in d.items()}
