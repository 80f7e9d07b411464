"""Inputs of the tests of the opt-in batched path for 128 < n <= 256 (test_batch_large_host.py, test_batch_large_gpu.py; not a
test module): the six shapes, the Python transcription of the LDS layout of k_batch_solve_large (csrc/batch_solve.hpp
lds_bytes with the pivot buffers of csrc/batch_large.hpp), the certificate and gap-rule families at these sizes.  No GPU needed."""
import functools

import numpy as np
import scipy.sparse as sp

import batch_cert_cases as cert
import batch_entry_families as F
import batch_gap_cases as G
import batch_resident_ref as ref

# (kind, args of the builder, seed of the instances): seven instances each
SHAPES = [
    ("banded", (129, 193, 4), 3000),   # first n beyond 128: one row into a ninth tile block
    ("random", (144, 200, 7), 3001),   # nine exact tile blocks
    ("random", (255, 300, 7), 3002),   # one below the cap
    ("random", (256, 384, 7), 3003),   # the cap: most tiles per wavefront
    ("banded", (256, 512, 6), 3004),   # the cap with the largest LDS
    ("random", (130, 1, 7), 3005),     # a single constraint row, no rho update
]
SHAPE_IDS = ["%s-%s" % (k, "x".join(str(a) for a in args)) for k, args, _ in SHAPES]
COUNT = 7
LDS_LIMIT = 160 * 1024
NW, PIVOT_W = 8, 256  # wavefronts of the workgroup, doubles per pivot row of the inversion


def case(i):
    """The shape as a case dict of batch_entry_families (so that F.reference serves it, once per process)."""
    kind, args, seed = SHAPES[i]
    return dict(id="large-" + SHAPE_IDS[i], kind=kind, args=tuple(args), n=args[0], m=args[1], count=COUNT, opts=F.OPTS, seed=seed)


def pattern_counts(pattern):
    """(n, m, nnz(A), stored entries of the full symmetric P) of a pattern (P upper triangle, A)."""
    pat_P, pat_A = pattern
    n, m = pat_A.shape[1], pat_A.shape[0]
    U = sp.triu(pat_P, format="coo")
    ndiag = int(np.count_nonzero(U.row == U.col))
    return n, m, int(pat_A.nnz), 2 * int(U.nnz) - ndiag


def lds_bytes(n, m, nnzA, nnzF):
    """carve<256>(..., words = false): the doubles, the constraint types (m ints, padded to 16 bytes), the 16-bit pattern."""
    doubles = n + (nnzA + 1) + nnzF + 10 * n + 12 * m + 16 * NW + 24 + (2 * 4 * PIVOT_W + 64) + 1
    shorts = 2 * (n + 1) + (m + 1) + 3 * nnzA + nnzF + 8
    return doubles * 8 + ((m * 4 + 15) // 16) * 16 + shorts * 2 + 16


def tiles_per_wave(n):
    nb = (n + 15) // 16
    return (nb * (nb + 1) // 2 + NW - 1) // NW


def dense_p_pattern(n, m, seed):
    """random(n, m, seed) with a dense P: its LDS need exceeds the limit at n = 200."""
    _, pat_A = F.random(n, m, seed)
    return F._finish(sp.triu(np.ones((n, n)), format="csc"), pat_A)


# ---- statuses and certificates ---------------------------------------------------------------------------------------------
CHAINS = [(130, 20), (256, 40)]


@functools.lru_cache(None)
def chain_family(n, extra):
    probs = cert.chain(n, extra, count=6)
    return cert.stack(probs), probs


INDEFINITE_OPTS = dict(cert.OPTS, scaling=0)


def indefinite(n, extra):
    """Instance 0 of the chain family with P[1, 1] = -0.0999, to be solved under INDEFINITE_OPTS (no scaling): with the
    starting rho = 0.1 on the box row of variable 1 the reduced KKT matrix is still positive definite (pivot 1e-4 + sigma), so
    setup and the first factorisation pass; the first rho update (iteration 50) lowers rho, the re-factorisation meets a
    negative pivot, and the oracle ends OSQP_NON_CVX at iteration 50 (test_batch_large_host.py)."""
    P, q, A, l, u = cert.chain(n, extra, count=1)[0]
    P = P.copy()
    k = int(np.flatnonzero((P.indices[P.indptr[1]:P.indptr[2]] == 1))[0]) + int(P.indptr[1])
    P.data[k] = -0.0999
    return [(P, q, A, l, u)]


# ---- gap rule --------------------------------------------------------------------------------------------------------------
PF_N, PF_K = 140, 6
PF_SEEDS = (100, 102, 104, 105, 106)


@functools.lru_cache(None)
def pf_family():
    probs = [G.pf_problem(PF_N, PF_K, s) for s in PF_SEEDS]
    return ref.stack(probs), probs


_trace = {}


def pf_trace(oq, oracle_lib):
    if "pf" not in _trace:
        _trace["pf"] = [G.trace_one(oq, oracle_lib, p, G.SETTINGS) for p in pf_family()[1]]
    return _trace["pf"]
