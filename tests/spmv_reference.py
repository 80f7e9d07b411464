"""An exact reference for the sparse products y = M x (csrc/kernels.hip k_spmv, csrc/panel.hip), on the host, and the check
that goes with it.

Reference.  Every product a_ij x_j of two doubles is split without error into p + e (Dekker's TwoProduct on Veltkamp
splits; no FMA needed), and the 2 L_i terms of row i are added by math.fsum, which returns the correctly rounded value of
the exact sum: exact_i is the true row sum rounded ONCE.  S_i = sum_j |a_ij| |x_j| comes out of the same terms
(|a x| = |p| + sign(p) e, exactly), L_i is the number of STORED entries of the row, explicit zeros included -- the kernels
multiply and add those like any other entry.

Check (assert_product).  A dot product of length L evaluated in floating point in ANY order of summation, with or without
fused multiply-adds, satisfies |computed - true| <= gamma_L S with gamma_L = L u / (1 - L u), u = 2^-53 (Higham, Accuracy
and Stability of Numerical Algorithms, 2nd ed., section 3.1: the bound holds for every order of evaluation).  The
reference adds one rounding of its own (<= u |true| <= u S), and (L + 2) u >= gamma_L + u for every L < 2^25, so

    |out_i - exact_i| <= (L_i + depth + 2) 2^-53 S_i

where depth is the number of partial sums a panel path adds on top (the NG groups of the layout: the row sums of the groups
are added once more, in group order); depth = 0 on the CSR kernel.  Nothing in the bound is measured.  A row without stored
entries has S_i = 0: it must come out as +0.0 exactly (sign included).

Integer family.  When every entry of M and x is a small integer and every partial sum stays below 2^53, every order of
summation is exact: the check is array_equal against the int64 product, and a dropped, doubled or misplaced entry cannot
hide behind a tolerance."""
import math
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53
_SPLIT = 134217729.0  # 2^27 + 1


def _two_product(a, b):
    """p + e = a * b exactly (element-wise; no overflow / underflow at the magnitudes the cases use)."""
    p = a * b
    t = _SPLIT * a; ah = t - (t - a); al = a - ah
    t = _SPLIT * b; bh = t - (t - b); bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


class Product:
    """What one product y = M x must be: exact (the true row sums rounded once), S (sum |a||x| per row), L (stored entries
    per row), exact_int (the int64 product when M and x are integer-valued, else None)."""

    def __init__(self, exact, S, L, exact_int=None):
        self.exact, self.S, self.L, self.exact_int = exact, S, L, exact_int


def _is_integral(a):
    return bool(np.all(a == np.rint(a)))


def reference(M, x):
    """The exact product of the sparse matrix M (any scipy format; stored zeros are kept and counted) with x."""
    M = sp.csr_matrix(M)
    x = np.asarray(x, dtype=np.float64)
    rows = M.shape[0]
    rp, ci, va = M.indptr, M.indices, np.asarray(M.data, dtype=np.float64)
    L = np.diff(rp).astype(np.int64)
    if _is_integral(va) and _is_integral(x):
        S = np.asarray(sp.csr_matrix((np.abs(va), ci, rp), shape=M.shape) @ np.abs(x)).ravel()
        if S.size == 0 or float(S.max()) < 2.0 ** 52:  # every partial sum of every order of summation is an exact integer
            Mi = sp.csr_matrix((va.astype(np.int64), ci, rp), shape=M.shape)
            exact_int = np.asarray(Mi @ x.astype(np.int64)).ravel().astype(np.int64)
            return Product(exact_int.astype(np.float64), S, L, exact_int)
    p, e = _two_product(va, x[ci])
    sgn = np.where(p < 0, -1.0, 1.0)
    ap, ae = np.abs(p), sgn * e
    exact = np.zeros(rows)
    S = np.zeros(rows)
    for i in range(rows):
        s, t = rp[i], rp[i + 1]
        if t > s:
            exact[i] = math.fsum(np.concatenate((p[s:t], e[s:t])).tolist())
            S[i] = math.fsum(np.concatenate((ap[s:t], ae[s:t])).tolist())
    return Product(exact, S, L, None)


def reference_fraction(M, x):
    """The same row sums in rational arithmetic (small instances: the reference of the reference)."""
    M = sp.csr_matrix(M)
    out, S = [], []
    for i in range(M.shape[0]):
        acc, sabs = Fraction(0), Fraction(0)
        for k in range(M.indptr[i], M.indptr[i + 1]):
            t = Fraction(float(M.data[k])) * Fraction(float(x[M.indices[k]]))
            acc += t
            sabs += abs(t)
        out.append(acc)
        S.append(sabs)
    return out, S


def bound(prod, depth=0):
    """The per-row bound on |out - exact| (module docstring)."""
    return (prod.L + depth + 2).astype(np.float64) * U * prod.S


def error_ratio(out, prod, depth=0):
    """max_i |out_i - exact_i| / bound_i over the rows with a non-zero bound (a record for the profiles; not a check)."""
    b = bound(prod, depth)
    nz = b > 0
    if not np.any(nz):
        return 0.0
    return float(np.max(np.abs(np.asarray(out)[nz] - prod.exact[nz]) / b[nz]))


def assert_product(out, prod, depth=0, what=""):
    """out is the product `prod` describes: integer-valued cases bit for bit, real-valued ones inside the per-row bound of a
    length-L dot product; rows without stored entries are +0.0."""
    out = np.asarray(out, dtype=np.float64)
    assert out.shape == prod.exact.shape, (what, out.shape, prod.exact.shape)
    assert np.all(np.isfinite(out)), (what, "non-finite entries", np.nonzero(~np.isfinite(out))[0][:8])
    empty = prod.L == 0
    bad = np.nonzero(empty & ((out != 0.0) | np.signbit(out)))[0]
    assert bad.size == 0, (what, "rows without entries must be +0.0", bad[:8], out[bad[:8]])
    if prod.exact_int is not None:
        bad = np.nonzero(out != prod.exact_int.astype(np.float64))[0]
        assert bad.size == 0 and np.array_equal(out, prod.exact_int.astype(np.float64)), (
            what, "integer product differs in rows", bad[:8], out[bad[:8]], prod.exact_int[bad[:8]])
        return
    err = np.abs(out - prod.exact)
    b = bound(prod, depth)
    bad = np.nonzero(err > b)[0]
    assert bad.size == 0, (what, "rows outside (L + depth + 2) u S", bad[:8], err[bad[:8]], b[bad[:8]])
