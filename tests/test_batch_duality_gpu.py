"""Primal objective, dual objective and duality gap of the resident batch (`ResidentBatch.duality`, osqp_amd_batch_duality,
DESIGN.md section 19) on the GPU: every row against the numpy statement (duality_ref.py) on the pair the solve returned for
that instance, at the derived rounding bound 4 (N + 8) 2^-53 S; the selection and device forms against the whole host call,
bit for bit; staleness; and that the call only reads the handle."""
import numpy as np
import pytest
import scipy.sparse as sp

from osqp_jl_amd import batch
from osqp_jl_amd.interface import OSQPError
import batch_cert_cases as cert_cases
import batch_entry_families as fam
import batch_resident_ref as ref
import duality_ref

pytestmark = pytest.mark.gpu

NO_SOLUTION = (-3, 3, -4, 4, -7)


def _no_rows(n, count, seed):
    """A pattern with m = 0: `count` strictly convex QPs without constraints."""
    rng = np.random.default_rng(seed)
    pat = sp.triu(sp.diags([np.ones(n - 1), np.ones(n), np.ones(n - 1)], [-1, 0, 1]), format="csc")
    pat.sort_indices()
    probs = []
    for _ in range(count):
        U = pat.copy()
        U.data = 0.3 * rng.standard_normal(U.nnz)
        full = (U + U.T).tolil()
        full.setdiag(np.asarray(abs(U + U.T).sum(axis=1)).ravel() + 0.1 + rng.random(n))
        P = sp.triu(full.tocsc(), format="csc"); P.sort_indices()
        probs.append((P, rng.standard_normal(n), sp.csc_matrix((0, n)), np.zeros(0), np.zeros(0)))
    args = (pat, sp.csc_matrix((0, n)), np.array([p[0].data for p in probs]), np.zeros((count, 0)), np.array([p[1] for p in probs]),
            np.zeros((count, 0)), np.zeros((count, 0)))
    return args, probs


def _family(name, oracle_lib):
    """(what ResidentBatch takes, [(P, q, A, l, u)], settings)"""
    if name in ("mpc", "mpc_polished"):
        probs = ref.mpc_instances(oracle_lib, 0, 8, 2)
        return ref.stack(probs), probs, dict(ref.OPTS, polish=name == "mpc_polished")
    if name == "banded":
        args, probs = fam.instances(fam.banded(128, 192, 4), 3, 11)
        return args, probs, dict(fam.OPTS)
    if name == "random":
        args, probs = fam.instances(fam.random(32, 48, 7), 3, 12)
        return args, probs, dict(fam.OPTS)
    if name == "no_rows":
        args, probs = _no_rows(7, 3, 13)
        return args, probs, dict(fam.OPTS)
    assert name == "infeasible"
    probs = cert_cases.mpc(oracle_lib, 3)  # instance 0 solvable, 1 primal infeasible, 2 dual infeasible
    return cert_cases.stack(probs), probs, dict(cert_cases.OPTS)


FAMILIES = ("mpc", "mpc_polished", "banded", "random", "no_rows", "infeasible")


def _check_rows(d, x, y, info, probs, tag):
    for i, (P, q, A, l, u) in enumerate(probs):
        if int(info[i, 1]) in NO_SOLUTION:
            assert np.all(np.isnan(d[i])), (tag, i, d[i])
            continue
        r = duality_ref.duality(P, q, A, l, u, x[i], y[i])
        tol = duality_ref.tolerance(r)
        got = dict(prim_obj=d[i, 0], dual_obj=d[i, 1], gap=d[i, 2])
        for key in got:
            print(f"{tag} inst {i} {key}: kernel {got[key]:.17g} numpy {r[key]:.17g} |diff| {abs(got[key] - r[key]):.3e} tol {tol:.3e}")
        for key in got:
            assert abs(got[key] - r[key]) <= tol, (tag, i, key, got[key], r[key], tol)
        assert abs(d[i, 0] - info[i, 4]) <= tol, (tag, i, d[i, 0], info[i, 4])  # info's obj_val: the same terms


@pytest.mark.parametrize("name", FAMILIES)
def test_rows_against_numpy_and_the_other_forms(product_lib, oracle_lib, name):
    args, probs, opts = _family(name, oracle_lib)
    rb = batch.ResidentBatch(product_lib, *args, **opts)
    x, y, info = rb.solve()
    d = rb.duality()
    assert d.shape == (rb.count, 3)
    if name == "infeasible":
        assert [int(s) for s in info[:, 1]] == [1, -3, -4]
    _check_rows(d, x, y, info, probs, name)
    # the same bits on every call, from the device form, and row by row from a selection
    assert np.array_equal(rb.duality(), d, equal_nan=True)
    dev = batch.DeviceArray(product_lib, rb.count, 3)
    assert rb.duality(out=dev) is dev and np.array_equal(dev.numpy(), d, equal_nan=True)
    dev.free()
    rows = [rb.count - 1, 0] if rb.count > 2 else [0]
    part = rb.duality(rows=rows)
    assert part.shape == (len(rows), 3) and np.array_equal(part, d[rows], equal_nan=True)
    dev = batch.DeviceArray(product_lib, len(rows), 3)
    rb.duality(out=dev, rows=rows)
    assert np.array_equal(dev.numpy(), d[rows], equal_nan=True)
    dev.free()
    rb.close()


def test_a_stale_instance_is_refused_by_name(product_lib, oracle_lib):
    args, probs, opts = _family("random", oracle_lib)
    rb = batch.ResidentBatch(product_lib, *args, **opts)
    with pytest.raises(OSQPError, match="instance 0 of the batch holds no current solution"):
        rb.duality()  # nothing has been solved yet
    rb.solve()
    d = rb.duality()
    rb.update(q=args[4][1:2] * 1.5, rows=[1])
    with pytest.raises(OSQPError, match="instance 1 of the batch holds no current solution"):
        rb.duality()
    with pytest.raises(OSQPError, match="instance 1 of the batch holds no current solution"):
        rb.duality(rows=[0, 1])
    assert np.array_equal(rb.duality(rows=[2, 0]), d[[2, 0]])  # the others are current and unchanged
    rb.solve(rows=[1])
    d2 = rb.duality()
    assert np.array_equal(d2[[0, 2]], d[[0, 2]]) and not np.array_equal(d2[1], d[1])
    assert product_lib.osqp_amd_batch_duality(None, None, 0) == 1
    assert product_lib.osqp_amd_batch_duality(rb.handle, None, 0) == 1
    rb.close()


@pytest.mark.parametrize("name", ["mpc_polished", "infeasible"])
def test_the_call_only_reads_the_handle(product_lib, oracle_lib, name):
    args, probs, opts = _family(name, oracle_lib)
    res = []
    for ask in (True, False):
        rb = batch.ResidentBatch(product_lib, *args, **opts)
        first = rb.solve()
        if ask:
            rb.duality()
            rb.duality(rows=[1])
        rb.update(q=args[4] * 1.01)
        second = rb.solve()
        res.append(first + second + rb.certificates())
        rb.close()
    for a, b in zip(*res):
        if a is None:
            assert b is None
            continue
        assert np.array_equal(a, b, equal_nan=True)
