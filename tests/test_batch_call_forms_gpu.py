"""The two forms of every resident call -- every instance (osqp_amd_batch_X) and a selection (osqp_amd_batch_X_rows) -- at
the corners where they differ on the host side: calls with nothing to do, the order of refusals, the whole call against the
identity selection in both pointer forms, and the results before the first solve.  The yardstick is bit-equality with the
same library on a twin handle, never a tolerance.  Two tiny families: n = 6, m = 9, five instances, and the m = 0 family of
test_batch_adjoint_gpu.test_a_batch_without_constraints (n = 5, four instances)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from osqp_jl_amd import batch
from osqp_jl_amd.interface import _iptr
from batch_resident_ref import OPTS
from test_batch_gpu import _family

pytestmark = pytest.mark.gpu

PAIRS = ("update_bounds", "update_matrices", "warm_start")  # the calls whose two arrays are both optional


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@functools.lru_cache(maxsize=None)
def _small():
    """(P0, A0, Px, Ax, q, l, u) with n = 6, m = 9, count = 5; computed once and never written to."""
    args = _family(6, 9, 5, 60905)[0]
    args = tuple(args[:2]) + tuple(np.ascontiguousarray(a, dtype=np.float64) for a in args[2:7])
    for a in args[2:]:
        a.setflags(write=False)
    return args


@functools.lru_cache(maxsize=None)
def _unconstrained():
    """m = 0, n = 5, count = 4: dense P, no rows."""
    rng = np.random.default_rng(50)
    n, count = 5, 4
    pat = sp.triu(sp.csc_matrix(np.ones((n, n))), format="csc"); pat.sort_indices()
    Px = []
    for _ in range(count):
        B = rng.standard_normal((n, n))
        U = sp.triu(sp.csc_matrix(B @ B.T + n * np.eye(n)), format="csc"); U.sort_indices()
        Px.append(U.data.copy())
    empty = np.zeros((count, 0))
    return pat, sp.csc_matrix((0, n)), np.array(Px), empty, rng.standard_normal((count, n)), empty, empty


def test_calls_with_nothing_to_do_and_the_order_of_refusals(product_lib):
    """Raw library calls after one solve: NULL arrays are a no-op in both forms, but a selection is checked first -- a bad one
    is refused even when there is nothing to do, also with m = 0.  None of it marks an instance stale or changes a bit."""
    lib = product_lib
    A, T = (batch.ResidentBatch(lib, *_small(), **OPTS) for _ in range(2))
    Z = batch.ResidentBatch(lib, *_unconstrained(), **OPTS)
    first = A.solve(); T.solve(); Z.solve()
    good, bad = np.array([3, 1], dtype=np.int64), np.array([1, 1], dtype=np.int64)
    for where in (0, 1):
        for name in PAIRS:
            assert getattr(lib, "osqp_amd_batch_" + name)(A.handle, None, None, where) == 0, name
            assert getattr(lib, "osqp_amd_batch_" + name + "_rows")(A.handle, _iptr(good), 2, None, None, where) == 0, name
            assert getattr(lib, "osqp_amd_batch_" + name + "_rows")(A.handle, _iptr(bad), 2, None, None, where) == 1, name
            assert "instance 1 is repeated" in lib.osqp_amd_last_error().decode(), name
    # m = 0: the bounds have no rows, whatever the pointers are; the selection is still checked
    some = np.zeros(8)
    for l, u in ((None, None), (some.ctypes.data, some.ctypes.data)):
        assert lib.osqp_amd_batch_update_bounds(Z.handle, l, u, 0) == 0
        assert lib.osqp_amd_batch_update_bounds_rows(Z.handle, _iptr(good), 2, l, u, 0) == 0
        assert lib.osqp_amd_batch_update_bounds_rows(Z.handle, _iptr(bad), 2, l, u, 0) == 1
        assert "instance 1 is repeated" in lib.osqp_amd_last_error().decode()
    # nothing was marked stale: the derivative calls refuse a stale instance by name
    assert np.all(A.adjoint(dx=np.ones((A.count, A.n)))["status"] == 1)
    assert np.all(Z.adjoint(dx=np.ones((Z.count, Z.n)))["status"] == 1)
    second, twin = A.solve(), T.solve()
    A.close(); T.close(); Z.close()
    assert np.all(first[2][:, 1] == 1)
    for got, want in zip(second, twin):
        assert _same(got, want)


@pytest.mark.parametrize("form", ["host", "device"])
def test_a_whole_call_is_the_identity_selection(product_lib, form):
    """update(q), update(l, u), update(Ax), warm_start(x, y), solve() and the results that follow, with polish on: the whole
    calls on one handle, `rows=arange(count)` on its twin, bit for bit."""
    lib = product_lib
    P0, A0, Px, Ax, q, l, u = _small()
    count, n, m = q.shape[0], q.shape[1], l.shape[1]
    rng = np.random.default_rng(7)
    q2, l2, u2, Ax2 = 1.1 * q, l - 0.1, u + 0.1, Ax * (1.0 + 0.05 * rng.standard_normal(Ax.shape))
    x0, y0 = 0.1 * rng.standard_normal((count, n)), 0.1 * rng.standard_normal((count, m))

    def arr(a):
        return a if form == "host" else batch.DeviceArray(lib, *a.shape).upload(a)

    def empty(*shape):
        return None if form == "host" else batch.DeviceArray(lib, *shape)

    def host(a):
        return a if isinstance(a, np.ndarray) else a.numpy()

    results = []
    for rows in (None, np.arange(count)):
        rb = batch.ResidentBatch(lib, P0, A0, Px, Ax, q, l, u, **dict(OPTS, polish=True))
        rb.update(q=arr(q2), rows=rows)
        rb.update(l=arr(l2), u=arr(u2), rows=rows)
        rb.update(Ax=arr(Ax2), rows=rows)
        rb.warm_start(x=arr(x0), y=arr(y0), rows=rows)
        out = None if form == "host" else (empty(count, n), empty(count, m), empty(count, 6))
        got = list(rb.solve(out=out, rows=rows))
        got.append(rb.polish_status(out=empty(count, 1), rows=rows))
        got.extend(rb.certificates(out=None if form == "host" else (empty(count, m), empty(count, n)), rows=rows))
        got.append(rb.duality(out=empty(count, 3), rows=rows))
        got = [np.asarray(host(a), dtype=np.float64).reshape(count, -1) for a in got]
        got.extend(rb.solve())
        rb.close()
        results.append(got)
    whole, selected = results
    assert np.all(whole[2][:, 1] == 1) and np.any(whole[3] != 0)  # solved, and polish ran
    assert len(whole) == len(selected) == 10
    for j, (a, b) in enumerate(zip(whole, selected)):
        assert _same(a, b), j


def test_results_of_a_selection_before_the_first_solve(product_lib):
    """polish_status is zeros and the certificates are NaN, in both pointer forms; a device array is overwritten."""
    lib = product_lib
    rb = batch.ResidentBatch(lib, *_small(), **dict(OPTS, polish=True))
    rows = [4, 0]
    ones = lambda *shape: batch.DeviceArray(lib, *shape).upload(np.ones(shape))
    st = rb.polish_status(rows=rows)
    p, d = rb.certificates(rows=rows)
    st_dev = rb.polish_status(out=ones(2, 1), rows=rows).numpy()
    p_dev, d_dev = (a.numpy() for a in rb.certificates(out=(ones(2, rb.m), ones(2, rb.n)), rows=rows))
    rb.close()
    assert st.shape == (2,) and np.all(st == 0) and st_dev.shape == (2, 1) and np.all(st_dev == 0)
    assert p.shape == p_dev.shape == (2, rb.m) and d.shape == d_dev.shape == (2, rb.n)
    assert np.all(np.isnan(p)) and np.all(np.isnan(d)) and np.all(np.isnan(p_dev)) and np.all(np.isnan(d_dev))
