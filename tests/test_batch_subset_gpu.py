"""Subset calls of the resident batch on the GPU: `update(rows=)`, `warm_start(rows=)`, `solve(rows=)` of
batch.ResidentBatch (osqp_amd_batch_*_rows).

The yardstick is bit-equality with the SAME library on sub-batches, never a tolerance.  For a selection `sel`, unsorted,
three handles are built from one family: A from all instances, S from the instances `sel` in that order, R from the rest.
A subset call on A must give what the whole-batch call gives on S, and must leave the other instances of A exactly where R
is.  Four families as in test_batch_resident_gpu.py: the MPC family on the fixed entry of the four-wavefront kernel and
(OSQP_AMD_BATCH_QUAD=0) on the 512-thread kernel, a generated family on a run-time entry, and one with 300 rows that only
the 512-thread kernel takes."""
import functools

import numpy as np
import pytest

from osqp_jl_amd import batch
from osqp_jl_amd.interface import _iptr
import batch_cert_cases as cases
import batch_resident_ref as ref
from batch_resident_ref import OPTS
from test_batch_gpu import _family

pytestmark = pytest.mark.gpu

FAMILIES = ["mpc", "quad64", "rows300", "mpc512"]
VARIANTS = [dict(), dict(adaptive_rho=0), dict(warm_start=False)]
# what a subset call changes, and the settings it is run under on top of the variant (matrix values with scaling on and off:
# only the selected instances may be re-equilibrated)
KINDS = [("q", {}), ("bounds", {}), ("matrices", dict(scaling=10)), ("matrices", dict(scaling=0)), ("warm", {})]


@functools.lru_cache(maxsize=None)
def _stacked(oracle_lib, family):
    """(P0, A0, Px, Ax, q, l, u) of a family, computed once per session and never written to."""
    if family in ("mpc", "mpc512"):
        args = ref.stack(ref.mpc_instances(oracle_lib, 0, 8, 2))
    elif family == "quad64":
        args = _family(64, 100, 6, 640100)[0]
    elif family == "rows300":
        args = _family(40, 300, 5, 40300)[0]
    else:
        args = cases.stack(cases.mpc(oracle_lib, 8))
    args = tuple(args[:2]) + tuple(np.ascontiguousarray(a, dtype=np.float64) for a in args[2:7])
    for a in args[2:]:
        a.setflags(write=False)
    return args


def _family_args(oracle_lib, family, monkeypatch):
    if family == "mpc512":
        monkeypatch.setenv("OSQP_AMD_BATCH_QUAD", "0")
    return _stacked(oracle_lib, family), {"mpc": 0, "quad64": 1, "rows300": -1, "mpc512": -1}[family]


def _check_kernel(lib, kernel):
    got = lib.osqp_amd_batch_last_kernel()
    assert (got >= 1) if kernel == 1 else (got == kernel), (got, kernel)


def _rows(args, idx):
    return tuple(args[:2]) + tuple(a[idx] for a in args[2:])


def _selection(count):
    """An unsorted selection that ends on the last instance and holds instance 2 (of the MPC family: the one whose scaling
    shows), and the instances it leaves out."""
    sel = np.array([count - 1, 0, 2])
    return sel, np.array([i for i in range(count) if i not in sel])


def _handles(lib, args, sel, rest, opts):
    return (batch.ResidentBatch(lib, *args, **opts), batch.ResidentBatch(lib, *_rows(args, sel), **opts),
            batch.ResidentBatch(lib, *_rows(args, rest), **opts))


def _same(a, b):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


def _assert_same(a, b, tag):
    for name, p, q in zip(("x", "y", "info"), a, b):
        assert p.shape == q.shape, (tag, name, p.shape, q.shape)
        assert np.array_equal(p, q, equal_nan=True), (tag, name, np.argwhere(~((p == q) | (np.isnan(p) & np.isnan(q))))[:4])


def _take(res, idx):
    return tuple(r[idx] for r in res)


def _change(kind, args, sel, first):
    """The compact [k x .] arguments of the subset call of this kind on the selected instances: update keywords, or the
    iterate of a warm start (x, y of the first solve, moved a little)."""
    Px, Ax, q, l, u = (a[sel] for a in args[2:])
    rng = np.random.default_rng(23)
    width = np.where(np.isfinite(u - l), u - l, 0.0)
    if kind == "q":
        return dict(q=q * (1 + 0.05 * rng.standard_normal(q.shape)))
    if kind == "bounds":
        return dict(l=l - 0.02 * width, u=u + 0.03 * width)
    if kind == "matrices":
        return dict(Px=Px * 1.1, Ax=Ax * (1 + 0.02 * rng.standard_normal(Ax.shape)))
    x, y = first[0][sel], first[1][sel]
    return dict(x=np.nan_to_num(x) * 0.9 + 0.01, y=np.nan_to_num(y) * 1.1)


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("family", FAMILIES)
def test_subset_equals_sub_batch(product_lib, oracle_lib, monkeypatch, family, variant):
    """After a first whole solve of all three handles: the subset call and `solve(rows=sel)` on A against the whole-batch
    calls on S; then one more whole solve of A, whose rows `sel` must be S's next solve and whose other rows R's second --
    the subset calls touched no record but the selected ones.  Every kind of change, under every variant."""
    args, kernel = _family_args(oracle_lib, family, monkeypatch)
    count = args[4].shape[0]
    sel, rest = _selection(count)
    for kind, extra in KINDS:
        opts = dict(OPTS, **VARIANTS[variant], **extra)
        tag = f"{family}/{variant}/{kind}/{extra}"
        A, S, R = _handles(product_lib, args, sel, rest, opts)
        first = A.solve()
        _assert_same(_take(first, sel), S.solve(), tag + " first, selected")
        _assert_same(_take(first, rest), R.solve(), tag + " first, others")
        change = _change(kind, args, sel, first)
        if kind == "warm":
            A.warm_start(rows=sel, **change); S.warm_start(**change)
            R.update_settings(warm_start=1)  # warm_start is a setting of the handle that any warm start switches on: A's is on now
        else:
            A.update(rows=sel, **change); S.update(**change)
        got = A.solve(rows=sel)
        _check_kernel(product_lib, kernel)
        assert batch.last_schedule(product_lib)["instances"] == len(sel)
        _assert_same(got, S.solve(), tag + " subset solve")
        whole = A.solve()
        _check_kernel(product_lib, kernel)
        _assert_same(_take(whole, sel), S.solve(), tag + " next whole solve, selected")
        _assert_same(_take(whole, rest), R.solve(), tag + " next whole solve, others")
        A.close(); S.close(); R.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_full_selection_is_the_whole_call(product_lib, oracle_lib, monkeypatch, family):
    """rows = arange(count) gives the bits of rows = None, call by call."""
    args, kernel = _family_args(oracle_lib, family, monkeypatch)
    count = args[4].shape[0]
    every = np.arange(count)
    A = batch.ResidentBatch(product_lib, *args, **OPTS)
    T = batch.ResidentBatch(product_lib, *args, **OPTS)
    _assert_same(A.solve(rows=every), T.solve(), family + " first")
    _check_kernel(product_lib, kernel)
    q2 = args[4] * 1.03
    A.update(q=q2, Ax=args[3] * 0.99, rows=every); T.update(q=q2, Ax=args[3] * 0.99)
    _assert_same(A.solve(rows=every), T.solve(), family + " after update")
    x0 = np.nan_to_num(T.solve()[0]) * 0.5
    A.solve()
    A.warm_start(x=x0, rows=np.ones(count, dtype=bool)); T.warm_start(x=x0)
    _assert_same(A.solve(rows=every), T.solve(), family + " after warm start")
    _assert_same(A.solve(), T.solve(rows=every), family + " last")
    A.close(); T.close()


def test_launch_size(product_lib, oracle_lib):
    """A subset solve launches k workgroups in the ADMM launch, one k_batch_cert, and with polish on one k_batch_polish."""
    args = _stacked(oracle_lib, "mpc")
    sel = np.array([5, 0, 3])
    A = batch.ResidentBatch(product_lib, *args, **OPTS)
    A.solve()
    assert batch.last_schedule(product_lib)["instances"] == 8
    n_cert, n_pol = product_lib.osqp_amd_batch_cert_launches(), product_lib.osqp_amd_batch_polish_launches()
    A.solve(rows=sel)
    assert batch.last_schedule(product_lib)["instances"] == 3
    assert product_lib.osqp_amd_batch_cert_launches() == n_cert + 1
    assert product_lib.osqp_amd_batch_polish_launches() == n_pol
    A.update_polish(1)
    A.solve(rows=sel[:2])
    assert batch.last_schedule(product_lib)["instances"] == 2
    assert product_lib.osqp_amd_batch_cert_launches() == n_cert + 2
    assert product_lib.osqp_amd_batch_polish_launches() == n_pol + 1
    A.update(q=args[4][sel], rows=sel)  # updates of vectors launch neither
    A.warm_start(x=np.zeros((3, 100)), rows=sel)
    assert product_lib.osqp_amd_batch_cert_launches() == n_cert + 2 and product_lib.osqp_amd_batch_polish_launches() == n_pol + 1
    A.close()


def test_certificates_and_polish_status_are_per_instance(product_lib, oracle_lib):
    """The MPC family with infeasible instances (batch_cert_cases.mpc: solvable, primal infeasible, dual infeasible in turn),
    polish on.  Instances 4 (primal infeasible) and 3 (solvable) swap their bounds on row 60, so 4 becomes solvable and 3
    primal infeasible; after `solve(rows=[4, 3])` their rows of certificates() and polish_status() are those of the sub-batch
    twin, every other row is what it was before the call.  Then polish off and the same selection again: the selected
    instances' polish status becomes 0, the others keep theirs."""
    args = _stacked(oracle_lib, "cert")
    opts = dict(OPTS, polish=True)
    sel = np.array([4, 3])
    rest = np.array([i for i in range(8) if i not in sel])
    A, S, R = _handles(product_lib, args, sel, rest, opts)
    first = A.solve()
    S.solve(); R.solve()
    assert [int(v) for v in first[2][:, 1]] == [1, -3, -4, 1, -3, -4, 1, -3]
    cert0, pol0 = A.certificates(), A.polish_status()
    assert np.all(np.isfinite(cert0[0][4])) and np.all(np.isnan(cert0[0][3])) and pol0[3] != 0 and pol0[4] == 0
    assert _same([c[sel] for c in cert0], S.certificates()) and _same([c[rest] for c in cert0], R.certificates())
    l, u = args[5][sel].copy(), args[6][sel].copy()
    l[:, 60], u[:, 60] = l[::-1, 60].copy(), u[::-1, 60].copy()
    A.update(l=l, u=u, rows=sel); S.update(l=l, u=u)
    got, want = A.solve(rows=sel), S.solve()
    _assert_same(got, want, "swapped bounds")
    assert [int(v) for v in got[2][:, 1]] == [1, -3]
    cert1, pol1 = A.certificates(), A.polish_status()
    assert _same([c[sel] for c in cert1], S.certificates()) and np.array_equal(pol1[sel], S.polish_status())
    assert np.all(np.isnan(cert1[0][4])) and np.all(np.isfinite(cert1[0][3])) and pol1[4] != 0 and pol1[3] == 0
    assert _same([c[rest] for c in cert1], [c[rest] for c in cert0]) and np.array_equal(pol1[rest], pol0[rest])
    assert _same([c[rest] for c in cert1], R.certificates()) and np.array_equal(pol1[rest], R.polish_status())
    A.update_polish(0); S.update_polish(0)
    _assert_same(A.solve(rows=sel), S.solve(), "polish off")
    pol2 = A.polish_status()
    assert np.all(pol2[sel] == 0) and np.array_equal(pol2[rest], pol0[rest]) and np.any(pol0[rest] != 0)
    assert _same([c[sel] for c in A.certificates()], S.certificates())
    A.close(); S.close(); R.close()


def test_retry_the_unsolved(product_lib, oracle_lib):
    """max_iter at the median of the oracle's cold iteration counts (rounded down to a multiple of check_termination): some
    instances are Solved, the others stop at the limit.  `update_settings(max_iter=4000)` and a solve of the unsolved ones
    alone gives what the sub-batch of those instances gives through the same two solves."""
    probs = ref.mpc_instances(oracle_lib, 0, 8, 2)
    args = _stacked(oracle_lib, "mpc")
    iters = [r.info.iter for r in ref.cold_oracle(oracle_lib, probs, **OPTS)]
    limit = int(np.median(iters)) // 25 * 25
    print("oracle iterations", iters, "max_iter", limit)
    assert max(iters) < 4000  # every instance can be solved within the limit of the retry
    opts = dict(OPTS, max_iter=limit)
    A = batch.ResidentBatch(product_lib, *args, **opts)
    x, y, info = A.solve()
    status = info[:, 1].astype(int)
    print("status", status, "iterations", info[:, 0])
    assert np.any(status == 1) and np.any(status != 1)
    unsolved = np.flatnonzero(status != 1)
    S = batch.ResidentBatch(product_lib, *_rows(args, unsolved), **opts)
    _assert_same(_take((x, y, info), unsolved), S.solve(), "at the limit")
    A.update_settings(max_iter=4000); S.update_settings(max_iter=4000)
    got = A.solve(rows=status != 1)  # the mask form
    _assert_same(got, S.solve(), "retried")
    assert np.all(got[2][:, 1] == 1)
    after = A.solve()
    assert np.all(after[2][:, 1] == 1)
    _assert_same(_take(after, unsolved), S.solve(), "whole solve after the retry")
    A.close(); S.close()


def test_adjoint_needs_every_instance_current(product_lib, oracle_lib):
    args = _stacked(oracle_lib, "quad64")
    count, n, m = args[4].shape[0], args[4].shape[1], args[5].shape[1]
    sel, rest = _selection(count)
    rng = np.random.default_rng(5)
    gx, gy = rng.standard_normal((count, n)), rng.standard_normal((count, m))
    A, S, R = _handles(product_lib, args, sel, rest, OPTS)
    with pytest.raises(batch.OSQPError, match="instance 0 .*resolve"):
        A.adjoint(dx=gx, dy=gy)
    A.solve(rows=sel); S.solve()
    with pytest.raises(batch.OSQPError, match="instance 1 .*resolve"):  # 0 and 2 are current now, 1 has never been solved
        A.adjoint(dx=gx, dy=gy)
    A.solve(); S.solve(); R.solve()
    q2 = args[4][sel] * 1.02
    A.update(q=q2, rows=sel); S.update(q=q2)
    with pytest.raises(batch.OSQPError, match="instance 0 .*resolve"):
        A.adjoint(dx=gx, dy=gy)
    A.solve(rows=sel[:1])
    with pytest.raises(batch.OSQPError, match="instance 0 .*resolve"):  # instance count - 1 is current again, 0 and 2 are not
        A.adjoint(dx=gx, dy=gy)
    A.solve(rows=sel[1:])
    S.solve()
    g = A.adjoint(dx=gx, dy=gy)
    gs, gr = S.adjoint(dx=gx[sel], dy=gy[sel]), R.adjoint(dx=gx[rest], dy=gy[rest])
    assert sorted(g) == sorted(gs) == sorted(gr) and np.all(g["status"] == 1)
    for key in g:
        assert np.array_equal(g[key][sel], gs[key], equal_nan=True), key
        assert np.array_equal(g[key][rest], gr[key], equal_nan=True), key
    A.warm_start(x=np.zeros((1, n)), rows=[3])
    with pytest.raises(batch.OSQPError, match="instance 3 .*resolve"):
        A.adjoint(dx=gx, dy=gy)
    A.close(); S.close(); R.close()


def test_device_form_equals_host_form(product_lib, oracle_lib):
    """Compact device arrays in and out (DeviceArray; a torch tensor goes the same way through data_ptr())."""
    args = _stacked(oracle_lib, "mpc")
    sel, rest = _selection(8)
    k, n, m = len(sel), 100, 200
    A, S, R = _handles(product_lib, args, sel, rest, OPTS)
    first = A.solve(); S.solve(); R.solve()
    q2, l2 = args[4][sel] * 0.97, args[5][sel] - 0.01
    dev = lambda a: batch.DeviceArray(product_lib, a.shape[0], a.shape[1]).upload(a)
    A.update(q=dev(q2), l=dev(l2), rows=sel); S.update(q=q2, l=l2)
    out = A.alloc(k)
    assert [o.shape for o in out] == [(k, n), (k, m), (k, 6)]
    assert A.solve(out=out, rows=sel) is out
    want = S.solve()
    _assert_same([o.numpy() for o in out], want, "device out")
    x0, y0 = first[0][sel] * 0.8, first[1][sel] * 0.8
    A.warm_start(x=dev(x0), y=dev(y0), rows=sel); S.warm_start(x=x0, y=y0)
    A.solve(out=out, rows=sel)
    _assert_same([o.numpy() for o in out], S.solve(), "device warm start")
    whole = A.solve()
    _assert_same(_take(whole, sel), S.solve(), "whole, selected")
    _assert_same(_take(whole, rest), R.solve(), "whole, others")
    with pytest.raises(ValueError, match=r"out\[0\]"):
        A.solve(out=A.alloc(), rows=sel)  # [count x .] arrays for a selection of k
    A.close(); S.close(); R.close()


def test_refusals_leave_the_handle_unchanged(product_lib, oracle_lib):
    """Bad selections and bad shapes raise -- in the Python helper and, called directly, in the library (return 1 and a
    message) -- and so does l > stored u on a selected row; the whole solve that follows still equals the twin's."""
    lib = product_lib
    args = _stacked(oracle_lib, "mpc")
    count, n, m = 8, 100, 200
    A = batch.ResidentBatch(lib, *args, **OPTS)
    T = batch.ResidentBatch(lib, *args, **OPTS)
    first = A.solve(); T.solve()
    q3 = np.zeros((3, n))
    for bad in ([1, 4, 1], [0, -1, 2], [0, count, 2], [], np.zeros(count, dtype=bool), list(range(count)) + [0]):
        with pytest.raises(ValueError, match="rows"):
            A.update(q=np.zeros((len(bad), n)), rows=bad)
        with pytest.raises(ValueError, match="rows"):
            A.warm_start(x=np.zeros((len(bad), n)), rows=bad)
        with pytest.raises(ValueError, match="rows"):
            A.solve(rows=bad)
    with pytest.raises(ValueError, match="q"):  # a [count x n] array with a selection of three
        A.update(q=args[4], rows=[5, 0, 3])
    with pytest.raises(ValueError, match="x"):
        A.warm_start(x=first[0], rows=[5, 0, 3])
    with pytest.raises(ValueError, match="u"):
        A.update(l=args[5][:3], u=args[6], rows=[5, 0, 3])
    # the library's own checks, past the helper
    x, y, info, ax = np.zeros((count + 1, n)), np.zeros((count + 1, m)), np.zeros((count + 1, 6)), np.ones((count + 1, A.nnzA))
    vec = lambda a: a.ctypes.data
    for rows, k, word in (([1, 4, 1], 3, "instance 1 is repeated"), ([0, -1, 2], 3, "out of range"), ([0, count, 2], 3, "out of range"),
                          ([0], 0, "1 <= k <= count"), (list(range(count)) + [0], count + 1, "1 <= k <= count")):
        r = np.array(rows, dtype=np.int64)
        rp = _iptr(r)
        calls = (lib.osqp_amd_batch_update_lin_cost_rows(A.handle, rp, k, vec(x), 0),
                 lib.osqp_amd_batch_update_bounds_rows(A.handle, rp, k, vec(y), vec(y), 0),
                 lib.osqp_amd_batch_update_matrices_rows(A.handle, rp, k, None, vec(ax), 0),
                 lib.osqp_amd_batch_warm_start_rows(A.handle, rp, k, vec(x), None, 0),
                 lib.osqp_amd_batch_resolve_rows(A.handle, rp, k, vec(x), vec(y), vec(info), 0))
        assert calls == (1, 1, 1, 1, 1), (rows, k, calls)
        assert word in lib.osqp_amd_last_error().decode(), (word, lib.osqp_amd_last_error().decode())
    mpc_handle = batch.MpcBatch(lib, 4, seed=2, **OPTS)  # the other family's handle
    one = np.zeros(1, dtype=np.int64)
    assert lib.osqp_amd_batch_resolve_rows(mpc_handle.handle, _iptr(one), 1, vec(x), vec(y), vec(info), 0) == 1
    mpc_handle.close()
    # l above the STORED u of one selected row, u not given: refused on the device, nothing changes
    l_bad = args[5][[5, 0, 3]].copy()
    l_bad[1, 7] = args[6][0, 7] + 1.0
    with pytest.raises(batch.OSQPError, match="lower bound"):
        A.update(l=l_bad, rows=[5, 0, 3])
    u_bad = args[6][[2]].copy()
    u_bad[0, 150] = args[5][2, 150] - 1.0
    with pytest.raises(batch.OSQPError, match="lower bound"):
        A.update(u=u_bad, rows=[2])
    A.adjoint(dx=np.ones((count, n)))  # the refused calls made nothing stale
    _assert_same(A.solve(), T.solve(), "after the refusals")
    _assert_same(A.solve(rows=[6, 1]), _take(T.solve(), [6, 1]), "a subset solve after them")
    A.close(); T.close()
