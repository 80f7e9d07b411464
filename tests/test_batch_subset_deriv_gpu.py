"""The reading calls of the resident batch for a selection, on the GPU: `adjoint(rows=)`, `jvp(rows=)`, `certificates(rows=)`,
`polish_status(rows=)` of batch.ResidentBatch (osqp_amd_batch_adjoint_rows, _jvp_rows, _certificates_rows,
_polish_status_rows) and `BatchQPLayer(..., rows=)`.

The yardstick is that of tests/test_batch_subset_gpu.py: bit-equality with the SAME library, never a tolerance.  Row j of a
call with `rows=sel` must be row sel[j] of the whole-batch call on the same handle, and -- with stale neighbours, where the
whole-batch call refuses -- the row of the whole-batch call on a handle S built from the selected instances alone."""
import numpy as np
import pytest
import scipy.sparse as sp

from osqp_jl_amd import batch
import batch_adjoint_ref as adj
import batch_jvp_ref as jv
import batch_resident_ref as ref
from batch_resident_ref import OPTS
from test_batch_jvp_gpu import _View
from test_batch_subset_gpu import _assert_same, _handles, _stacked, _take

pytestmark = pytest.mark.gpu

NDIR = 3
FAMILIES = ["tiny", "wide300", "tri128", "mpc"]


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _problems(oracle_lib, family):
    probs = adj.problems(oracle_lib, family)
    return probs[:8] if family == "mpc" else probs


def _assert_adjoint_rows(got, whole, sel, tag):
    assert sorted(got) == sorted(whole), (tag, sorted(got), sorted(whole))
    for key in got:
        assert got[key].shape == whole[key][sel].shape and got[key].dtype == whole[key].dtype, (tag, key, got[key].shape)
        assert _same(got[key], whole[key][sel]), (tag, key)


def _assert_jvp_rows(got, whole, sel, tag):
    assert sorted(got) == sorted(whole), (tag, sorted(got), sorted(whole))
    for key in got:
        want = whole[key][:, sel] if key in ("x", "y") and whole[key].ndim == 3 else whole[key][sel]
        assert got[key].shape == want.shape and got[key].dtype == want.dtype, (tag, key, got[key].shape, want.shape)
        assert _same(got[key], want), (tag, key)


@pytest.mark.parametrize("family", FAMILIES)
def test_selection_equals_the_rows_of_the_whole_call(product_lib, oracle_lib, family):
    lib = product_lib
    probs = _problems(oracle_lib, family)
    rb = batch.ResidentBatch(lib, *ref.stack(probs), **dict(OPTS, polish=True))
    count = rb.count
    rb.solve()
    gx, gy = adj.incoming(family, count, rb.n, rb.m)
    d = jv.tangents(family, NDIR, probs)
    g, t = rb.adjoint(dx=gx, dy=gy), rb.jvp(**d)
    t_part = rb.jvp(q=d["q"], Ax=d["Ax"])
    t_one = rb.jvp(**{k: v[1] for k, v in d.items()})
    assert np.any(g["status"] == 1) and np.any(g["q"] != 0.0) and np.any(t["x"] != 0.0)
    main = np.array([2, 0]) if family == "tri128" else np.array([count - 1, 0, 2])
    n_adj, n_jvp = lib.osqp_amd_batch_adjoint_launches(), lib.osqp_amd_batch_jvp_launches()
    calls = 0
    for sel in (main, main[:1], main[-1:], np.arange(count)):
        tag = f"{family}/{sel.tolist()}"
        _assert_adjoint_rows(rb.adjoint(dx=gx[sel], dy=gy[sel], rows=sel), g, sel, tag)
        _assert_jvp_rows(rb.jvp(**{k: v[:, sel] for k, v in d.items()}, rows=sel), t, sel, tag)
        # a want subset, a tangent subset, one direction without the leading axis
        part = rb.adjoint(dx=gx[sel], dy=gy[sel], want=("l", "Ax"), rows=sel)
        assert sorted(part) == ["Ax", "act", "l", "status"]
        _assert_adjoint_rows(part, {k: g[k] for k in part}, sel, tag + " want")
        _assert_jvp_rows(rb.jvp(q=d["q"][:, sel], Ax=d["Ax"][:, sel], rows=sel), t_part, sel, tag + " tangent subset")
        _assert_jvp_rows(rb.jvp(**{k: v[1, sel] for k, v in d.items()}, rows=sel), t_one, sel, tag + " one direction")
        calls += 1
    assert lib.osqp_amd_batch_adjoint_launches() == n_adj + 2 * calls and lib.osqp_amd_batch_jvp_launches() == n_jvp + 3 * calls
    mask = np.zeros(count, dtype=bool)
    mask[main] = True
    _assert_adjoint_rows(rb.adjoint(dx=gx[mask], dy=gy[mask], rows=mask), g, np.flatnonzero(mask), family + " mask")
    rb.close()


def test_stale_neighbours(product_lib, oracle_lib):
    """The capability itself: every instance of A gets a new q, only `sel` is re-solved -- and differentiated, with the
    bits of the sub-batch twin S.  The derivative calls write nothing on the handle: the next whole solve of A is the next
    solve of S on the selected rows and of R on the others."""
    lib = product_lib
    family = "tiny"
    probs = _problems(oracle_lib, family)
    args = ref.stack(probs)
    count = len(probs)
    sel = np.array([count - 1, 0, 2])
    rest = np.array([i for i in range(count) if i not in sel])
    A, S, R = _handles(lib, args, sel, rest, dict(OPTS, polish=True))
    A.solve(); S.solve(); R.solve()
    q2 = np.asarray(args[4]) * 1.05 + 0.01
    A.update(q=q2); S.update(q=q2[sel]); R.update(q=q2[rest])
    _assert_same(A.solve(rows=sel), S.solve(), "subset solve")
    gx, gy = adj.incoming(family, count, A.n, A.m)
    d = jv.tangents(family, NDIR, probs)
    g = A.adjoint(dx=gx[sel], dy=gy[sel], rows=sel)
    t = A.jvp(**{k: v[:, sel] for k, v in d.items()}, rows=sel)
    gs, ts = S.adjoint(dx=gx[sel], dy=gy[sel]), S.jvp(**{k: v[:, sel] for k, v in d.items()})
    assert sorted(g) == sorted(gs) and sorted(t) == sorted(ts) and np.all(g["status"] == 1)
    for key in g:
        assert g[key].shape == gs[key].shape and _same(g[key], gs[key]), key
    for key in t:
        assert t[key].shape == ts[key].shape and _same(t[key], ts[key]), key
    n_adj, n_jvp = lib.osqp_amd_batch_adjoint_launches(), lib.osqp_amd_batch_jvp_launches()
    with pytest.raises(batch.OSQPError, match="instance 1 .*resolve"):  # the whole-batch rule is what it was
        A.adjoint(dx=gx, dy=gy)
    with pytest.raises(batch.OSQPError, match="instance 1 .*resolve"):
        A.jvp(**d)
    bad = np.array([count - 1, 3, 1])  # the first stale one in the order of rows
    with pytest.raises(batch.OSQPError, match="instance 3 .*resolve"):
        A.adjoint(dx=gx[bad], dy=gy[bad], rows=bad)
    with pytest.raises(batch.OSQPError, match="instance 3 .*resolve"):
        A.jvp(**{k: v[:, bad] for k, v in d.items()}, rows=bad)
    assert lib.osqp_amd_batch_adjoint_launches() == n_adj and lib.osqp_amd_batch_jvp_launches() == n_jvp
    whole = A.solve()
    _assert_same(_take(whole, sel), S.solve(), "next whole solve, selected")
    _assert_same(_take(whole, rest), R.solve(), "next whole solve, others")
    A.close(); S.close(); R.close()


def test_instances_without_a_solution(product_lib, oracle_lib):
    """The batch of test_instances_without_a_solution_get_status_zero_and_zero_rows: 16 MPC instances, max_iter = 100,
    instances 1, 5, 9 primal infeasible.  Status 0 and zero rows land at the POSITIONS of the unsolved instances."""
    probs = ref.mpc_instances(oracle_lib, 0, 16, 2)
    args = ref.stack(probs)
    l2, u2 = args[5].copy(), args[6].copy()
    for i in (1, 5, 9):
        l2[i, 60] = u2[i, 60] = 1000.0
    rb = batch.ResidentBatch(product_lib, *args, **dict(OPTS, max_iter=100, polish=True))
    rb.update(l=l2, u=u2)
    x, y, info = rb.solve()
    status = info[:, 1].astype(int)
    solved = [int(i) for i in np.flatnonzero(status == 1) if i != 15][:2]
    assert len(solved) == 2
    sel = np.array([5, solved[1], 15, 1, solved[0], 9])
    print("status", status, "selection", sel)
    assert np.sum(status[sel] == -3) >= 2 and np.sum(status[sel] == 1) >= 2
    moved = [(P, q, A, l2[i], u2[i]) for i, (P, q, A, l, u) in enumerate(probs)]
    gx, gy = adj.incoming("mpc", rb.count, rb.n, rb.m)
    d = jv.tangents("mpc", NDIR, moved)
    g, t = rb.adjoint(dx=gx, dy=gy), rb.jvp(**d)
    gs = rb.adjoint(dx=gx[sel], dy=gy[sel], rows=sel)
    ts = rb.jvp(**{k: v[:, sel] for k, v in d.items()}, rows=sel)
    rb.close()
    assert np.array_equal(gs["status"] != 0, status[sel] == 1) and np.array_equal(ts["status"] != 0, status[sel] == 1)
    for pos in np.flatnonzero(status[sel] != 1):
        assert gs["status"][pos] == 0 and ts["status"][pos] == 0 and not np.any(gs["act"][pos]) and not np.any(ts["act"][pos])
        assert all(not np.any(gs[k][pos]) for k in adj.GRADS), pos
        assert not np.any(ts["x"][:, pos]) and not np.any(ts["y"][:, pos]), pos  # in every direction
    solved_pos = np.flatnonzero(status[sel] == 1)
    assert np.any(gs["q"][solved_pos] != 0.0) and np.any(ts["x"][:, solved_pos] != 0.0)
    _assert_adjoint_rows(gs, g, sel, "adjoint")
    _assert_jvp_rows(ts, t, sel, "jvp")


def test_a_batch_without_constraints(product_lib, oracle_lib):
    """m = 0, n = 5, count 4: "y" / "act" are left out and there is no primal certificate."""
    rng = np.random.default_rng(50)
    n, count = 5, 4
    pat = sp.triu(sp.csc_matrix(np.ones((n, n))), format="csc"); pat.sort_indices()
    Px = []
    for _ in range(count):
        B = rng.standard_normal((n, n))
        U = sp.triu(sp.csc_matrix(B @ B.T + n * np.eye(n)), format="csc"); U.sort_indices()
        Px.append(U.data.copy())
    q = rng.standard_normal((count, n))
    rb = batch.ResidentBatch(product_lib, pat, sp.csc_matrix((0, n)), np.array(Px), np.zeros((count, 0)), q, np.zeros((count, 0)),
                             np.zeros((count, 0)), **OPTS)
    rb.solve()
    gx = rng.standard_normal((count, n))
    d = dict(q=rng.standard_normal((2, count, n)), Px=rng.standard_normal((2, count, pat.nnz)))
    g, t = rb.adjoint(dx=gx), rb.jvp(**d)
    sel = np.array([3, 1])
    gs = rb.adjoint(dx=gx[sel], rows=sel)
    ts = rb.jvp(**{k: v[:, sel] for k, v in d.items()}, l=np.zeros((2, 2, 0)), Ax=np.zeros((2, 2, 0)), rows=sel)
    assert sorted(gs) == ["Px", "q", "status"] and sorted(ts) == ["status", "x"] and np.all(gs["status"] == 1)
    _assert_adjoint_rows(gs, g, sel, "m = 0 adjoint")
    _assert_jvp_rows(ts, t, sel, "m = 0 jvp")
    p, dual = rb.certificates(rows=sel)
    assert p is None and _same(dual, rb.certificates()[1][sel]) and dual.shape == (2, n)
    assert np.array_equal(rb.polish_status(rows=sel), rb.polish_status()[sel])
    rb.close()


def test_certificates_and_polish_status_of_a_selection(product_lib, oracle_lib):
    """The handle of test_certificates_and_polish_status_are_per_instance (solvable, primal infeasible, dual infeasible in
    turn; polish on): before the first solve, after a whole solve, and after a subset solve without polish."""
    args = _stacked(oracle_lib, "cert")
    rb = batch.ResidentBatch(product_lib, *args, **dict(OPTS, polish=True))
    sels = (np.array([7, 0, 5, 4]), np.array([3]), np.arange(8), np.array([False, True, True, False, False, False, True, False]))

    def check(tag):
        cert, pol = rb.certificates(), rb.polish_status()
        for sel in sels:
            idx = np.flatnonzero(sel) if sel.dtype == bool else sel
            got, gpol = rb.certificates(rows=sel), rb.polish_status(rows=sel)
            assert got[0].shape == (len(idx), rb.m) and got[1].shape == (len(idx), rb.n) and gpol.shape == (len(idx),), tag
            assert _same(got[0], cert[0][idx]) and _same(got[1], cert[1][idx]), (tag, idx)
            assert gpol.dtype == pol.dtype and np.array_equal(gpol, pol[idx]), (tag, idx)
        return cert, pol

    cert, pol = check("before the first solve")
    assert np.all(np.isnan(cert[0])) and np.all(np.isnan(cert[1])) and not np.any(pol)
    info = rb.solve()[2]
    assert [int(v) for v in info[:, 1]] == [1, -3, -4, 1, -3, -4, 1, -3]
    cert, pol = check("after a whole solve")
    assert np.all(np.isfinite(cert[0][4])) and np.all(np.isfinite(cert[1][5])) and np.all(np.isnan(cert[0][0])) and np.any(pol != 0)
    sw = np.array([4, 3])
    l, u = args[5][sw].copy(), args[6][sw].copy()
    l[:, 60], u[:, 60] = l[::-1, 60].copy(), u[::-1, 60].copy()
    rb.update(l=l, u=u, rows=sw)
    rb.update_polish(0)
    assert [int(v) for v in rb.solve(rows=sw)[2][:, 1]] == [1, -3]
    cert, pol = check("after a subset solve without polish")
    assert np.all(np.isnan(cert[0][4])) and np.all(np.isfinite(cert[0][3])) and pol[3] == 0 and pol[4] == 0 and np.any(pol != 0)
    # the device form
    k = 4
    dp, dd, ds = (batch.DeviceArray(product_lib, k, c) for c in (rb.m, rb.n, 1))
    out = rb.certificates(out=(dp, dd), rows=sels[0])
    assert out[0] is dp and out[1] is dd and _same(dp.numpy(), cert[0][sels[0]]) and _same(dd.numpy(), cert[1][sels[0]])
    assert rb.polish_status(out=ds, rows=sels[0]) is ds and np.array_equal(ds.numpy().ravel(), pol[sels[0]])
    only = rb.certificates(out=(None, dd), rows=sels[0][::-1])
    assert only[1] is dd and _same(dd.numpy(), cert[1][sels[0][::-1]])
    with pytest.raises(ValueError, match="no certificate"):
        rb.certificates(out=(None, None), rows=sels[0])
    for a in (dp, dd, ds):
        a.free()
    rb.close()


def test_device_form_equals_host_form(product_lib, oracle_lib):
    family = "tiny"
    probs = _problems(oracle_lib, family)
    rb = batch.ResidentBatch(product_lib, *ref.stack(probs), **dict(OPTS, polish=True))
    rb.solve()
    count = rb.count
    sel = np.array([count - 1, 0, 2])
    k = len(sel)
    gx, gy = adj.incoming(family, count, rb.n, rb.m)
    d = {name: np.ascontiguousarray(v[:, sel]) for name, v in jv.tangents(family, NDIR, probs).items()}
    keep = []

    def dev(rows, cols):
        keep.append(batch.DeviceArray(product_lib, rows, cols))
        return keep[-1]

    host_g = rb.adjoint(dx=gx[sel], dy=gy[sel], rows=sel)
    cols = dict(q=rb.n, l=rb.m, u=rb.m, Px=rb.nnzP, Ax=rb.nnzA, act=rb.m, status=1)
    out = {name: dev(k, c) for name, c in cols.items()}
    dgx, dgy = dev(k, rb.n).upload(gx[sel]), dev(k, rb.m).upload(gy[sel])
    assert rb.adjoint(dx=dgx, dy=dgy, out=out, rows=sel) is out
    for name in cols:
        assert _same(out[name].numpy().reshape(host_g[name].shape), host_g[name]), name
    host_t = rb.jvp(**d, rows=sel)
    din = {name: _View(dev(NDIR * k, v.shape[2]).upload(v.reshape(NDIR * k, -1)), NDIR) for name, v in d.items()}
    tout = dict(x=_View(dev(NDIR * k, rb.n), NDIR), y=_View(dev(NDIR * k, rb.m), NDIR), act=dev(k, rb.m), status=dev(k, 1))
    assert rb.jvp(**din, out=tout, rows=sel) is tout
    for name in tout:
        assert _same(tout[name].numpy().reshape(host_t[name].shape), host_t[name]), name
    # refusals, before the library is called: [count x .] arrays with a selection of k, host and device arrays mixed
    n_adj, n_jvp = product_lib.osqp_amd_batch_adjoint_launches(), product_lib.osqp_amd_batch_jvp_launches()
    with pytest.raises(ValueError, match="dx"):
        rb.adjoint(dx=dev(count, rb.n), dy=dgy, out=out, rows=sel)
    with pytest.raises(ValueError, match=r"out\['q'\]"):
        rb.adjoint(dx=dgx, dy=dgy, out=dict(out, q=dev(count, rb.n)), rows=sel)
    with pytest.raises(ValueError, match="both"):
        rb.adjoint(dx=dgx, dy=gy[sel], out=out, rows=sel)
    with pytest.raises(ValueError, match="q"):
        rb.jvp(q=_View(dev(NDIR * count, rb.n), NDIR), out=tout, rows=sel)
    with pytest.raises(ValueError, match="all be host arrays or all device arrays"):
        rb.jvp(q=din["q"], l=d["l"], out=tout, rows=sel)
    assert product_lib.osqp_amd_batch_adjoint_launches() == n_adj and product_lib.osqp_amd_batch_jvp_launches() == n_jvp
    for a in keep:
        a.free()
    rb.close()


def test_torch_layer_with_a_selection(product_lib, oracle_lib):
    import torch
    from torch.autograd import forward_ad

    from osqp_jl_amd.qp_layer import BatchQPLayer

    family = "ineq"
    probs = adj.problems(oracle_lib, family)
    args = ref.stack(probs)
    rb = batch.ResidentBatch(product_lib, *args, **dict(OPTS, polish=True))
    layer = BatchQPLayer(rb)
    count = rb.count
    sel = [count - 1, 0, 2]
    rest = [i for i in range(count) if i not in sel]
    dev = torch.device("cuda:0")
    gx, gy = adj.incoming(family, count, rb.n, rb.m)
    wx, wy = torch.tensor(gx[sel], device=dev), torch.tensor(gy[sel], device=dev)
    q_t = torch.tensor(args[4], device=dev, requires_grad=True)
    x, y = layer(q=q_t[sel], rows=sel)
    assert tuple(x.shape) == (3, rb.n) and tuple(y.shape) == (3, rb.m) and tuple(layer.info.shape) == (3, 6)
    assert np.all(layer.info.cpu().numpy()[:, 1] == 1)
    ((wx * x).sum() + (wy * y).sum()).backward()
    want = rb.adjoint(dx=gx[sel], dy=gy[sel], want=("q",), rows=sel)["q"]
    grad = q_t.grad.cpu().numpy()
    assert _same(grad[sel], want) and np.any(want != 0.0) and not np.any(grad[rest])
    # forward mode
    d = {k: v[0] for k, v in jv.tangents(family, 1, probs).items()}
    q0 = torch.tensor(args[4][sel], device=dev)
    with forward_ad.dual_level():
        x, y = layer(q=forward_ad.make_dual(q0, torch.tensor(d["q"][sel], device=dev)), rows=np.array(sel))
        tx, ty = forward_ad.unpack_dual(x).tangent, forward_ad.unpack_dual(y).tangent
        t = rb.jvp(q=d["q"][sel], rows=sel)
        assert tx is not None and ty is not None and np.any(t["x"] != 0.0)
        assert _same(tx.cpu().numpy(), t["x"]) and _same(ty.cpu().numpy(), t["y"])
    # the stamps are per instance
    qa = torch.tensor(args[4], device=dev, requires_grad=True)
    x1, _ = layer(q=qa[[5, 0]], rows=[5, 0])
    x2, _ = layer(q=qa[[2, 3]], rows=[2, 3])
    x1.sum().backward()
    x2.sum().backward()  # disjoint selections: both run
    assert np.all(np.any(qa.grad.cpu().numpy()[[5, 0, 2, 3]] != 0.0, axis=1)) and not np.any(qa.grad.cpu().numpy()[[1, 4]])
    x1, _ = layer(q=qa[[5, 0]], rows=[5, 0])
    x3, _ = layer(q=qa[[0, 1]], rows=[0, 1])
    with pytest.raises(RuntimeError, match="solved again"):
        x1.sum().backward()
    x3.sum().backward()
    x1, _ = layer(q=qa[[5, 0]], rows=[5, 0])
    xw, _ = layer(q=qa)
    with pytest.raises(RuntimeError, match="solved again"):
        x1.sum().backward()
    xw.sum().backward()
    rb.close()
