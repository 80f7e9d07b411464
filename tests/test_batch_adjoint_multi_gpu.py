"""Several cotangents per adjoint launch on the GPU (osqp_amd_batch_adjoint_multi, _multi_rows: the cotangent loop of
k_batch_adjoint; the leading axis of `ResidentBatch.adjoint`; `ResidentBatch.jacobian`; `torch.func.vmap` / `jacrev` through
`qp_layer.BatchQPLayer`).

Two yardsticks.  Bit-equality with the SAME library: cotangent c of an ncot call against the one-cotangent call with that
pair, a selection against the rows of the whole call, chunks against one launch, the device form against the host form, the
torch routes against `ResidentBatch`.  And `batch_adjoint_ref.exact` / `batch_jvp_ref.exact` on the device's own x, y, act,
with the bounds of tests/test_batch_adjoint_gpu.py and tests/test_batch_jvp_gpu.py: 1000 x MEASURED_C[family] of the two host
files, over at least MIN_NONDEGENERATE[family] instances.

Shapes: tiny (n 5, m 3, 8 instances: the smallest), wide300 (m 300 > the 256 threads: the strided row loops), tri128 (n 128:
the register-vector limit of the solves), mpc (the target family; all 64 instances of the reference module, because the
comparison with `exact` must cover 20 non-degenerate ones and the first 16 hold fewer).

FIGURES of a run on the MI355X (the tests print them), worst relative figure over the three cotangents (bound): tiny 1.1e-15
(1.0e-12), wide300 3.2e-12 (3.3e-9), tri128 1.3e-14 (8.7e-12), mpc 1.0e-14 on 23 non-degenerate instances (4.3e-12); m = 0
1.1e-16; `jacobian` reverse / forward: tiny 6.4e-16 / 6.4e-16 (1.0e-12 / 1.3e-12), ineq 3.4e-14 / 2.1e-14 (8.9e-12 / 1.3e-11)."""
import numpy as np
import pytest
import scipy.sparse as sp

from osqp_jl_amd import batch
import batch_adjoint_ref as adj
import batch_jvp_ref as jv
import batch_resident_ref as ref
from batch_resident_ref import OPTS
from test_batch_adjoint_host import MEASURED_C
from test_batch_jvp_gpu import _View
from test_batch_jvp_host import MEASURED_C as JVP_MEASURED_C

pytestmark = pytest.mark.gpu

NCOT = 3
FAMILIES = ["tiny", "wide300", "tri128", "mpc"]
_runs = {}


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _cotangents(family, ncot, count, n, m):
    rng = np.random.default_rng(7000 + sum(map(ord, family)))
    return rng.standard_normal((ncot, count, n)), rng.standard_normal((ncot, count, m))


def _run(product_lib, oracle_lib, family):
    """One handle per family, once per session: resolve (polish = 0 after a polished one, as test_batch_adjoint_gpu.py), one
    call with NCOT cotangents, NCOT calls with one, and the variants the independence test compares."""
    if family not in _runs:
        lib = product_lib
        probs = adj.problems(oracle_lib, family)
        rb = batch.ResidentBatch(lib, *ref.stack(probs), **dict(OPTS, polish=True))
        rb.solve()
        rb.update_polish(0)
        x, y, info = rb.solve()
        GX, GY = _cotangents(family, NCOT, rb.count, rb.n, rb.m)
        before = lib.osqp_amd_batch_adjoint_launches()
        multi = rb.adjoint(dx=GX, dy=GY)
        launches = lib.osqp_amd_batch_adjoint_launches() - before
        single = [rb.adjoint(dx=GX[c], dy=GY[c]) for c in range(NCOT)]
        lead = rb.adjoint(dx=GX[1:2], dy=GY[1:2])  # one cotangent with the leading axis
        no_dy, zero_dy = rb.adjoint(dx=GX), rb.adjoint(dx=GX, dy=np.zeros_like(GY))
        rb.close()
        _runs[family] = dict(probs=probs, x=x, y=y, info=info, GX=GX, GY=GY, multi=multi, single=single, lead=lead, no_dy=no_dy,
                             zero_dy=zero_dy, launches=launches)
    return _runs[family]


@pytest.mark.parametrize("family", FAMILIES)
def test_cotangents_are_independent(product_lib, oracle_lib, family):
    """Every output of cotangent c of one launch has the bits of the one-cotangent call with that pair -- which a missing
    barrier between the cotangents, a clobbered x or anything carried over would break; the ncot = 1 call with a leading
    axis has the bits of the call without; a missing dy is a dy of zeros; one launch, whatever ncot."""
    r = _run(product_lib, oracle_lib, family)
    multi, single = r["multi"], r["single"]
    count = len(r["probs"])
    assert r["launches"] == 1
    assert np.any(multi["status"] == 1) and multi["status"].shape == (count,) and multi["act"].shape == r["single"][0]["act"].shape
    for c in range(NCOT):
        assert sorted(single[c]) == sorted(multi)
        for k in adj.GRADS:
            assert multi[k].shape == (NCOT,) + single[c][k].shape and np.any(single[c][k] != 0.0), (k, multi[k].shape)
            assert _same(multi[k][c], single[c][k]), (family, c, k)
        assert _same(multi["act"], single[c]["act"]) and _same(multi["status"], single[c]["status"])
    for k in adj.GRADS:
        assert r["lead"][k].shape == (1,) + single[1][k].shape and _same(r["lead"][k][0], single[1][k]), k
        assert not _same(multi[k][0], multi[k][1])  # the cotangents differ, so must the results
    assert sorted(r["no_dy"]) == sorted(r["zero_dy"]) and all(_same(r["no_dy"][k], r["zero_dy"][k]) for k in r["no_dy"])


@pytest.mark.parametrize("family", FAMILIES)
def test_every_cotangent_agrees_with_the_exact_adjoint(product_lib, oracle_lib, family):
    r = _run(product_lib, oracle_lib, family)
    g, info = r["multi"], r["info"]
    solved = np.flatnonzero(info[:, 1] == 1)
    worst, used = [0.0] * NCOT, []
    for i in solved:
        P, q, A, l, u = r["probs"][i]
        if g["status"][i] != 1 or not adj.nondegenerate(A, g["act"][i], len(q)):
            continue
        used.append(int(i))
        for c in range(NCOT):
            want = adj.exact(P, A, r["x"][i], r["y"][i], g["act"][i], r["GX"][c, i], r["GY"][c, i])
            worst[c] = max(worst[c], adj.rel_err({k: g[k][c, i] for k in adj.GRADS}, want))
    print(f"{family}: Solved {len(solved)} of {len(info)}, non-degenerate {len(used)}, kernel vs exact worst rel per cotangent "
          f"{', '.join(f'{w:.2e}' for w in worst)} (bound {1000 * MEASURED_C[family]:.1e})")
    assert np.all(g["status"][solved] == 1)
    assert len(used) >= adj.MIN_NONDEGENERATE[family]
    assert max(worst) <= 1000 * MEASURED_C[family], worst


def test_a_selection_with_stale_neighbours(product_lib, oracle_lib):
    """`rows=`: an unsorted selection and k = 1 give the rows of the whole call; neighbours made stale by `update(rows=...)`
    do not block the call, a stale SELECTED instance does."""
    lib = product_lib
    probs = adj.problems(oracle_lib, "tiny")
    args = ref.stack(probs)
    rb = batch.ResidentBatch(lib, *args, **dict(OPTS, polish=True))
    rb.solve()
    count = rb.count
    GX, GY = _cotangents("tiny", NCOT, count, rb.n, rb.m)
    whole = rb.adjoint(dx=GX, dy=GY)
    sels = (np.array([count - 1, 0, 2]), np.array([4]))
    others = np.array([1, 3, 5])
    rb.update(q=np.asarray(args[4])[others] * 1.05, rows=others)  # stale neighbours
    with pytest.raises(batch.OSQPError, match="instance 1 .*resolve"):
        rb.adjoint(dx=GX, dy=GY)
    before = lib.osqp_amd_batch_adjoint_launches()
    for sel in sels:
        got = rb.adjoint(dx=GX[:, sel], dy=GY[:, sel], rows=sel)
        assert sorted(got) == sorted(whole)
        for k in adj.GRADS:
            assert got[k].shape == (NCOT, len(sel), whole[k].shape[2]) and _same(got[k], whole[k][:, sel]), (sel, k)
        assert _same(got["act"], whole["act"][sel]) and _same(got["status"], whole["status"][sel]) and np.all(got["status"] == 1)
    assert lib.osqp_amd_batch_adjoint_launches() == before + len(sels)
    bad = np.array([count - 1, 3, 0])
    with pytest.raises(batch.OSQPError, match="instance 3 .*resolve"):
        rb.adjoint(dx=GX[:, bad], dy=GY[:, bad], rows=bad)
    assert lib.osqp_amd_batch_adjoint_launches() == before + len(sels)
    rb.close()


def test_instances_without_a_solution_get_zero_rows_in_every_cotangent(product_lib, oracle_lib):
    """The batch of test_batch_adjoint_gpu.py::test_instances_without_a_solution_get_status_zero_and_zero_rows: 16 MPC
    instances, max_iter = 100, instances 1, 5, 9 primal infeasible (NaN rows in x and y)."""
    probs = ref.mpc_instances(oracle_lib, 0, 16, 2)
    args = ref.stack(probs)
    l2, u2 = args[5].copy(), args[6].copy()
    for i in (1, 5, 9):
        l2[i, 60] = u2[i, 60] = 1000.0
    rb = batch.ResidentBatch(product_lib, *args, **dict(OPTS, max_iter=100, polish=True))
    rb.update(l=l2, u=u2)
    x, y, info = rb.solve()
    GX, GY = _cotangents("mpc", NCOT, rb.count, rb.n, rb.m)
    g = rb.adjoint(dx=GX, dy=GY)
    one = rb.adjoint(dx=GX[2], dy=GY[2])
    sel = np.array([5, 0, 9])
    gs = rb.adjoint(dx=GX[:, sel], dy=GY[:, sel], rows=sel)
    rb.close()
    print("status", info[:, 1], "adjoint status", g["status"])
    assert np.all(info[[1, 5, 9], 1] == -3) and np.sum(info[:, 1] == 1) >= 4
    assert np.array_equal(g["status"] != 0, info[:, 1] == 1)
    for i in np.flatnonzero(info[:, 1] != 1):
        assert g["status"][i] == 0 and not np.any(g["act"][i])
        assert all(not np.any(g[k][:, i]) for k in adj.GRADS), i  # zeros in EVERY cotangent: no NaN either
    assert all(np.all(np.isfinite(g[k])) for k in adj.GRADS)
    solved = np.flatnonzero(info[:, 1] == 1)
    assert all(np.any(g["q"][c, solved] != 0.0) for c in range(NCOT)) and all(_same(g[k][2], one[k]) for k in adj.GRADS)
    assert all(_same(gs[k], g[k][:, sel]) for k in adj.GRADS) and _same(gs["status"], g["status"][sel])  # zeros at the POSITIONS


def test_a_batch_without_constraints(product_lib, oracle_lib):
    """m = 0, n = 5, ncot = 2: dq = -P^-1 g_x for each cotangent, and dPx."""
    rng = np.random.default_rng(50)
    n, count = 5, 4
    pat = sp.triu(sp.csc_matrix(np.ones((n, n))), format="csc"); pat.sort_indices()
    Px, Ps = [], []
    for _ in range(count):
        B = rng.standard_normal((n, n))
        U = sp.triu(sp.csc_matrix(B @ B.T + n * np.eye(n)), format="csc"); U.sort_indices()
        Px.append(U.data.copy()); Ps.append(U)
    q = rng.standard_normal((count, n))
    rb = batch.ResidentBatch(product_lib, pat, sp.csc_matrix((0, n)), np.array(Px), np.zeros((count, 0)), q, np.zeros((count, 0)),
                             np.zeros((count, 0)), **OPTS)
    x, y, info = rb.solve()
    GX = rng.standard_normal((2, count, n))
    g = rb.adjoint(dx=GX)
    single = [rb.adjoint(dx=GX[c]) for c in range(2)]
    with_dy = rb.adjoint(dx=GX, dy=np.zeros((2, count, 0)))
    rb.close()
    assert np.all(info[:, 1] == 1) and np.all(g["status"] == 1) and sorted(g) == ["Px", "q", "status"]
    assert g["q"].shape == (2, count, n) and g["Px"].shape == (2, count, pat.nnz)
    worst = 0.0
    for c in range(2):
        assert _same(g["q"][c], single[c]["q"]) and _same(g["Px"][c], single[c]["Px"]) and _same(with_dy["q"], g["q"])
        for i in range(count):
            want = adj.exact(Ps[i], sp.csc_matrix((0, n)), x[i], np.zeros(0), np.zeros(0, int), GX[c, i], np.zeros(0))
            worst = max(worst, adj.rel_err(dict(q=g["q"][c, i], Px=g["Px"][c, i], l=[], u=[], Ax=[]), want))
    print(f"m = 0: worst rel {worst:.2e}")
    assert worst <= 1000 * MEASURED_C["tiny"], worst


def test_host_and_device_forms_are_bit_identical(product_lib, oracle_lib):
    lib = product_lib
    probs = adj.problems(oracle_lib, "tiny")
    rb = batch.ResidentBatch(lib, *ref.stack(probs), **dict(OPTS, polish=True))
    rb.solve()
    count, ncot = rb.count, 2
    GX, GY = _cotangents("tiny", ncot, count, rb.n, rb.m)
    host = rb.adjoint(dx=GX, dy=GY)
    keep = []

    def dev(rows, cols):
        keep.append(batch.DeviceArray(lib, rows, cols))
        return keep[-1]

    cols = dict(q=rb.n, l=rb.m, u=rb.m, Px=rb.nnzP, Ax=rb.nnzA)
    out = {k: _View(dev(ncot * count, c), ncot) for k, c in cols.items()}
    out.update(act=dev(count, rb.m), status=dev(count, 1))
    dgx = _View(dev(ncot * count, rb.n).upload(GX.reshape(ncot * count, -1)), ncot)
    dgy = _View(dev(ncot * count, rb.m).upload(GY.reshape(ncot * count, -1)), ncot)
    before = lib.osqp_amd_batch_adjoint_launches()
    assert rb.adjoint(dx=dgx, dy=dgy, out=out) is out
    assert lib.osqp_amd_batch_adjoint_launches() == before + 1
    for k in out:
        assert _same(out[k].numpy().reshape(host[k].shape), host[k]), k
    sel = np.array([6, 1])
    part = {k: _View(dev(ncot * 2, cols[k]), ncot) for k in ("q", "Ax")}
    sgx = _View(dev(ncot * 2, rb.n).upload(np.ascontiguousarray(GX[:, sel]).reshape(ncot * 2, -1)), ncot)
    rb.adjoint(dx=sgx, want=("q", "Ax"), out=part, rows=sel)
    want = rb.adjoint(dx=GX, want=("q", "Ax"))
    assert all(_same(part[k].numpy(), want[k][:, sel]) for k in part)
    with pytest.raises(ValueError, match=r"out\['q'\]"):  # refused before the library is called
        rb.adjoint(dx=dgx, dy=dgy, out=dict(out, q=dev(count, rb.n)))
    assert lib.osqp_amd_batch_adjoint_launches() == before + 3
    for a in keep:
        a.free()
    rb.close()


@pytest.mark.parametrize("family", ["tiny", "ineq"])
def test_jacobian_on_the_device(product_lib, oracle_lib, family):
    """Reverse mode against `batch_adjoint_ref.exact` with unit cotangents, forward mode against `batch_jvp_ref.exact` with unit
    directions, both on the device's own x, y, act; chunks and `out_rows` against the full result, bit for bit."""
    lib = product_lib
    probs = adj.problems(oracle_lib, family)
    rb = batch.ResidentBatch(lib, *ref.stack(probs), **dict(OPTS, polish=True))
    rb.solve()
    rb.update_polish(0)
    x, y, info = rb.solve()
    of, wrt = ("x", "y"), ("q", "l", "u")
    n, m, count = rb.n, rb.m, rb.count
    n_adj, n_jvp = lib.osqp_amd_batch_adjoint_launches(), lib.osqp_amd_batch_jvp_launches()
    rev = rb.jacobian(of=of, wrt=wrt, mode="reverse")
    fwd = rb.jacobian(of=of, wrt=wrt, mode="forward")
    assert (lib.osqp_amd_batch_adjoint_launches(), lib.osqp_amd_batch_jvp_launches()) == (n_adj + 1, n_jvp + 1)  # one launch each
    rev2, fwd2 = rb.jacobian(of=of, wrt=wrt, mode="reverse", chunk=2), rb.jacobian(of=of, wrt=wrt, mode="forward", chunk=2)
    assert lib.osqp_amd_batch_adjoint_launches() == n_adj + 1 + (n + m + 1) // 2
    assert lib.osqp_amd_batch_jvp_launches() == n_jvp + 1 + (n + 2 * m + 1) // 2
    pick = dict(x=[n - 1, 1], y=[m - 1, 0])
    rev_p, fwd_p = (rb.jacobian(of=of, wrt=wrt, mode=mode, out_rows=pick) for mode in ("reverse", "forward"))
    rb.close()
    cols = dict(x=n, y=m, q=n, l=m, u=m)
    assert sorted(map(str, rev)) == sorted(map(str, fwd)) == sorted(map(str, [(o, w) for o in of for w in wrt] + ["act", "status"]))
    for o in of:
        for w in wrt:
            assert rev[(o, w)].shape == fwd[(o, w)].shape == (count, cols[o], cols[w])
            assert _same(rev2[(o, w)], rev[(o, w)]) and _same(fwd2[(o, w)], fwd[(o, w)]), (o, w)
            assert _same(rev_p[(o, w)], rev[(o, w)][:, pick[o], :]) and _same(fwd_p[(o, w)], fwd[(o, w)][:, pick[o], :]), (o, w)
    assert _same(rev["act"], fwd["act"]) and _same(rev["status"], fwd["status"]) and _same(rev2["status"], rev["status"])
    w_rev, w_fwd, used = 0.0, 0.0, []
    for i in np.flatnonzero(info[:, 1] == 1):
        P, q, A, l, u = probs[i]
        act = rev["act"][i]
        if rev["status"][i] != 1 or not adj.nondegenerate(A, act, n):
            continue
        used.append(int(i))
        for j in range(n + m):  # row j of the Jacobian of (x, y): the adjoint of the unit cotangent e_j
            e = np.zeros(n + m); e[j] = 1.0
            want = adj.exact(P, A, x[i], y[i], act, e[:n], e[n:])
            o, a = ("x", j) if j < n else ("y", j - n)
            got = dict(q=rev[(o, "q")][i, a], l=rev[(o, "l")][i, a], u=rev[(o, "u")][i, a], Px=want["Px"], Ax=want["Ax"])
            w_rev = max(w_rev, adj.rel_err(got, want))
        for w in wrt:  # column b of the Jacobian with respect to w: the sensitivities along the unit direction e_b of w
            for b in range(cols[w]):
                e = np.zeros(cols[w]); e[b] = 1.0
                tx, ty = jv.exact(P, A, x[i], y[i], act, {w: e})
                w_fwd = max(w_fwd, jv.rel_err(fwd[("x", w)][i, :, b], fwd[("y", w)][i, :, b], tx, ty))
    print(f"{family}: non-degenerate {len(used)}, jacobian vs exact worst rel: reverse {w_rev:.2e} (bound {1000 * MEASURED_C[family]:.1e}), "
          f"forward {w_fwd:.2e} (bound {1000 * JVP_MEASURED_C[family]:.1e})")
    assert len(used) >= adj.MIN_NONDEGENERATE[family]
    assert w_rev <= 1000 * MEASURED_C[family], w_rev
    assert w_fwd <= 1000 * JVP_MEASURED_C[family], w_fwd


def test_torch_batched_reverse_mode(product_lib, oracle_lib):
    """`torch.func.jacrev` and `vmap` over a VJP of the layer: ONE adjoint launch each, with the bits of `ResidentBatch`."""
    import torch

    from osqp_jl_amd.qp_layer import BatchQPLayer

    lib = product_lib
    probs = adj.problems(oracle_lib, "tiny")
    args = ref.stack(probs)
    rb = batch.ResidentBatch(lib, *args, **dict(OPTS, polish=True))
    layer = BatchQPLayer(rb)
    count, n = rb.count, rb.n
    dev = torch.device("cuda:0")
    q_t = torch.tensor(args[4], device=dev)

    def f(q):
        return layer(q=q)[0]

    before = lib.osqp_amd_batch_adjoint_launches()
    J = torch.func.jacrev(f)(q_t)
    assert lib.osqp_amd_batch_adjoint_launches() == before + 1  # count * n cotangents, one launch
    assert tuple(J.shape) == (count, n, count, n)
    J = J.cpu().numpy()
    jac = rb.jacobian(of=("x",), wrt=("q",), mode="reverse")
    want = np.zeros((count, n, count, n))
    for i in range(count):
        want[i, :, i, :] = jac[("x", "q")][i]  # block-diagonal over the instances
    assert np.all(jac["status"] == 1) and np.any(want != 0.0) and _same(J, want)
    jl = layer.jacobian(of=("x",), wrt=("q",), mode="reverse")  # the same on the device
    assert jl[("x", "q")].is_cuda and _same(jl[("x", "q")].cpu().numpy(), jac[("x", "q")])
    assert _same(jl["status"].cpu().numpy().ravel(), jac["status"]) and _same(jl["act"].cpu().numpy(), jac["act"])
    # vmap over a VJP: three cotangents, one launch, the bits of three backward calls
    G = torch.tensor(_cotangents("tiny", NCOT, count, n, rb.m)[0], device=dev)
    xs, vjp_fn = torch.func.vjp(f, q_t)
    before = lib.osqp_amd_batch_adjoint_launches()
    (dq,) = torch.func.vmap(vjp_fn)(G)
    assert lib.osqp_amd_batch_adjoint_launches() == before + 1 and tuple(dq.shape) == (NCOT, count, n)
    for c in range(NCOT):
        q_c = torch.tensor(args[4], device=dev, requires_grad=True)
        layer(q=q_c)[0].backward(G[c])
        assert _same(dq[c].cpu().numpy(), q_c.grad.cpu().numpy()) and np.any(q_c.grad.cpu().numpy() != 0.0), c
    # the stamp rule holds for the batched pull-back
    xs, vjp_fn = torch.func.vjp(f, q_t)
    layer(q=q_t)
    before = lib.osqp_amd_batch_adjoint_launches()
    with pytest.raises(RuntimeError, match="solved again"):
        torch.func.vmap(vjp_fn)(G)
    assert lib.osqp_amd_batch_adjoint_launches() == before
    rb.close()
