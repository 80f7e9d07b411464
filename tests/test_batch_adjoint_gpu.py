"""Adjoint derivatives on the resident batch (osqp_amd_batch_adjoint: k_batch_adjoint; `ResidentBatch.adjoint`;
`qp_layer.BatchQPFunction`) on the GPU.  The reference is `batch_adjoint_ref.exact` -- a dense solve with the KKT matrix of
the active set in the caller's units -- on the GPU's OWN returned x, y and act, which isolates the kernel from ADMM noise;
compared are the instances whose K is non-singular under the returned act.

Bound of the kernel against `exact`, relative to max(1, max|exact|) per gradient: 1000 times the model-vs-exact figure
tests/test_batch_adjoint_host.py records for the family (MEASURED_C): the kernel sums in another order, and
cond K * eps <= 1e-9 on these families.
FIGURES: NOT YET MEASURED ON THE MI355X -- this file was written without access to a device.  What is known: the kernel's
source executed on the CPU (one thread per work-item, barriers for the workgroup's) from the oracle's scaled state, against
`exact` on the non-degenerate instances -- tiny 1.0e-15, ineq 9.0e-15, wide300 3.3e-12, tri128 8.3e-15, eq100 2.5e-15, mpc
(first 16) 5.1e-15: the model's own figures, a factor 200 or more inside the bounds.  The first test prints the figures of
a run; whoever runs it on a device replaces this paragraph with them."""
import numpy as np
import pytest
import scipy.sparse as sp

from osqp_jl_amd import batch
import batch_adjoint_ref as adj
import batch_resident_ref as ref
from batch_resident_ref import OPTS
from test_batch_adjoint_host import MEASURED_C
from test_batch_polish_gpu import TOL as POLISH_TOL

pytestmark = pytest.mark.gpu

_runs = {}


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _run(product_lib, oracle_lib, family):
    """One handle per family, once per session: resolve with polish = 1 (and the act of that state, `act_polished`), again
    with polish = 0, adjoint with every output."""
    if family not in _runs:
        probs = adj.problems(oracle_lib, family)
        args = ref.stack(probs)
        rb = batch.ResidentBatch(product_lib, *args, **dict(OPTS, polish=True))
        rb.solve()
        pst = rb.polish_status()
        gx, gy = adj.incoming(family, rb.count, rb.n, rb.m)
        act_polished = rb.adjoint(dx=gx, dy=gy, want=())["act"]
        rb.update_polish(0)
        x, y, info = rb.solve()
        g = rb.adjoint(dx=gx, dy=gy)
        rb.close()
        _runs[family] = dict(probs=probs, x=x, y=y, info=info, pst=pst, gx=gx, gy=gy, g=g, act_polished=act_polished)
    return _runs[family]


def _against_exact(probs, x, y, g, gx, gy, rows):
    """(worst relative error, instances compared) over the non-degenerate instances among `rows`."""
    worst, used = 0.0, []
    for i in rows:
        P, q, A, l, u = probs[i]
        if g["status"][i] != 1 or not adj.nondegenerate(A, g["act"][i], len(q)):
            continue
        want = adj.exact(P, A, x[i], y[i], g["act"][i], gx[i], gy[i])
        worst = max(worst, adj.rel_err({k: g[k][i] for k in adj.GRADS}, want))
        used.append(i)
    return worst, used


@pytest.mark.parametrize("family", adj.FAMILIES)
def test_kernel_agrees_with_the_exact_adjoint(product_lib, oracle_lib, family):
    """The five gradients against `exact` on the x, y, act returned after the polish = 0 resolve; status 1 on every Solved
    instance; and the act of the POLISHED state (the adjoint called between the two resolves) equal to the classification of
    the oracle's polished iterate wherever both sides accepted the polish.  Like is compared with like: the ADMM re-solve
    that follows moves weakly active rows by its own noise (on the oracle itself it flips one row of MPC instance 45), which
    is what the first comparison is isolated from; the rows where the re-solved act differs are printed."""
    r = _run(product_lib, oracle_lib, family)
    g, info = r["g"], r["info"]
    solved = np.flatnonzero(info[:, 1] == 1)
    worst, used = _against_exact(r["probs"], r["x"], r["y"], g, r["gx"], r["gy"], solved)
    sols = adj.oracle_solutions(oracle_lib, family)
    both = [i for i in range(len(sols)) if r["pst"][i] == 1 and sols[i]["polish"] == 1]
    differ = [i for i in both if not np.array_equal(r["act_polished"][i], sols[i]["act"])]
    later = [i for i in both if not np.array_equal(g["act"][i], sols[i]["act"])]
    print(f"{family}: Solved {len(solved)} of {len(info)}, non-degenerate {len(used)}, kernel vs exact worst rel {worst:.2e} "
          f"(bound {1000 * MEASURED_C[family]:.1e}), polish accepted on both sides {len(both)}, polished act differs at {differ}, re-solved act at {later}")
    assert np.all(g["status"][solved] == 1)
    assert len(used) >= adj.MIN_NONDEGENERATE[family]
    assert worst <= 1000 * MEASURED_C[family], worst
    assert not differ


def test_host_and_device_forms_are_bit_identical_and_outputs_independent(product_lib, oracle_lib):
    probs = adj.problems(oracle_lib, "ineq")
    rb = batch.ResidentBatch(product_lib, *ref.stack(probs), **dict(OPTS, polish=True))
    rb.solve()
    gx, gy = adj.incoming("ineq", rb.count, rb.n, rb.m)
    host = rb.adjoint(dx=gx, dy=gy)
    cols = dict(q=rb.n, l=rb.m, u=rb.m, Px=rb.nnzP, Ax=rb.nnzA, act=rb.m, status=1)
    dev = {k: batch.DeviceArray(product_lib, rb.count, c) for k, c in cols.items()}
    dgx, dgy = (batch.DeviceArray(product_lib, *a.shape).upload(a) for a in (gx, gy))
    assert rb.adjoint(dx=dgx, dy=dgy, out=dev) is dev
    for k in cols:
        assert _same(dev[k].numpy().reshape(host[k].shape), host[k]), k
    part = rb.adjoint(dx=gx, dy=gy, want=("l", "Ax"))
    assert sorted(part) == ["Ax", "act", "l", "status"]
    assert all(_same(part[k], host[k]) for k in part)
    only_x, only_y = rb.adjoint(dx=gx, want=("q",)), rb.adjoint(dx=gx, dy=np.zeros_like(gy), want=("q",))
    assert _same(only_x["q"], only_y["q"])  # a missing gradient is zero
    for d in list(dev.values()) + [dgx, dgy]:
        d.free()
    rb.close()


def test_instances_without_a_solution_get_status_zero_and_zero_rows(product_lib, oracle_lib):
    """The batch of test_batch_polish_gpu.py::test_instances_without_a_solution_are_left_alone: 16 MPC instances,
    max_iter = 100, instances 1, 5, 9 primal infeasible (NaN rows in x and y)."""
    probs = ref.mpc_instances(oracle_lib, 0, 16, 2)
    args = ref.stack(probs)
    l2, u2 = args[5].copy(), args[6].copy()
    for i in (1, 5, 9):
        l2[i, 60] = u2[i, 60] = 1000.0
    rb = batch.ResidentBatch(product_lib, *args, **dict(OPTS, max_iter=100, polish=True))
    rb.update(l=l2, u=u2)
    x, y, info = rb.solve()
    gx, gy = adj.incoming("mpc", rb.count, rb.n, rb.m)
    g = rb.adjoint(dx=gx, dy=gy)
    rb.close()
    print("status", info[:, 1], "adjoint status", g["status"])
    assert np.all(info[[1, 5, 9], 1] == -3) and np.sum(info[:, 1] == 1) >= 4
    assert np.array_equal(g["status"] != 0, info[:, 1] == 1)
    for i in np.flatnonzero(info[:, 1] != 1):
        assert g["status"][i] == 0 and not np.any(g["act"][i])
        assert all(not np.any(g[k][i]) for k in adj.GRADS), i  # zeros: no NaN either
    assert all(np.all(np.isfinite(g[k])) for k in adj.GRADS)
    moved = [(P, q, A, l2[i], u2[i]) for i, (P, q, A, l, u) in enumerate(probs)]
    worst, used = _against_exact(moved, x, y, g, gx, gy, np.flatnonzero(info[:, 1] == 1))
    print(f"Solved neighbours compared {used}, worst rel {worst:.2e}")
    assert len(used) >= 1 and worst <= 1000 * MEASURED_C["mpc"], worst


def test_a_batch_without_constraints(product_lib, oracle_lib):
    """m = 0, n = 5: dq = -P^-1 g_x, and dPx."""
    rng = np.random.default_rng(50)
    n, count = 5, 4
    pat = sp.triu(sp.csc_matrix(np.ones((n, n))), format="csc"); pat.sort_indices()
    Px, probs = [], []
    for _ in range(count):
        B = rng.standard_normal((n, n))
        U = sp.triu(sp.csc_matrix(B @ B.T + n * np.eye(n)), format="csc"); U.sort_indices()
        Px.append(U.data.copy())
        probs.append((U, rng.standard_normal(n), sp.csc_matrix((0, n)), np.zeros(0), np.zeros(0)))
    q = np.array([p[1] for p in probs])
    rb = batch.ResidentBatch(product_lib, pat, sp.csc_matrix((0, n)), np.array(Px), np.zeros((count, 0)), q, np.zeros((count, 0)),
                             np.zeros((count, 0)), **OPTS)
    x, y, info = rb.solve()
    gx = rng.standard_normal((count, n))
    g = rb.adjoint(dx=gx)
    rb.close()
    assert np.all(info[:, 1] == 1) and np.all(g["status"] == 1) and sorted(g) == ["Px", "q", "status"]
    worst = 0.0
    for i, (P, qi, A, l, u) in enumerate(probs):
        want = adj.exact(P, A, x[i], np.zeros(0), np.zeros(0, int), gx[i], np.zeros(0))
        assert np.allclose(want["q"], -np.linalg.solve(adj.full_P(P), gx[i]), rtol=0, atol=1e-13)
        worst = max(worst, adj.rel_err(dict(g, q=g["q"][i], Px=g["Px"][i], l=[], u=[], Ax=[]), want))
    print(f"m = 0: worst rel {worst:.2e}")
    assert worst <= 1000 * MEASURED_C["tiny"], worst


def test_life_cycle_of_the_adjoint(product_lib, oracle_lib):
    probs = adj.problems(oracle_lib, "tiny")
    args = ref.stack(probs)
    gx, gy = adj.incoming("tiny", len(probs), 5, 3)
    a = batch.ResidentBatch(product_lib, *args, **dict(OPTS, polish=True))
    twin = batch.ResidentBatch(product_lib, *args, **dict(OPTS, polish=True))
    n_adj, n_pol = product_lib.osqp_amd_batch_adjoint_launches(), product_lib.osqp_amd_batch_polish_launches()
    with pytest.raises(batch.OSQPError, match="resolve"):  # before any resolve
        a.adjoint(dx=gx, dy=gy)
    first_a, first_t = a.solve(), twin.solve()
    g = a.adjoint(dx=gx, dy=gy)
    second_a, second_t = a.solve(), twin.solve()
    assert all(_same(p, q) for p, q in zip(first_a + second_a, first_t + second_t))  # the adjoint changes nothing on the handle
    assert product_lib.osqp_amd_batch_adjoint_launches() == n_adj + 1  # the refused call and the twin launched nothing
    assert product_lib.osqp_amd_batch_polish_launches() == n_pol + 4  # one per resolve, as before
    assert all(_same(v, w) for v, w in zip(a.adjoint(dx=gx, dy=gy).values(), a.adjoint(dx=gx, dy=gy).values()))
    a.update(q=args[4] * 1.01)
    with pytest.raises(batch.OSQPError, match="resolve"):  # the data changed since the last resolve
        a.adjoint(dx=gx, dy=gy)
    a.solve()
    a.warm_start(x=first_a[0])
    with pytest.raises(batch.OSQPError, match="resolve"):  # the iterate changed
        a.adjoint(dx=gx, dy=gy)
    a.solve()
    assert np.all(a.adjoint(dx=gx, dy=gy)["status"] == 1)
    buf = np.zeros((len(probs), 5))
    assert product_lib.osqp_amd_batch_adjoint(a.handle, None, None, buf.ctypes.data, None, None, None, None, None, None, 0) == 1
    mpc_handle = batch.MpcBatch(product_lib, 4, seed=2, **OPTS)  # the other family's handle is refused
    assert product_lib.osqp_amd_batch_adjoint(mpc_handle.handle, buf.ctypes.data, None, buf.ctypes.data, None, None, None, None, None, None, 0) == 1
    mpc_handle.close()
    assert product_lib.osqp_amd_batch_adjoint_launches() == n_adj + 4
    assert np.all(g["status"] == 1)
    a.close(); twin.close()


def test_end_to_end_finite_differences(product_lib, oracle_lib):
    """`tiny`, polish = 1: three GPU solves, at the data and at +-h d along (q, l, u), h = 1e-4 (the solution is piecewise
    affine in these); compared are the instances with three accepted polishes and one returned act.  Each polished x / y is
    within the polish tests' tolerance of the exact one, so |fd - analytic| <= TOL / h * |g|_1."""
    probs = adj.problems(oracle_lib, "tiny")
    args = ref.stack(probs)
    count, n, m = len(probs), 5, 3
    gx, gy = adj.incoming("tiny", count, n, m)
    rng = np.random.default_rng(11)
    dq, dl, du = rng.standard_normal((count, n)), rng.standard_normal((count, m)), rng.standard_normal((count, m))
    du = np.where(args[5] == args[6], dl, du)  # an equality row moves as one
    h, runs = 1e-4, []
    for s in (0.0, 1.0, -1.0):
        rb = batch.ResidentBatch(product_lib, *args[:4], args[4] + s * h * dq, args[5] + s * h * dl, args[6] + s * h * du,
                                 **dict(OPTS, polish=True))
        x, y, info = rb.solve()
        runs.append(dict(x=x, y=y, pst=rb.polish_status(), g=rb.adjoint(dx=gx, dy=gy)))
        rb.close()
    base, used, worst = runs[0], 0, 0.0
    for i in range(count):
        if not all(r["pst"][i] == 1 and np.array_equal(r["g"]["act"][i], base["g"]["act"][i]) for r in runs):
            continue
        used += 1
        loss = [gx[i] @ r["x"][i] + gy[i] @ r["y"][i] for r in runs[1:]]
        fd = (loss[0] - loss[1]) / (2 * h)
        an = float(base["g"]["q"][i] @ dq[i] + base["g"]["l"][i] @ dl[i] + base["g"]["u"][i] @ du[i])
        bound = POLISH_TOL / h * (np.sum(np.abs(gx[i])) + np.sum(np.abs(gy[i])))
        print(f"inst {i}: fd {fd:.12e} analytic {an:.12e} |diff| {abs(fd - an):.2e} bound {bound:.2e}")
        worst = max(worst, abs(fd - an) / bound)
    print(f"{used} of {count} compared, worst |diff| / bound {worst:.2e}")
    assert used >= 5 and worst <= 1.0


def test_torch_layer(product_lib, oracle_lib):
    import torch

    from osqp_jl_amd.qp_layer import BatchQPLayer

    probs = adj.problems(oracle_lib, "ineq")
    args = ref.stack(probs)
    rb = batch.ResidentBatch(product_lib, *args, **dict(OPTS, polish=True))
    layer = BatchQPLayer(rb)
    gx, gy = adj.incoming("ineq", rb.count, rb.n, rb.m)
    dev = torch.device("cuda:0")
    wx, wy = torch.tensor(gx, device=dev), torch.tensor(gy, device=dev)
    names = ("q", "l", "u", "Px", "Ax")
    host = dict(q=args[4], l=args[5], u=args[6], Px=args[2], Ax=args[3])
    t = {k: torch.tensor(host[k], device=dev, requires_grad=True) for k in names}
    x, y = layer(**t)
    ((wx * x).sum() + (wy * y).sum()).backward()
    want = rb.adjoint(dx=gx, dy=gy)
    for k in names:
        assert _same(t[k].grad.cpu().numpy(), want[k]), k
    # only the inputs that require a gradient get one; None keeps the handle's data
    q2, l2 = torch.tensor(host["q"], device=dev, requires_grad=True), torch.tensor(host["l"], device=dev)
    x2, y2 = layer(q=q2, l=l2)
    ((wx * x2).sum() + (wy * y2).sum()).backward()
    assert l2.grad is None and _same(q2.grad.cpu().numpy(), rb.adjoint(dx=gx, dy=gy, want=("q",))["q"])
    # the handle holds one solution: the first graph's backward after a second forward raises
    q3 = torch.tensor(host["q"], device=dev, requires_grad=True)
    x3, _ = layer(q=q3)
    layer(q=q2)
    with pytest.raises(RuntimeError, match="solved again"):
        x3.sum().backward()
    rb.close()
