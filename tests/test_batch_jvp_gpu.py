"""Forward sensitivities on the resident batch (osqp_amd_batch_jvp: k_batch_jvp; `ResidentBatch.jvp`;
`qp_layer.BatchQPFunction.jvp`) on the GPU.  The reference is `batch_jvp_ref.exact` -- a dense solve with the KKT matrix of the
active set in the caller's units -- on the GPU's OWN returned x, y and act, which isolates the kernel from ADMM noise; compared
are the instances whose K is non-singular under the returned act.

Bounds.  Kernel against `exact`, relative to max(1, max|exact|) per output: 1000 times the model-vs-exact figure
tests/test_batch_jvp_host.py records for the family (MEASURED_C) -- the margin of the adjoint GPU test over its CPU model: the
kernel sums in another order, and cond K * eps <= 1e-9 on these families.  Duality with the device adjoint,
|g_x . tx + g_y . ty - sum <g_k, d_k>| / max(1, sum |terms|): 1000 times the same quantity of the two CPU models (MEASURED_D).
Both tests print their figures before they assert.  Measured on an MI355X when this file was written (kernel vs exact /
duality gap): tiny 7.8e-16 / 1.2e-16, ineq 1.5e-14 / 8.9e-17, wide300 3.0e-12 / 1.5e-16, tri128 1.1e-14 / 3.5e-17, eq100
3.7e-15 / 1.6e-16, mpc 5.7e-15 / 5.6e-17; end to end against central differences of polished solves, worst entry 2.0e-11
(tiny) and 3.5e-10 (ineq) under the bound 1e-2."""
import numpy as np
import pytest
import scipy.sparse as sp

from osqp_jl_amd import batch
import batch_adjoint_ref as adj
import batch_jvp_ref as jv
import batch_resident_ref as ref
from batch_resident_ref import OPTS
from test_batch_jvp_host import MEASURED_C, MEASURED_D
from test_batch_polish_gpu import TOL as POLISH_TOL

pytestmark = pytest.mark.gpu

NDIR = 3
_runs = {}


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _run(product_lib, oracle_lib, family):
    """One handle per family, once per session: resolve with polish = 1, again with polish = 0, then on that state the
    sensitivities along NDIR directions of all five arrays, each direction alone, a subset of the tangents with and without
    explicit zeros for the others, and the adjoint."""
    if family not in _runs:
        probs = jv.problems(oracle_lib, family)
        rb = batch.ResidentBatch(product_lib, *ref.stack(probs), **dict(OPTS, polish=True))
        rb.solve()
        rb.update_polish(0)
        x, y, info = rb.solve()
        d = jv.tangents(family, NDIR, probs)
        gx, gy = adj.incoming(family, rb.count, rb.n, rb.m)
        t = rb.jvp(**d)
        alone = [rb.jvp(**{k: v[j] for k, v in d.items()}) for j in range(NDIR)]
        part = rb.jvp(q=d["q"], Ax=d["Ax"])
        zeros = rb.jvp(q=d["q"], Ax=d["Ax"], l=np.zeros_like(d["l"]), u=np.zeros_like(d["u"]), Px=np.zeros_like(d["Px"]))
        g = rb.adjoint(dx=gx, dy=gy)
        rb.close()
        _runs[family] = dict(probs=probs, x=x, y=y, info=info, d=d, t=t, alone=alone, part=part, zeros=zeros, gx=gx, gy=gy, g=g)
    return _runs[family]


def _against_exact(probs, x, y, t, d, rows):
    """(worst relative error over the directions, instances compared) over the non-degenerate instances among `rows`."""
    worst, used = 0.0, []
    for i in rows:
        P, q, A, l, u = probs[i]
        if t["status"][i] != 1 or not jv.nondegenerate(A, t["act"][i], len(q)):
            continue
        for j in range(d["q"].shape[0]):
            want = jv.exact(P, A, x[i], y[i], t["act"][i], jv.direction(d, j, i))
            worst = max(worst, jv.rel_err(t["x"][j, i], t["y"][j, i], *want))
        used.append(i)
    return worst, used


@pytest.mark.parametrize("family", jv.FAMILIES)
def test_kernel_agrees_with_the_exact_sensitivities(product_lib, oracle_lib, family):
    r = _run(product_lib, oracle_lib, family)
    t, info = r["t"], r["info"]
    solved = np.flatnonzero(info[:, 1] == 1)
    worst, used = _against_exact(r["probs"], r["x"], r["y"], t, r["d"], solved)
    print(f"{family}: Solved {len(solved)} of {len(info)}, non-degenerate {len(used)}, kernel vs exact worst rel {worst:.2e} "
          f"(bound {1000 * MEASURED_C[family]:.1e})")
    assert t["x"].shape == (NDIR,) + r["x"].shape and t["y"].shape == (NDIR,) + r["y"].shape
    assert np.all(t["status"][solved] == 1)
    assert _same(t["act"], r["g"]["act"])  # the classification of the adjoint
    assert len(used) >= jv.MIN_NONDEGENERATE[family]
    assert worst <= 1000 * MEASURED_C[family], worst


@pytest.mark.parametrize("family", jv.FAMILIES)
def test_duality_with_the_device_adjoint(product_lib, oracle_lib, family):
    r = _run(product_lib, oracle_lib, family)
    t, g, worst, used = r["t"], r["g"], 0.0, 0
    for i in np.flatnonzero(r["info"][:, 1] == 1):
        if t["status"][i] != 1 or g["status"][i] != 1 or not jv.nondegenerate(r["probs"][i][2], t["act"][i], len(r["probs"][i][1])):
            continue
        used += 1
        for j in range(NDIR):
            worst = max(worst, jv.duality_gap(r["gx"][i], r["gy"][i], t["x"][j, i], t["y"][j, i], {k: g[k][i] for k in adj.GRADS},
                                              jv.direction(r["d"], j, i)))
    print(f"{family}: {used} instances, duality gap jvp / adjoint worst rel {worst:.2e} (bound {1000 * MEASURED_D[family]:.1e})")
    assert used >= jv.MIN_NONDEGENERATE[family]
    assert worst <= 1000 * MEASURED_D[family], worst


@pytest.mark.parametrize("family", jv.FAMILIES)
def test_directions_are_independent(product_lib, oracle_lib, family):
    r = _run(product_lib, oracle_lib, family)
    t = r["t"]
    for j, one in enumerate(r["alone"]):
        assert one["x"].shape == r["x"].shape and one["y"].shape == r["y"].shape
        assert _same(one["x"], t["x"][j]) and _same(one["y"], t["y"][j]), j
        assert _same(one["act"], t["act"]) and _same(one["status"], t["status"])
    assert all(_same(r["part"][k], r["zeros"][k]) for k in ("x", "y", "act", "status"))  # a missing tangent is zero
    assert np.any(r["part"]["x"] != t["x"])


class _View:
    """A [ndir x count x cols] view of a DeviceArray of ndir * count rows: what `ResidentBatch.jvp` takes by address."""

    def __init__(self, arr, ndir):
        self.arr, self.shape = arr, (ndir, arr.shape[0] // ndir, arr.shape[1])

    def data_ptr(self):
        return self.arr.data_ptr()

    def numpy(self):
        return self.arr.numpy().reshape(self.shape)


def test_host_and_device_forms_are_bit_identical_and_outputs_independent(product_lib, oracle_lib):
    probs = jv.problems(oracle_lib, "ineq")
    rb = batch.ResidentBatch(product_lib, *ref.stack(probs), **dict(OPTS, polish=True))
    rb.solve()
    d = jv.tangents("ineq", NDIR, probs)
    host = rb.jvp(**d)
    keep = []

    def dev(rows, cols):
        keep.append(batch.DeviceArray(product_lib, rows, cols))
        return keep[-1]

    # several directions: [ndir x count x cols] device arrays by address
    din = {k: _View(dev(NDIR * rb.count, v.shape[2]).upload(v.reshape(NDIR * rb.count, -1)), NDIR) for k, v in d.items()}
    out = dict(x=_View(dev(NDIR * rb.count, rb.n), NDIR), y=_View(dev(NDIR * rb.count, rb.m), NDIR), act=dev(rb.count, rb.m), status=dev(rb.count, 1))
    assert rb.jvp(**din, out=out) is out
    for k in out:
        assert _same(out[k].numpy().reshape(host[k].shape), host[k]), k
    # one direction, plain DeviceArrays, act and status not wanted
    one = rb.jvp(**{k: v[1] for k, v in d.items()})
    din1 = {k: dev(rb.count, v.shape[2]).upload(v[1]) for k, v in d.items()}
    out1 = dict(x=dev(rb.count, rb.n), y=dev(rb.count, rb.m))
    rb.jvp(**din1, out=out1)
    assert _same(out1["x"].numpy(), one["x"]) and _same(out1["y"].numpy(), one["y"])
    assert _same(one["x"], host["x"][1]) and _same(one["y"], host["y"][1])
    # the C entry with one output only: the other is not changed by its absence
    tx, ty = np.empty_like(host["x"]), np.empty_like(host["y"])
    ptr = [d[k].ctypes.data for k in jv.TANGENTS]
    assert product_lib.osqp_amd_batch_jvp(rb.handle, NDIR, *ptr, tx.ctypes.data, None, None, None, 0) == 0
    assert product_lib.osqp_amd_batch_jvp(rb.handle, NDIR, *ptr, None, ty.ctypes.data, None, None, 0) == 0
    assert _same(tx, host["x"]) and _same(ty, host["y"])
    for a in keep:
        a.free()
    rb.close()


def test_instances_without_a_solution_get_status_zero_and_zero_rows(product_lib, oracle_lib):
    """The batch of the adjoint test of the same name: 16 MPC instances, max_iter = 100, instances 1, 5, 9 primal infeasible."""
    probs = ref.mpc_instances(oracle_lib, 0, 16, 2)
    args = ref.stack(probs)
    l2, u2 = args[5].copy(), args[6].copy()
    for i in (1, 5, 9):
        l2[i, 60] = u2[i, 60] = 1000.0
    rb = batch.ResidentBatch(product_lib, *args, **dict(OPTS, max_iter=100, polish=True))
    rb.update(l=l2, u=u2)
    x, y, info = rb.solve()
    moved = [(P, q, A, l2[i], u2[i]) for i, (P, q, A, l, u) in enumerate(probs)]
    d = jv.tangents("mpc", NDIR, moved)
    t = rb.jvp(**d)
    rb.close()
    print("status", info[:, 1], "jvp status", t["status"])
    assert np.all(info[[1, 5, 9], 1] == -3) and np.sum(info[:, 1] == 1) >= 4
    assert np.array_equal(t["status"] != 0, info[:, 1] == 1)
    for i in np.flatnonzero(info[:, 1] != 1):
        assert t["status"][i] == 0 and not np.any(t["act"][i])
        assert not np.any(t["x"][:, i]) and not np.any(t["y"][:, i]), i  # zeros in every direction: no NaN either
    assert np.all(np.isfinite(t["x"])) and np.all(np.isfinite(t["y"]))
    worst, used = _against_exact(moved, x, y, t, d, np.flatnonzero(info[:, 1] == 1))
    print(f"Solved neighbours compared {used}, worst rel {worst:.2e}")
    assert len(used) >= 1 and worst <= 1000 * MEASURED_C["mpc"], worst


def test_a_batch_without_constraints(product_lib, oracle_lib):
    """m = 0, n = 5: tx = -P^-1 (tq + tP x); y-sized and A-sized tangents are ignored, "y" and "act" are left out."""
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
    d = dict(q=rng.standard_normal((2, count, n)), Px=rng.standard_normal((2, count, pat.nnz)))
    t = rb.jvp(**d, l=np.zeros((2, count, 0)), Ax=np.zeros((2, count, 0)))
    rb.close()
    assert np.all(info[:, 1] == 1) and np.all(t["status"] == 1) and sorted(t) == ["status", "x"]
    worst = 0.0
    for i, (P, qi, A, l, u) in enumerate(probs):
        for j in range(2):
            dj = dict(q=d["q"][j, i], Px=d["Px"][j, i])
            want = jv.exact(P, A, x[i], np.zeros(0), np.zeros(0, int), dj)
            tP = jv.tangent_matrices(P, A, dj)[0]
            assert np.allclose(want[0], -np.linalg.solve(adj.full_P(P), dj["q"] + tP @ x[i]), rtol=0, atol=1e-13)
            worst = max(worst, jv.rel_err(t["x"][j, i], np.zeros(0), *want))
    print(f"m = 0: worst rel {worst:.2e}")
    assert worst <= 1000 * MEASURED_C["tiny"], worst


def test_life_cycle_of_the_jvp(product_lib, oracle_lib):
    probs = jv.problems(oracle_lib, "tiny")
    args = ref.stack(probs)
    d = {k: v[0] for k, v in jv.tangents("tiny", 1, probs).items()}
    lib = product_lib
    a = batch.ResidentBatch(lib, *args, **dict(OPTS, polish=True))
    twin = batch.ResidentBatch(lib, *args, **dict(OPTS, polish=True))
    n_jvp = lib.osqp_amd_batch_jvp_launches()
    with pytest.raises(batch.OSQPError, match="resolve"):  # before any resolve
        a.jvp(**d)
    first_a, first_t = a.solve(), twin.solve()
    others = (lib.osqp_amd_batch_adjoint_launches(), lib.osqp_amd_batch_polish_launches(), lib.osqp_amd_batch_cert_launches())
    t = a.jvp(**d)
    again = a.jvp(**d)
    assert (lib.osqp_amd_batch_adjoint_launches(), lib.osqp_amd_batch_polish_launches(), lib.osqp_amd_batch_cert_launches()) == others
    assert lib.osqp_amd_batch_jvp_launches() == n_jvp + 2  # the refused call launched nothing
    assert all(_same(t[k], again[k]) for k in t)
    second_a, second_t = a.solve(), twin.solve()
    assert all(_same(p, q) for p, q in zip(first_a + second_a, first_t + second_t))  # the jvp changes nothing on the handle
    a.update(q=args[4] * 1.01)
    with pytest.raises(batch.OSQPError, match="instance 0 .*resolve"):  # the data changed since the last resolve
        a.jvp(**d)
    a.solve()
    a.warm_start(x=first_a[0])
    with pytest.raises(batch.OSQPError, match="resolve"):  # the iterate changed
        a.jvp(**d)
    a.solve()
    a.update(q=args[4][[5, 2]] * 1.02, rows=[5, 2])
    with pytest.raises(batch.OSQPError, match="instance 2 "):  # the first stale instance is named
        a.jvp(**d)
    a.solve(rows=[2])
    with pytest.raises(batch.OSQPError, match="instance 5 "):
        a.jvp(**d)
    a.solve(rows=[5])
    a.update_settings(eps_abs=1e-4)  # a setting change does not make the solution stale
    assert np.all(a.jvp(**d)["status"] == 1)
    assert lib.osqp_amd_batch_jvp_launches() == n_jvp + 3
    buf = np.zeros((len(probs), 5))
    assert lib.osqp_amd_batch_jvp(a.handle, 1, None, None, None, None, None, buf.ctypes.data, None, None, None, 0) == 1  # no tangent
    assert lib.osqp_amd_batch_jvp(a.handle, 1, buf.ctypes.data, None, None, None, None, None, None, None, None, 0) == 1  # no output
    assert lib.osqp_amd_batch_jvp(a.handle, 0, buf.ctypes.data, None, None, None, None, buf.ctypes.data, None, None, None, 0) == 1  # ndir < 1
    mpc_handle = batch.MpcBatch(lib, 4, seed=2, **OPTS)  # the other family's handle is refused
    assert lib.osqp_amd_batch_jvp(mpc_handle.handle, 1, buf.ctypes.data, None, None, None, None, buf.ctypes.data, None, None, None, 0) == 1
    mpc_handle.close()
    assert lib.osqp_amd_batch_jvp_launches() == n_jvp + 3
    assert np.all(t["status"] == 1)
    a.close(); twin.close()


@pytest.mark.parametrize("family,need", [("tiny", 7), ("ineq", 4)])
def test_end_to_end_finite_differences(product_lib, oracle_lib, family, need):
    """polish = 1: three GPU solves, at the data and at +-h d along (q, l, u), h = 1e-4 (the solution is piecewise affine in
    these, so on one active set the central difference has no truncation error); compared are the instances with three
    accepted polishes and one returned act.  Each polished x / y is within the polish tests' tolerance of the exact one, so
    every entry of the central difference is within 2 TOL / 2h of the exact derivative."""
    probs = jv.problems(oracle_lib, family)
    args = ref.stack(probs)
    count = len(probs)
    d = {k: v[0] for k, v in jv.tangents(family, 1, probs).items() if k in ("q", "l", "u")}  # tu = tl on the equality rows
    h, runs = 1e-4, []
    for s in (0.0, 1.0, -1.0):
        rb = batch.ResidentBatch(product_lib, *args[:4], args[4] + s * h * d["q"], args[5] + s * h * d["l"], args[6] + s * h * d["u"],
                                 **dict(OPTS, polish=True))
        x, y, info = rb.solve()
        runs.append(dict(x=x, y=y, pst=rb.polish_status(), t=rb.jvp(**d)))
        rb.close()
    base, used, worst = runs[0], 0, 0.0
    for i in range(count):
        if not all(r["pst"][i] == 1 and r["t"]["status"][i] == 1 and np.array_equal(r["t"]["act"][i], base["t"]["act"][i]) for r in runs):
            continue
        used += 1
        fdx, fdy = (runs[1]["x"][i] - runs[2]["x"][i]) / (2 * h), (runs[1]["y"][i] - runs[2]["y"][i]) / (2 * h)
        ex, ey = float(np.max(np.abs(fdx - base["t"]["x"][i]))), float(np.max(np.abs(fdy - base["t"]["y"][i])))
        print(f"inst {i}: max |fd - tx| {ex:.2e}  max |fd - ty| {ey:.2e}  bound {POLISH_TOL / h:.2e}")
        worst = max(worst, ex, ey)
    print(f"{family}: {used} of {count} compared, worst entry {worst:.2e} (bound {POLISH_TOL / h:.1e})")
    assert used >= need and worst <= POLISH_TOL / h


def test_torch_forward_mode(product_lib, oracle_lib):
    import torch
    from torch.autograd import forward_ad

    from osqp_jl_amd.qp_layer import BatchQPLayer

    probs = jv.problems(oracle_lib, "ineq")
    args = ref.stack(probs)
    rb = batch.ResidentBatch(product_lib, *args, **dict(OPTS, polish=True))
    layer = BatchQPLayer(rb)
    d = {k: v[0] for k, v in jv.tangents("ineq", 1, probs).items()}
    dev = torch.device("cuda:0")
    q, l = torch.tensor(args[4], device=dev), torch.tensor(args[5], device=dev)
    with forward_ad.dual_level():
        x, y = layer(q=forward_ad.make_dual(q, torch.tensor(d["q"], device=dev)), l=forward_ad.make_dual(l, torch.tensor(d["l"], device=dev)))
        px, tx = forward_ad.unpack_dual(x)
        py, ty = forward_ad.unpack_dual(y)
        want = rb.jvp(q=d["q"], l=d["l"])
        assert tx is not None and ty is not None
        assert _same(tx.cpu().numpy(), want["x"]) and _same(ty.cpu().numpy(), want["y"])
        assert np.any(want["x"] != 0.0)
    # a tensor input without a tangent counts as zero
    with forward_ad.dual_level():
        x, y = layer(q=forward_ad.make_dual(q, torch.tensor(d["q"], device=dev)), l=l)
        assert _same(forward_ad.unpack_dual(x).tangent.cpu().numpy(), rb.jvp(q=d["q"])["x"])
    # backward on the same layer: the check of the adjoint GPU test
    gx, gy = adj.incoming("ineq", rb.count, rb.n, rb.m)
    wx, wy = torch.tensor(gx, device=dev), torch.tensor(gy, device=dev)
    q2 = torch.tensor(args[4], device=dev, requires_grad=True)
    x2, y2 = layer(q=q2)
    ((wx * x2).sum() + (wy * y2).sum()).backward()
    assert _same(q2.grad.cpu().numpy(), rb.adjoint(dx=gx, dy=gy, want=("q",))["q"])
    rb.close()
