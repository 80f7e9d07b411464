"""Adjoint derivatives of the shared batch (osqp_amd_shared_batch_adjoint: k_shared_adjoint, k_shared_reduce_rows;
`SharedBatch.adjoint`; `qp_layer.SharedBatchQPLayer`) on the GPU.  Families, filters and the reference of the sums:
tests/batch_shared_adjoint_cases.py.  The reference of the gradients is `batch_adjoint_ref.exact` on the GPU's OWN returned x, y
and act, on the Solved instances that pass `well_conditioned` (cond K <= 1e8); at least count - 3 instances per family.

Bound of the kernel against `exact`, relative to max(1, max|exact|) per gradient: 1000 times the model-vs-exact figure
tests/test_batch_shared_adjoint_host.py records for the family (MEASURED_C): the kernel sums in another order.
FIGURES of the first test on an MI355X (kernel vs exact, instances compared; bound):
  banded-17      5.8e-15   35 of 35   (4.4e-12)
  banded-33-eq   7.5e-15   35 of 35   (7.5e-12)
  banded-128     6.0e-14   35 of 35   (6.1e-11)
  random-129-eq  5.7e-14   35 of 35   (5.4e-11)
  banded-256     2.2e-13   10 of 11   (2.1e-10; instance 1 has cond K 1.3e14 and is filtered)
  banded-240     8.4e-14   19 of 19   (9.0e-11; T = 8)
Everything else here is an equality of bits: instance i of a batch against the batch of one, a permutation, cotangent c of an
ncot = 3 call against a call of its own, host against device form, any `want` / `sums` against any other, the sums against the
numpy loop in the order of the contract, a resolve after an adjoint against one without."""
import numpy as np
import pytest

from osqp_jl_amd import batch
import batch_adjoint_ref as adj
import batch_shared_adjoint_cases as SA
import batch_shared_cases as S
from test_batch_shared_adjoint_host import MEASURED_C

pytestmark = pytest.mark.gpu

OPTS = S.OPTS
NCOT = 3
GRADS = ("q", "l", "u", "Px", "Ax")
SUMS = ("Px_sum", "Ax_sum")
_runs = {}


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _make(lib, base, q, l, u, **opts):
    P, q0, A, l0, u0 = base
    sb = batch.SharedBatch(lib, P, A, q0, l0, u0, q.shape[0], **dict(OPTS, **opts))
    sb.update(q=q, l=l if l.shape[1] else None, u=u if u.shape[1] else None)
    return sb


def _run(lib, name):
    """One handle per family, once per session (left open for the tests that call it again): solve, then ONE adjoint with three
    cotangents, every gradient and both sums."""
    if name not in _runs:
        base, q, l, u = SA.family(name)
        sb = _make(lib, base, q, l, u)
        x, y, info = sb.solve()
        gx, gy = SA.cotangents(name, NCOT, *q.shape, l.shape[1])
        g = sb.adjoint(dx=gx, dy=gy, sums=("Px", "Ax"))
        _runs[name] = dict(sb=sb, base=base, q=q, l=l, u=u, x=x, y=y, info=info, gx=gx, gy=gy, g=g, T=SA.CASES[name][4])
    return _runs[name]


# ---- 1. the five families against the exact adjoint ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SA.CASES))
def test_kernel_agrees_with_the_exact_adjoint(product_lib, name):
    r = _run(product_lib, name)
    P, A = r["base"][0], r["base"][2]
    g, info = r["g"], r["info"]
    solved = np.flatnonzero(info[:, 1] == 1)
    worst, used = 0.0, []
    for i in solved:
        if g["status"][i] != 1 or not SA.well_conditioned(P, A, g["act"][i]):
            continue
        want = adj.exact(P, A, r["x"][i], r["y"][i], g["act"][i], r["gx"][0, i], r["gy"][0, i])
        worst = max(worst, adj.rel_err({k: g[k][0, i] for k in GRADS}, want))
        used.append(i)
    print(f"{name}: Solved {len(solved)} of {len(info)}, compared {len(used)}, kernel vs exact worst rel {worst:.2e} "
          f"(bound {1000 * MEASURED_C[name]:.1e})")
    assert np.all(g["status"][solved] == 1)
    assert len(used) >= len(info) - 3
    assert worst <= 1000 * MEASURED_C[name], worst


# ---- 2. bits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["banded-17", "random-129-eq", "banded-256", "banded-240"])
def test_bits_do_not_depend_on_the_batch_the_call_or_the_outputs(product_lib, name):
    lib = product_lib
    r = _run(lib, name)
    sb, base, q, l, u, gx, gy, g, T = (r[k] for k in ("sb", "base", "q", "l", "u", "gx", "gy", "g", "T"))
    count = q.shape[0]
    # instance i of the batch against the batch of one: first and last column of a tile, the first of the next, the last one
    for i in (0, T - 1, T, 2 * T + 2):
        one = _make(lib, base, q[i:i + 1], l[i:i + 1], u[i:i + 1])
        one.solve()
        g1 = one.adjoint(dx=gx[:, i:i + 1], dy=gy[:, i:i + 1], sums=("Px", "Ax"))
        one.close()
        for k in GRADS:
            assert _same(g1[k], g[k][:, i:i + 1]), (i, k)
        assert _same(g1["act"], g["act"][i:i + 1]) and _same(g1["status"], g["status"][i:i + 1])
        assert _same(g1["Px_sum"], g["Px"][:, i]) and _same(g1["Ax_sum"], g["Ax"][:, i])  # the sum of one row is that row
    # a permutation of the instances
    perm = np.random.default_rng(3).permutation(count)
    pb = _make(lib, base, q[perm], l[perm], u[perm])
    pb.solve()
    gp = pb.adjoint(dx=gx[:, perm], dy=gy[:, perm])
    pb.close()
    for k in GRADS:
        assert _same(gp[k], g[k][:, perm]), k
    assert _same(gp["act"], g["act"][perm]) and _same(gp["status"], g["status"][perm])
    # cotangent c of the ncot = 3 call against a call of its own (2-D arrays: the plain entry of one cotangent)
    for c in range(NCOT):
        gc = sb.adjoint(dx=gx[c], dy=gy[c], sums=("Px", "Ax"))
        for k in GRADS + SUMS:
            assert _same(gc[k], g[k][c]), (c, k)
    # host form against device form (one cotangent, DeviceArray is two-dimensional)
    host = sb.adjoint(dx=gx[0], dy=gy[0], sums=("Px", "Ax"))
    cols = dict(q=sb.n, l=sb.m, u=sb.m, Px=sb.nnzP, Ax=sb.nnzA, act=sb.m, status=1)
    dev = {k: batch.DeviceArray(lib, count, c) for k, c in cols.items()}
    dev.update(Px_sum=batch.DeviceArray(lib, 1, sb.nnzP), Ax_sum=batch.DeviceArray(lib, 1, sb.nnzA))
    dgx, dgy = (batch.DeviceArray(lib, *a.shape).upload(a) for a in (gx[0], gy[0]))
    assert sb.adjoint(dx=dgx, dy=dgy, sums=("Px", "Ax"), out=dev) is dev
    for k in dev:
        assert _same(dev[k].numpy().reshape(host[k].shape), host[k]), k
    for d in list(dev.values()) + [dgx, dgy]:
        d.free()
    # every output is independent of what else was asked for
    for want, sums in ((("l", "Ax"), ()), ((), ("Ax",)), (("Px",), ("Px",)), (("q",), ("Px", "Ax")), ((), ())):
        part = sb.adjoint(dx=gx, dy=gy, want=want, sums=sums)
        assert sorted(part) == sorted(want + tuple(s + "_sum" for s in sums) + ("act", "status"))
        assert all(_same(part[k], g[k]) for k in part), (want, sums)
    # a missing cotangent is zero
    only_x, zero_y = sb.adjoint(dx=gx, sums=("Px", "Ax")), sb.adjoint(dx=gx, dy=np.zeros_like(gy), sums=("Px", "Ax"))
    only_y, zero_x = sb.adjoint(dy=gy, sums=("Px", "Ax")), sb.adjoint(dx=np.zeros_like(gx), dy=gy, sums=("Px", "Ax"))
    for k in GRADS + SUMS + ("act", "status"):
        assert _same(only_x[k], zero_y[k]) and _same(only_y[k], zero_x[k]), k


# ---- 3. the summed matrix gradients ----------------------------------------------------------------------------------------------
def _check_sums(g, only):
    for c in range(NCOT):
        for k in ("Px", "Ax"):
            want = SA.block_sum(g[k][c])
            assert _same(g[k + "_sum"][c], want), (c, k)
            assert _same(only[k + "_sum"][c], want), (c, k, "rows not requested")


@pytest.mark.parametrize("name,count", [("banded-17", 1), ("banded-17", 16), ("banded-17", 17), ("banded-17", 35), ("banded-256", 11)])
def test_sums_have_the_bits_of_the_block_of_16_loop(product_lib, name, count):
    if count == SA.count_of(name):
        r = _run(product_lib, name)
        sb, gx, gy, g = r["sb"], r["gx"], r["gy"], r["g"]
    else:
        base, q, l, u = SA.family(name, count)
        sb = _make(product_lib, base, q, l, u)
        sb.solve()
        gx, gy = SA.cotangents(name, NCOT, *q.shape, l.shape[1])
        g = sb.adjoint(dx=gx, dy=gy, sums=("Px", "Ax"))
    only = sb.adjoint(dx=gx, dy=gy, want=(), sums=("Px", "Ax"))
    assert np.all(g["status"] == 1) and all(np.any(g[k]) for k in SUMS)
    _check_sums(g, only)
    if count != SA.count_of(name):
        sb.close()


def test_sums_through_a_row_scratch_of_several_chunks(product_lib):
    """Enough cotangents on `banded-17` that the rows of 35 instances exceed the handle's row scratch (64 MiB): the call that
    wants the sums alone then runs chunk by chunk (16, 16 and 3 instances) and must give the bits of the call whose rows stay
    in its own arrays."""
    r = _run(product_lib, "banded-17")
    sb, count = r["sb"], r["q"].shape[0]
    ncot = (64 << 20) // (8 * 32 * (sb.nnzP + sb.nnzA)) + 1  # more than 1 / 32 of the scratch per instance: chunks of 16
    rng = np.random.default_rng(4)
    gx = np.tile(r["gx"], (ncot // NCOT + 1, 1, 1))[:ncot] * (1.0 + rng.random((ncot, 1, 1)))
    rows = sb.adjoint(dx=gx, want=("Px", "Ax"), sums=("Px", "Ax"))
    only = sb.adjoint(dx=gx, want=(), sums=("Px", "Ax"))
    for k in ("Px", "Ax"):
        assert _same(only[k + "_sum"], rows[k + "_sum"]), k
        for c in (0, 1, ncot - 1):
            assert _same(rows[k + "_sum"][c], SA.block_sum(rows[k][c])), (k, c)
    assert count == 35 and ncot * (sb.nnzP + sb.nnzA) * 8 * 32 > (64 << 20)


# ---- 4. statuses -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(17, 5), (130, 20)], ids=["chain-17", "chain-130"])
def test_instances_without_a_solution_get_zero_rows(product_lib, shape):
    base, q, l, u = S.chain(*shape)
    sb = _make(product_lib, base, q, l, u)
    x, y, info = sb.solve()
    gx, gy = SA.cotangents("chain", NCOT, *q.shape, l.shape[1])
    g = sb.adjoint(dx=gx, dy=gy, sums=("Px", "Ax"))
    sb.close()
    assert list(info[:, 1]) == S.CHAIN_STATUS
    solved = info[:, 1] == 1
    assert np.array_equal(g["status"], solved.astype(int))
    for i in np.flatnonzero(~solved):
        assert not np.any(g["act"][i]) and all(not np.any(g[k][:, i]) for k in GRADS), i  # zeros: no NaN either
    assert all(np.all(np.isfinite(g[k])) for k in GRADS + SUMS)
    for c in range(NCOT):
        for k in ("Px", "Ax"):
            assert np.any(g[k + "_sum"][c])
            assert _same(g[k + "_sum"][c], SA.block_sum(g[k][c]))
            assert _same(g[k + "_sum"][c], SA.block_sum(g[k][c][solved]))  # the sum over the Solved ones: zero rows add nothing


def test_a_batch_without_constraints(product_lib):
    base, q, l, u = S.unconstrained()
    sb = _make(product_lib, base, q, l, u)
    x, y, info = sb.solve()
    gx = np.random.default_rng(50).standard_normal(q.shape)
    g = sb.adjoint(dx=gx, sums=("Px", "Ax"))
    sb.close()
    assert np.all(info[:, 1] == 1) and np.all(g["status"] == 1)
    assert sorted(g) == ["Px", "Px_sum", "q", "status"]  # widths 0 for l, u, Ax, act
    Pd = adj.full_P(base[0])
    for i in range(q.shape[0]):
        want = -np.linalg.solve(Pd, gx[i])
        assert np.max(np.abs(g["q"][i] - want)) <= 1e-12 * max(1.0, np.max(np.abs(want))), i
    assert _same(g["Px_sum"], SA.block_sum(g["Px"]))


# ---- 5. currency, 6. the launch counter ------------------------------------------------------------------------------------------
def test_currency_and_the_launch_counter(product_lib):
    lib = product_lib
    base, q, l, u = SA.family("banded-17")
    gx, gy = SA.cotangents("banded-17", NCOT, *q.shape, l.shape[1])
    a, twin = _make(lib, base, q, l, u), _make(lib, base, q, l, u)
    n0 = batch.shared_adjoint_launches(lib)

    def refused():
        with pytest.raises(batch.OSQPError, match="holds no current solution: call osqp_amd_shared_batch_resolve"):
            a.adjoint(dx=gx, dy=gy)

    refused()  # before the first resolve
    first_a, first_t = a.solve(), twin.solve()
    g = a.adjoint(dx=gx, dy=gy, sums=("Px", "Ax"))
    assert batch.shared_adjoint_launches(lib) == n0 + 1  # one per accepted call whatever ncot, none for the refused one
    a.adjoint(dx=gx[0], dy=gy[0])
    assert batch.shared_adjoint_launches(lib) == n0 + 2
    second_a, second_t = a.solve(), twin.solve()
    for got, want in zip(first_a + second_a, first_t + second_t):  # the adjoint only reads the handle
        assert _same(got, want)
    a.update(q=q * 1.01)
    refused()
    a.solve()
    a.update(l=l - 0.01, u=u + 0.01)
    refused()
    a.solve()
    a.warm_start(x=first_a[0])
    refused()
    a.solve()
    a.update_settings(rho=0.5)
    refused()
    a.solve()
    assert np.all(a.adjoint(dx=gx, dy=gy)["status"] == 1)  # accepted again after a resolve
    assert batch.shared_adjoint_launches(lib) == n0 + 3
    buf = np.zeros((q.shape[0], q.shape[1]))
    assert lib.osqp_amd_shared_batch_adjoint(a.handle, 1, None, None, buf.ctypes.data, *([None] * 8), 0) == 1  # neither dx nor dy
    assert lib.osqp_amd_shared_batch_adjoint(a.handle, 0, buf.ctypes.data, None, buf.ctypes.data, *([None] * 8), 0) == 1  # ncot = 0
    assert batch.shared_adjoint_launches(lib) == n0 + 3
    assert np.all(g["status"] == 1)
    a.close(); twin.close()


# ---- 7. the factor scratch is not per instance -----------------------------------------------------------------------------------
def test_device_bytes_do_not_grow_with_count_times_n_squared(product_lib):
    r = _run(product_lib, "banded-256")
    small = r["sb"].device_bytes()  # count 11, after adjoint calls
    base, q, l, u = SA.family("banded-256", 64)
    sb = _make(product_lib, base, q, l, u)
    before = sb.device_bytes()
    sb.solve()
    gx, gy = SA.cotangents("banded-256", 1, *q.shape, l.shape[1])
    assert np.sum(sb.adjoint(dx=gx[0], dy=gy[0], sums=("Px", "Ax"))["status"] == 1) >= 60
    large = sb.device_bytes()
    sb.close()
    n = q.shape[1]
    print(f"device bytes: count 11 {small}, count 64 {large} (before its first adjoint {before}); 53 n^2 8 = {53 * n * n * 8}")
    assert large > before  # the factor blocks are allocated at first use and counted
    assert abs(large - small) < 53 * n * n * 8


# ---- 8. the torch layer ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["banded-33-eq", "random-129-eq"])
def test_torch_layer(product_lib, name):
    import torch

    from osqp_jl_amd.qp_layer import SharedBatchQPLayer

    lib = product_lib
    base, q, l, u = SA.family(name)
    sb = _make(lib, base, q, l, u)
    layer = SharedBatchQPLayer(sb)
    gx, gy = SA.cotangents(name, NCOT, *q.shape, l.shape[1])
    dev = torch.device("cuda:0")
    w, v = torch.tensor(gx[0], device=dev), torch.tensor(gy[0], device=dev)
    t = {k: torch.tensor(a, device=dev, requires_grad=True) for k, a in (("q", q), ("l", l), ("u", u))}
    t["Px"], t["Ax"] = layer.Px.clone().requires_grad_(True), layer.Ax.clone().requires_grad_(True)
    x, y = layer(**t)
    assert tuple(layer.info.shape) == (sb.count, 6) and bool((layer.info[:, 1] == 1).all())
    ((w * x).sum() + (v * y).sum()).backward()
    want = sb.adjoint(dx=gx[0], dy=gy[0], sums=("Px", "Ax"))
    for k in ("q", "l", "u"):
        assert _same(t[k].grad.cpu().numpy(), want[k]), k
    for k in ("Px", "Ax"):
        assert tuple(t[k].grad.shape) == (len(want[k + "_sum"]),) and _same(t[k].grad.cpu().numpy(), want[k + "_sum"]), k
    # vmap of the pull-back over three cotangents: one adjoint call
    qv = torch.tensor(q, device=dev, requires_grad=True)
    xs, vjp_fn = torch.func.vjp(lambda qq: layer(q=qq)[0], qv)
    G = torch.tensor(gx, device=dev)
    n0 = batch.shared_adjoint_launches(lib)
    (dq,) = torch.func.vmap(vjp_fn)(G)
    assert batch.shared_adjoint_launches(lib) == n0 + 1
    assert _same(dq.cpu().numpy(), sb.adjoint(dx=gx, want=("q",))["q"])
    # the shared values are the handle's own: anything else is a new model
    bad = layer.Px.clone()
    bad[0] = torch.nextafter(bad[0], bad[0] + 1.0)  # one ulp
    with pytest.raises(ValueError, match="a new model is a new handle"):
        layer(q=t["q"], Px=bad)
    # the handle holds one solution: the first graph's backward after a second forward raises
    q3 = torch.tensor(q, device=dev, requires_grad=True)
    x3, _ = layer(q=q3)
    layer(q=qv)
    with pytest.raises(RuntimeError, match="solved again"):
        x3.sum().backward()
    sb.close()
