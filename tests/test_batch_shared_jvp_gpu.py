"""Forward sensitivities of the shared batch (osqp_amd_shared_batch_jvp: k_shared_jvp; `SharedBatch.jvp`, `SharedBatch.jacobian`;
forward mode of `qp_layer.SharedBatchQPLayer`) on the GPU.  Families, tangents and references: tests/batch_shared_jvp_cases.py.
The reference of the sensitivities is `batch_jvp_ref.exact` on the GPU's OWN returned x, y and act, on the Solved instances that
pass `well_conditioned` (cond K <= 1e8); at least count - 3 instances per family.

Bound of the kernel against `exact`, relative to max(1, max|exact|): 1000 times the model-vs-exact figure
tests/test_batch_shared_jvp_host.py records for the family (MEASURED_C): the kernel sums in another order.
Bound of the duality with the device adjoint, |gx . tx + gy . ty - sum_k <g_k, d_k>| / max(1, sum |terms|): 1000 times the same
quantity of the two CPU models (MEASURED_D = 1.5e-16), per well-conditioned instance and summed over the batch with the
adjoint's "Px_sum" / "Ax_sum".
FIGURES: tests 1, 2, 9 and 10 print theirs before they assert (`pytest -s`).  NOT YET RECORDED HERE: when this file was written
no MI355X could be had, so none of these tests has run on a GPU; the bounds below come from the CPU models alone:
  test 1, kernel vs exact (bound, instances the oracle's states keep): banded-17 9.2e-12 (35 of 35), banded-33-eq 1.7e-11 (35 of
  35), banded-128 5.9e-11 (35 of 35), random-129-eq 6.3e-11 (35 of 35), banded-256 2.1e-10 (10 of 11; instance 1 has cond K
  1.3e14 and is filtered), banded-240 9.9e-11 (19 of 19; T = 8);
  test 2, duality per instance and summed: 1.5e-13;
  test 9, end to end against central differences (h = 1e-5, eps 1e-10): 1e-2, at least 30 of 35 instances.
Everything else here is an equality of bits: instance i of a batch against the batch of one, a permutation, direction d of an
ndir = 3 call against a call of its own, a missing tangent against zeros, host against device form, one output against both, a
workgroup that serves several instances against the batch of one, a resolve after a JVP against one without."""
import types

import numpy as np
import pytest
import scipy.sparse as sp

from osqp_jl_amd import batch
import batch_adjoint_ref as adj
import batch_jvp_ref as jref
import batch_shared_jvp_cases as SJ
import batch_shared_cases as S
from test_batch_shared_jvp_host import MEASURED_C, MEASURED_D

pytestmark = pytest.mark.gpu

OPTS = S.OPTS
NDIR = 3
TAN = SJ.TANGENTS
_runs = {}


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _make(lib, base, q, l, u, **opts):
    P, q0, A, l0, u0 = base
    sb = batch.SharedBatch(lib, P, A, q0, l0, u0, q.shape[0], **dict(OPTS, **opts))
    sb.update(q=q, l=l if l.shape[1] else None, u=u if u.shape[1] else None)
    return sb


def _rows(t, sl):
    """The tangents `t` for the instances `sl` (a slice or an index array): the shared ones stay whole."""
    return {k: (a if k in SJ.SHARED else a[:, sl]) for k, a in t.items()}


def _run(lib, name):
    """One handle per family, once per session (left open for the tests that call it again): solve, ONE JVP with three
    directions and all five tangents, and one adjoint (one cotangent, rows and sums) for the duality test."""
    if name not in _runs:
        base, q, l, u = SJ.family(name)
        sb = _make(lib, base, q, l, u)
        x, y, info = sb.solve()
        t = SJ.tangents(name, NDIR)
        j = sb.jvp(**t)
        gx, gy = SJ.cotangents(name, 1, *q.shape, l.shape[1])
        g = sb.adjoint(dx=gx[0], dy=gy[0], sums=("Px", "Ax"))
        _runs[name] = dict(sb=sb, base=base, q=q, l=l, u=u, x=x, y=y, info=info, t=t, j=j, gx=gx[0], gy=gy[0], g=g, T=SJ.CASES[name][4])
    return _runs[name]


def _usable(r):
    P, A = r["base"][0], r["base"][2]
    return [i for i in np.flatnonzero(r["info"][:, 1] == 1) if r["j"]["status"][i] == 1 and SJ.well_conditioned(P, A, r["j"]["act"][i])]


# ---- 1. the six families against the exact sensitivities -----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SJ.CASES))
def test_kernel_agrees_with_the_exact_sensitivities(product_lib, name):
    r = _run(product_lib, name)
    P, A = r["base"][0], r["base"][2]
    j, g, info = r["j"], r["g"], r["info"]
    solved = np.flatnonzero(info[:, 1] == 1)
    used, worst = _usable(r), 0.0
    for i in used:
        want = jref.exact(P, A, r["x"][i], r["y"][i], j["act"][i], SJ.direction(r["t"], 0, i))
        worst = max(worst, jref.rel_err(j["x"][0, i], j["y"][0, i], *want))
    print(f"{name}: Solved {len(solved)} of {len(info)}, compared {len(used)}, kernel vs exact worst rel {worst:.2e} "
          f"(bound {1000 * MEASURED_C[name]:.1e})")
    assert j["x"].shape == (NDIR,) + r["q"].shape and j["y"].shape == (NDIR,) + r["l"].shape
    assert np.all(j["status"][solved] == 1)
    assert _same(j["act"], g["act"]) and _same(j["status"], g["status"])  # classified as the adjoint classifies
    assert len(used) >= len(info) - 3
    assert worst <= 1000 * MEASURED_C[name], worst


# ---- 2. duality with the device adjoint ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SJ.CASES))
def test_duality_with_the_device_adjoint(product_lib, name):
    r = _run(product_lib, name)
    j, g, t, gx, gy = r["j"], r["g"], r["t"], r["gx"], r["gy"]
    used = _usable(r)
    worst = 0.0
    for d in range(NDIR):
        for i in used:
            gap = jref.duality_gap(gx[i], gy[i], j["x"][d, i], j["y"][d, i], {k: g[k][i] for k in TAN}, SJ.direction(t, d, i))
            worst = max(worst, gap)
    print(f"{name}: duality per instance, {len(used)} instances x {NDIR} directions, worst {worst:.2e} (bound {1000 * MEASURED_D:.1e})")
    for i in sorted(set(np.flatnonzero(g["status"] == 1)) - set(used)):  # filtered (cond K > 1e8): reported, the bound is not theirs
        gap = max(jref.duality_gap(gx[i], gy[i], j["x"][d, i], j["y"][d, i], {k: g[k][i] for k in TAN}, SJ.direction(t, d, i)) for d in range(NDIR))
        print(f"{name}: instance {i} (filtered) duality {gap:.2e}")
    every = bool(np.all(g["status"] == 1))
    summed = 0.0
    if every:  # the sum over the instances: the shared values get ONE gradient and ONE tangent
        for d in range(NDIR):
            lhs = np.concatenate([(gx * j["x"][d]).ravel(), (gy * j["y"][d]).ravel()])
            rhs = np.concatenate([(g[k] * t[k][d]).ravel() for k in ("q", "l", "u")] + [g[k + "_sum"] * t[k][d] for k in SJ.SHARED])
            summed = max(summed, abs(float(lhs.sum()) - float(rhs.sum())) / max(1.0, float(np.abs(lhs).sum() + np.abs(rhs).sum())))
        print(f"{name}: duality summed over {len(gx)} instances with Px_sum / Ax_sum, worst {summed:.2e} (bound {1000 * MEASURED_D:.1e})")
    assert len(used) >= len(gx) - 3
    assert worst <= 1000 * MEASURED_D, worst
    assert summed <= 1000 * MEASURED_D, summed


# ---- 3. bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["banded-17", "random-129-eq", "banded-256", "banded-240"])
def test_bits_do_not_depend_on_the_batch_the_call_or_the_outputs(product_lib, name):
    import torch

    lib = product_lib
    r = _run(lib, name)
    sb, base, q, l, u, t, j, T = (r[k] for k in ("sb", "base", "q", "l", "u", "t", "j", "T"))
    count = q.shape[0]
    # instance i of the batch against the batch of one: first and last column of a tile, the first of the next, the last one
    for i in (0, T - 1, T, 2 * T + 2):
        one = _make(lib, base, q[i:i + 1], l[i:i + 1], u[i:i + 1])
        one.solve()
        j1 = one.jvp(**_rows(t, slice(i, i + 1)))
        one.close()
        assert _same(j1["x"], j["x"][:, i:i + 1]) and _same(j1["y"], j["y"][:, i:i + 1]), i
        assert _same(j1["act"], j["act"][i:i + 1]) and _same(j1["status"], j["status"][i:i + 1]), i
    # a permutation of the instances
    perm = np.random.default_rng(3).permutation(count)
    pb = _make(lib, base, q[perm], l[perm], u[perm])
    pb.solve()
    jp = pb.jvp(**_rows(t, perm))
    pb.close()
    assert _same(jp["x"], j["x"][:, perm]) and _same(jp["y"], j["y"][:, perm])
    assert _same(jp["act"], j["act"][perm]) and _same(jp["status"], j["status"][perm])
    # direction d of the NDIR call against a call of its own: 2-D arrays and [nnz] matrix tangents
    for d in range(NDIR):
        jd = sb.jvp(**{k: a[d] for k, a in t.items()})
        assert jd["x"].shape == q.shape and _same(jd["x"], j["x"][d]) and _same(jd["y"], j["y"][d]), d
        assert _same(jd["act"], j["act"]) and _same(jd["status"], j["status"])
    # a missing tangent is zero
    zero = {k: np.zeros_like(a) for k, a in t.items()}
    per, per0 = sb.jvp(q=t["q"], l=t["l"], u=t["u"]), sb.jvp(q=t["q"], l=t["l"], u=t["u"], Px=zero["Px"], Ax=zero["Ax"])
    mat, mat0 = sb.jvp(Px=t["Px"], Ax=t["Ax"]), sb.jvp(q=zero["q"], l=zero["l"], u=zero["u"], Px=t["Px"], Ax=t["Ax"])
    for k in ("x", "y", "act", "status"):
        assert _same(per[k], per0[k]) and _same(mat[k], mat0[k]), k
    assert np.any(per["x"]) and np.any(mat["x"]) and not _same(per["x"], j["x"])
    # host form against device form, and one output against both
    dev = torch.device("cuda", sb.device)
    dt = {k: torch.tensor(a, device=dev) for k, a in t.items()}
    empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    out = dict(x=empty(NDIR, count, sb.n), y=empty(NDIR, count, sb.m), act=empty(count, sb.m), status=empty(count, 1))
    only_x, only_y = dict(x=empty(NDIR, count, sb.n)), dict(y=empty(NDIR, count, sb.m))
    torch.cuda.synchronize()
    assert sb.jvp(**dt, out=out) is out
    sb.jvp(**dt, out=only_x)
    sb.jvp(**dt, out=only_y)
    for k in out:
        assert _same(out[k].cpu().numpy().reshape(j[k].shape), j[k]), k
    assert _same(only_x["x"].cpu().numpy(), j["x"]) and _same(only_y["y"].cpu().numpy(), j["y"])


# ---- 4. a workgroup that serves several instances ----------------------------------------------------------------------------------
def test_a_workgroup_that_serves_several_instances(product_lib):
    """`random-129-eq` keeps its factor in global scratch: W = 256 or 512 workgroups with a block each, so at count = 1027 a
    workgroup serves two to five instances one after the other -- the stride loop with its barrier at the head."""
    lib, name, count = product_lib, "random-129-eq", 1027
    r = _run(lib, name)
    base, q, l, u = SJ.family(name, count)
    t = {k: a[:2] for k, a in SJ.tangents(name, NDIR, count).items()}
    sb = _make(lib, base, q, l, u)
    x, y, info = sb.solve()
    j = sb.jvp(**t)
    sb.close()
    small = SJ.count_of(name)
    assert _same(x[:small], r["x"]) and _same(j["x"][:, :small], r["j"]["x"][:2]) and _same(j["y"][:, :small], r["j"]["y"][:2])
    assert _same(j["act"][:small], r["j"]["act"]) and _same(j["status"][:small], r["j"]["status"])
    assert np.array_equal(j["status"], (info[:, 1] == 1).astype(int)) and np.all(np.isfinite(j["x"])) and np.all(np.isfinite(j["y"]))
    for i in (256, 512, 1024, 1026):
        one = _make(lib, base, q[i:i + 1], l[i:i + 1], u[i:i + 1])
        one.solve()
        j1 = one.jvp(**_rows(t, slice(i, i + 1)))
        one.close()
        assert j1["status"][0] == 1 and np.any(j1["x"]), i
        assert _same(j1["x"], j["x"][:, i:i + 1]) and _same(j1["y"], j["y"][:, i:i + 1]), i
        assert _same(j1["act"], j["act"][i:i + 1]) and _same(j1["status"], j["status"][i:i + 1]), i


# ---- 5. statuses -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(17, 5), (130, 20)], ids=["chain-17", "chain-130"])
def test_instances_without_a_solution_get_zero_rows(product_lib, shape):
    base, q, l, u = S.chain(*shape)
    sb = _make(product_lib, base, q, l, u)
    x, y, info = sb.solve()
    rng = np.random.default_rng(61)
    (pi, _), (ai, _) = adj.patterns(base[0], base[2])
    t = dict(q=rng.standard_normal((NDIR,) + q.shape), l=rng.standard_normal((NDIR,) + l.shape), u=rng.standard_normal((NDIR,) + u.shape),
             Px=rng.standard_normal((NDIR, len(pi))), Ax=rng.standard_normal((NDIR, len(ai))))
    j = sb.jvp(**t)
    sb.close()
    assert list(info[:, 1]) == S.CHAIN_STATUS
    solved = info[:, 1] == 1
    assert np.array_equal(j["status"], solved.astype(int))
    for i in np.flatnonzero(~solved):
        assert not np.any(j["act"][i]) and not np.any(j["x"][:, i]) and not np.any(j["y"][:, i]), i  # zeros: no NaN either
    for i in np.flatnonzero(solved):
        assert np.any(j["x"][:, i]), i
    assert np.all(np.isfinite(j["x"])) and np.all(np.isfinite(j["y"]))


# ---- 6. m = 0 ----------------------------------------------------------------------------------------------------------------------
def test_a_batch_without_constraints(product_lib):
    base, q, l, u = S.unconstrained()
    sb = _make(product_lib, base, q, l, u)
    x, y, info = sb.solve()
    rng = np.random.default_rng(50)
    tq, tPx = rng.standard_normal(q.shape), rng.standard_normal(sb.nnzP)
    j = sb.jvp(q=tq, Px=tPx)
    sb.close()
    assert np.all(info[:, 1] == 1) and np.all(j["status"] == 1)
    assert sorted(j) == ["status", "x"]  # widths 0 for y and act
    Pd = adj.full_P(base[0])
    tP = jref.tangent_matrices(base[0], base[2], dict(Px=tPx))[0]
    for i in range(q.shape[0]):
        want = -np.linalg.solve(Pd, tq[i] + tP @ x[i])
        assert np.max(np.abs(j["x"][i] - want)) <= 1e-12 * max(1.0, np.max(np.abs(want))), i


# ---- 7. currency and the launch counter --------------------------------------------------------------------------------------------
def test_currency_and_the_launch_counter(product_lib):
    lib = product_lib
    base, q, l, u = SJ.family("banded-17")
    t = SJ.tangents("banded-17", NDIR)
    a, twin = _make(lib, base, q, l, u), _make(lib, base, q, l, u)
    n0 = batch.shared_jvp_launches(lib)

    def refused():
        with pytest.raises(batch.OSQPError, match="holds no current solution: call osqp_amd_shared_batch_resolve"):
            a.jvp(**t)

    refused()  # before the first resolve
    first_a, first_t = a.solve(), twin.solve()
    j = a.jvp(**t)
    assert batch.shared_jvp_launches(lib) == n0 + 1  # one per accepted call whatever ndir, none for the refused one
    a.jvp(q=t["q"][0], Px=t["Px"][0])
    assert batch.shared_jvp_launches(lib) == n0 + 2
    second_a, second_t = a.solve(), twin.solve()
    for got, want in zip(first_a + second_a, first_t + second_t):  # the JVP only reads the handle
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
    assert np.all(a.jvp(**t)["status"] == 1)  # accepted again after a resolve
    assert batch.shared_jvp_launches(lib) == n0 + 3
    tq, out = np.ascontiguousarray(t["q"][0]), np.zeros(q.shape)
    assert lib.osqp_amd_shared_batch_jvp(a.handle, 1, None, None, None, None, None, out.ctypes.data, None, None, None, 0) == 1  # no tangent
    assert b"need a tangent" in lib.osqp_amd_last_error()
    assert lib.osqp_amd_shared_batch_jvp(a.handle, 0, tq.ctypes.data, None, None, None, None, out.ctypes.data, None, None, None, 0) == 1  # ndir = 0
    assert b"ndir >= 1" in lib.osqp_amd_last_error()
    assert batch.shared_jvp_launches(lib) == n0 + 3 and not np.any(out)  # nothing written
    assert np.all(j["status"] == 1)
    a.close(); twin.close()


# ---- 8. the factor blocks are the adjoint's ----------------------------------------------------------------------------------------
def test_jvp_and_adjoint_share_the_factor_blocks(product_lib):
    import torch

    lib = product_lib
    base, q, l, u = SJ.family("banded-256")
    t = SJ.tangents("banded-256", 1)
    gx, gy = SJ.cotangents("banded-256", 1, *q.shape, l.shape[1])
    dev = torch.device("cuda:0")
    dt = {k: torch.tensor(a[0], device=dev) for k, a in t.items()}
    dgx, dgy = torch.tensor(gx[0], device=dev), torch.tensor(gy[0], device=dev)
    empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    count, n, m = q.shape[0], q.shape[1], l.shape[1]
    torch.cuda.synchronize()
    grown = []
    for jvp_first in (False, True):
        sb = _make(lib, base, q, l, u)
        sb.solve()
        sizes = [sb.device_bytes()]
        for is_jvp in (jvp_first, not jvp_first):  # device arrays: no staging buffer grows
            if is_jvp:
                sb.jvp(**dt, out=dict(x=empty(count, n), y=empty(count, m)))
            else:
                sb.adjoint(dx=dgx, dy=dgy, want=("q",), out=dict(q=empty(count, n)))
            sizes.append(sb.device_bytes())
        sb.close()
        print(f"device bytes (JVP first: {jvp_first}): after the solve {sizes[0]}, after the first call {sizes[1]}, after the second {sizes[2]}")
        assert sizes[2] == sizes[1]  # no second set of factor blocks, whichever call came first
        grown.append(sizes[1] - sizes[0])
    assert grown[0] == grown[1] and grown[0] in (256 * n * n * 8, 512 * n * n * 8)  # W blocks of n x n doubles, W from the shape alone


# ---- 9. end to end against finite differences --------------------------------------------------------------------------------------
def test_end_to_end_finite_differences(product_lib):
    """One direction with all five tangents, tu = tl, h = 1e-5: three handles -- a new model is a new handle -- on the base and on
    (P +- h tP, A +- h tA), each with q, l, u +- h t, solved to eps 1e-10.  Compared are the instances that are Solved in all
    three with one act; the central difference then carries O(h^2) of truncation and 1e-10 / 1e-5 of the solves' error."""
    lib, name, h = product_lib, "banded-17", 1e-5
    base, q, l, u = SJ.family(name)
    t = {k: a[0] for k, a in SJ.tangents(name, 1).items()}
    t["u"] = t["l"]
    P0, q0, A0, l0, u0 = base
    Pu = sp.csc_matrix(sp.triu(P0)); Pu.sort_indices()
    Ac = sp.csc_matrix(A0); Ac.sort_indices()
    runs = []
    for s in (0.0, 1.0, -1.0):
        Ps, As = Pu.copy(), Ac.copy()
        Ps.data, As.data = Pu.data + s * h * t["Px"], Ac.data + s * h * t["Ax"]
        sb = _make(lib, (Ps, q0, As, l0, u0), q + s * h * t["q"], l + s * h * t["l"], u + s * h * t["u"], eps_abs=1e-10, eps_rel=1e-10,
                   max_iter=50000)
        x, y, info = sb.solve()
        runs.append(dict(x=x, y=y, info=info, j=sb.jvp(**t)))
        sb.close()
    mid, used, worst = runs[0], 0, 0.0
    for i in range(q.shape[0]):
        if not all(r["info"][i, 1] == 1 and r["j"]["status"][i] == 1 and np.array_equal(r["j"]["act"][i], mid["j"]["act"][i]) for r in runs):
            continue
        used += 1
        fdx, fdy = (runs[1]["x"][i] - runs[2]["x"][i]) / (2 * h), (runs[1]["y"][i] - runs[2]["y"][i]) / (2 * h)
        worst = max(worst, jref.rel_err(fdx, fdy, mid["j"]["x"][i], mid["j"]["y"][i]))
    print(f"{name}: {used} of {q.shape[0]} compared, central difference vs JVP worst rel {worst:.2e} (bound 1e-2), "
          f"most iterations {int(max(r['info'][:, 0].max() for r in runs))}")
    assert used >= 30
    assert worst <= 1e-2, worst


# ---- 10. Jacobians -----------------------------------------------------------------------------------------------------------------
def test_jacobian(product_lib):
    lib, name = product_lib, "banded-17"
    r = _run(lib, name)
    sb, count = r["sb"], r["q"].shape[0]
    bound = 1000 * MEASURED_C[name]
    for o, w in (("x", "q"), ("x", "Px"), ("y", "Ax")):
        fwd = sb.jacobian(of=(o,), wrt=(w,), mode="forward")
        rev = sb.jacobian(of=(o,), wrt=(w,), mode="reverse", chunk=5)
        cols_o, cols_w = dict(x=sb.n, y=sb.m)[o], dict(q=sb.n, Px=sb.nnzP, Ax=sb.nnzA)[w]
        assert fwd[(o, w)].shape == rev[(o, w)].shape == (count, cols_o, cols_w)
        assert _same(fwd["act"], r["j"]["act"]) and _same(fwd["status"], r["j"]["status"]) and _same(rev["status"], fwd["status"])
        for b in (0, cols_w // 2, cols_w - 1):  # column b: the unit direction b, applied to every instance at once
            unit = np.zeros((count, cols_w) if w == "q" else (cols_w,))
            unit[..., b] = 1.0
            assert _same(fwd[(o, w)][:, :, b], sb.jvp(**{w: unit})[o]), (o, w, b)
        assert _same(fwd[(o, w)], sb.jacobian(of=(o,), wrt=(w,), mode="forward", chunk=4)[(o, w)])  # the chunks are independent
        gap = float(np.max(np.abs(fwd[(o, w)] - rev[(o, w)]))) / max(1.0, float(np.max(np.abs(rev[(o, w)]))))
        print(f"{name}: d{o}/d{w} forward vs reverse {gap:.2e} (bound {bound:.1e})")
        assert np.any(fwd[(o, w)]) and gap <= bound, (o, w, gap)
    # "auto": the mode with fewer solves per instance (reverse on a tie) -- told by the call that was made
    def calls(**kw):
        n0 = (batch.shared_jvp_launches(lib), batch.shared_adjoint_launches(lib))
        J = sb.jacobian(**kw)
        return J, (batch.shared_jvp_launches(lib) - n0[0], batch.shared_adjoint_launches(lib) - n0[1])

    J, made = calls(of=("x", "y"), wrt=("q",))  # n + m output components, n columns: forward
    assert made == (1, 0) and _same(J[("y", "q")], sb.jacobian(of=("x", "y"), wrt=("q",), mode="forward")[("y", "q")])
    J, made = calls(of=("x",), wrt=("Px",))  # n output components, nnzP > n columns: reverse
    assert sb.nnzP > sb.n and made == (0, 1) and _same(J[("x", "Px")], sb.jacobian(of=("x",), wrt=("Px",), mode="reverse")[("x", "Px")])
    J, made = calls(of=("x",), wrt=("q",))  # a tie: reverse
    assert made == (0, 1)


# ---- 11. the torch layer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["banded-33-eq", "random-129-eq"])
def test_torch_forward_mode(product_lib, name):
    import torch
    from torch.autograd import forward_ad

    from osqp_jl_amd.qp_layer import SharedBatchQPFunction, SharedBatchQPLayer

    lib = product_lib
    base, q, l, u = SJ.family(name)
    sb = _make(lib, base, q, l, u)
    layer = SharedBatchQPLayer(sb)
    t = {k: a[0] for k, a in SJ.tangents(name, 1).items()}
    dev = torch.device("cuda:0")
    qt = torch.tensor(q, device=dev, requires_grad=True)
    Pxp = torch.nn.Parameter(layer.Px.clone())
    n0 = batch.shared_jvp_launches(lib)
    with forward_ad.dual_level():
        x, y = layer(q=forward_ad.make_dual(qt, torch.tensor(t["q"], device=dev)), Px=forward_ad.make_dual(Pxp, torch.tensor(t["Px"], device=dev)))
        px, tx = forward_ad.unpack_dual(x)
        py, ty = forward_ad.unpack_dual(y)
        assert batch.shared_jvp_launches(lib) == n0 + 1  # ONE call for the whole batch
        want = sb.jvp(q=t["q"], Px=t["Px"])
        assert np.all(want["status"] == 1) and np.any(want["x"])
        assert _same(tx.cpu().numpy(), want["x"]) and _same(ty.cpu().numpy(), want["y"])
        # backward still works on the same forward
        (px.sum() + py.sum()).backward()
    g = sb.adjoint(dx=np.ones(q.shape), dy=np.ones(l.shape), want=("q",), sums=("Px",))
    assert _same(qt.grad.cpu().numpy(), g["q"]) and _same(Pxp.grad.cpu().numpy(), g["Px_sum"])
    # the handle holds one solution: the tangents of a forward that a later one has replaced are refused
    ctx = types.SimpleNamespace(sb=sb, stamp=sb._qp_layer_served, given=("q",))
    layer(q=qt.detach())
    with pytest.raises(RuntimeError, match="solved again"):
        SharedBatchQPFunction.jvp(ctx, None, torch.tensor(t["q"], device=dev), None, None, None, None)
    sb.close()
