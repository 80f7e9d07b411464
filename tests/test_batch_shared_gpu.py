"""The shared batch (batch.SharedBatch: one model, many right-hand sides on one KKT inverse; k_batch_solve_shared) on the GPU.
The families and the reference -- one oracle model per instance, set up on the base data and then updated -- are
tests/batch_shared_cases.py; tests/test_batch_shared_host.py holds them to what these tests rest on.  Comparison with the
reference is `batch_resident_ref.compare`: status equal, iteration count within one check, Solved solutions within
50 max(eps_abs, 1e-7) relative to max(1, |ref|), NaN rows where the reference has no solution."""
import numpy as np
import pytest

import osqp_jl_amd as oq
from osqp_jl_amd import batch
import batch_entry_families as F
import batch_resident_ref as ref
import batch_shared_cases as S

pytestmark = pytest.mark.gpu

OPTS = S.OPTS
SHARED_KERNEL = -3


def _same(a, b):
    return all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


def _make(lib, base, count, **opts):
    P, q0, A, l0, u0 = base
    return batch.SharedBatch(lib, P, A, q0, l0, u0, count, **opts)


def _solve(lib, base, q, l, u, **opts):
    sb = _make(lib, base, q.shape[0], **opts)
    sb.update(q=q, l=l if l.shape[1] else None, u=u if u.shape[1] else None)
    out = sb.solve()
    sb.close()
    return out


def _family(name, count=None):
    return S.unconstrained(count=5 if count is None else count) if name == "m0" else S.boxed(name, count)


# ---- 1. shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("many", [False, True], ids=["one", "2T+3"])
@pytest.mark.parametrize("name", list(S.BOXED) + ["m0"])
def test_shape(product_lib, oracle_lib, name, many):
    lib = product_lib
    base = _family(name, 1)[0]
    T = batch.shared_plan(lib, base[0], base[2])["T"]
    count = 2 * T + 3 if many else 1
    base, q, l, u = _family(name, count)
    refs = S.reference(oracle_lib, ("shape", name, count), base, q, l, u, **OPTS)
    sb = _make(lib, base, count, **OPTS)
    sb.update(q=q, l=l if l.shape[1] else None, u=u if u.shape[1] else None)
    before = batch.shared_launches(lib)
    x, y, info = sb.solve()
    assert batch.shared_launches(lib) == before + 1  # one launch per resolve
    assert lib.osqp_amd_batch_last_kernel() == SHARED_KERNEL
    sb.close()
    ref.compare(x, y, info, refs, OPTS, tag=f"{name} T={T}")
    assert np.all(info[:, 5] == 0)
    assert _same((x, y, info), _solve(lib, base, q, l, u, **OPTS))  # two identical handles: identical bits


# ---- 2. independence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["banded-17", "banded-129-eq", "banded-256"])
def test_instance_bits_do_not_depend_on_the_batch(product_lib, name):
    lib = product_lib
    base = S.boxed(name, 1)[0]
    T = batch.shared_plan(lib, base[0], base[2])["T"]
    count = 2 * T + 3
    base, q, l, u = S.boxed(name, count)
    x, y, info = _solve(lib, base, q, l, u, **OPTS)
    assert len(set(info[:T, 0])) > 1  # different stop iterations inside the first tile
    for i in (0, T - 1, T, 2 * T + 2):  # first and last column of a full tile, the first of the next, the last of the partial tile
        one = _solve(lib, base, q[i:i + 1], l[i:i + 1], u[i:i + 1], **OPTS)
        assert _same(one, (x[i:i + 1], y[i:i + 1], info[i:i + 1])), i
    perm = np.random.default_rng(3).permutation(count)
    xp, yp, ip = _solve(lib, base, q[perm], l[perm], u[perm], **OPTS)
    assert _same((xp, yp, ip), (x[perm], y[perm], info[perm]))


# ---- 3. masking and statuses -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [dict(), dict(max_iter=30), dict(scaling=0), dict(scaled_termination=1)],
                         ids=["default", "max_iter30", "unscaled", "scaled_termination"])
@pytest.mark.parametrize("shape", S.CHAINS, ids=lambda s: "chain-%d" % s[0])
def test_chain_statuses(product_lib, oracle_lib, shape, variant):
    """Nine instances in one batch -- solvable, primal infeasible, dual infeasible in turn -- each with its oracle's status and
    its own stop iteration in info column 0."""
    opts = dict(OPTS, **variant)
    base, q, l, u = S.chain(*shape)
    refs = S.reference(oracle_lib, ("chain-gpu", shape, tuple(sorted(variant.items()))), base, q, l, u, **opts)
    x, y, info = _solve(product_lib, base, q, l, u, **opts)
    ref.compare(x, y, info, refs, opts, tag=f"chain {shape} {variant}")
    if not variant:
        assert [int(s) for s in info[:, 1]] == S.CHAIN_STATUS
    if variant == dict(max_iter=30) and shape == S.CHAINS[0]:
        assert [int(s) for s in info[:, 1]] == S.CHAIN_STATUS_30
    assert len(set(info[:, 0])) > 1
    for k, r in enumerate(refs):
        if r.info.status_val in (-3, -4, 3, 4):
            assert np.all(np.isnan(y[k]))


# ---- 4. life cycle -----------------------------------------------------------------------------------------------------------
def _life_cycle(lib, oracle_lib, name, device, **opts):
    base, q, l, u = S.boxed(name)
    count = q.shape[0]
    sb = _make(lib, base, count, **opts)
    ob = S.OracleShared(oracle_lib, base, count, **opts)
    up = (lambda a: batch.DeviceArray(lib, *a.shape).upload(a)) if device else (lambda a: a)
    outs = []

    def solve(tag):
        if device:
            out = sb.alloc()
            sb.solve(out=out)
            got = tuple(o.numpy() for o in out)
        else:
            got = sb.solve()
        ref.compare(*got, ob.solve(), opts, tag=f"{name} {tag}")
        outs.append(got)
        return got

    solve("base")  # every instance holds (q0, l0, u0)
    sb.update(q=up(q), l=up(l), u=up(u)); ob.update(q=q, l=l, u=u)
    x1, y1, _ = solve("updated")
    q2, l2, u2 = S.perturbed(l, u, q)
    sb.update(q=up(q2), l=up(l2), u=up(u2)); ob.update(q=q2, l=l2, u=u2)
    solve("perturbed, re-solved")
    sb.warm_start(x=up(x1), y=up(y1)); ob.warm_start(x=x1, y=y1)
    solve("warm-started")
    sb.close(); ob.close()
    return outs


@pytest.mark.parametrize("warm", [1, 0], ids=["warm", "cold"])
@pytest.mark.parametrize("name", ["banded-33-eq", "banded-129-eq"])
def test_life_cycle(product_lib, oracle_lib, name, warm):
    opts = dict(OPTS, warm_start=bool(warm))
    host = _life_cycle(product_lib, oracle_lib, name, False, **opts)
    dev = _life_cycle(product_lib, oracle_lib, name, True, **opts)
    for a, b in zip(host, dev):
        assert _same(a, b)  # host arrays and device arrays: the same bits


# ---- 5. rho update -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["banded-17", "banded-129-eq"])
def test_rho_update(product_lib, oracle_lib, name):
    base, q, l, u = S.boxed(name)
    sb = _make(product_lib, base, q.shape[0], **OPTS)
    ob = S.OracleShared(oracle_lib, base, q.shape[0], **OPTS)
    sb.update(q=q, l=l, u=u); ob.update(q=q, l=l, u=u)
    ref.compare(*sb.solve(), ob.solve(), OPTS, tag=f"{name} rho 1.0")
    sb.update_settings(rho=0.3); ob.update_settings(rho=0.3)
    q2, l2, u2 = S.perturbed(l, u, q)
    sb.update(q=q2, l=l2, u=u2); ob.update(q=q2, l=l2, u=u2)
    ref.compare(*sb.solve(), ob.solve(), OPTS, tag=f"{name} rho 0.3")
    sb.close(); ob.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_setup_refusals(product_lib):
    base = S.boxed("banded-17", 1)[0]
    with pytest.raises(oq.OSQPError, match="adaptive_rho"):
        _make(product_lib, base, 3, **dict(OPTS, adaptive_rho=1))
    P, A = F.pattern("banded", (257, 300, 3))
    _, probs = F.instances((P, A), 1, 1)
    Pb, qb, Ab, lb, ub = probs[0]
    with pytest.raises(oq.OSQPError, match="n <= 256"):
        batch.SharedBatch(product_lib, Pb, Ab, qb, lb, ub, 3, **OPTS)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_update_refusals_leave_the_handle_as_it_was(product_lib, device):
    lib = product_lib
    up = (lambda a: batch.DeviceArray(lib, *a.shape).upload(a)) if device else (lambda a: a)
    # boxed family with equalities: an inequality row of one instance turned into an equality, and l > u
    base, q, l, u = S.boxed("banded-33-eq")
    sb, twin = _make(lib, base, q.shape[0], **OPTS), _make(lib, base, q.shape[0], **OPTS)
    for h in (sb, twin):
        h.update(q=q, l=l, u=u)
    bad_l = l.copy(); bad_l[4, 9] = u[4, 9]
    with pytest.raises(oq.OSQPError, match=r"kind of a row.*instance 4, row 9"):
        sb.update(l=up(bad_l), u=up(u))
    bad_l = l.copy(); bad_l[2, 7] = u[2, 7] + 1.0; bad_l[5, 1] = u[5, 1] + 1.0
    with pytest.raises(oq.OSQPError, match=r"lower bound greater than upper bound.*instance 2, row 7"):
        sb.update(l=up(bad_l), u=up(u))
    with pytest.raises(oq.OSQPError, match="cannot be updated"):
        sb.update_settings(polish=1)
    with pytest.raises(oq.OSQPError, match="cannot be updated"):
        sb.update_settings(adaptive_rho=1)
    assert _same(sb.solve(), twin.solve())
    assert _same(sb.solve(), twin.solve())  # and the warm re-solve
    sb.close(); twin.close()
    # chain family: a loose row of one instance given bounds
    base, q, l, u = S.chain(17, 5)
    sb, twin = _make(lib, base, 9, **OPTS), _make(lib, base, 9, **OPTS)
    for h in (sb, twin):
        h.update(q=q, l=l, u=u)
    assert l[3, 0] < -1e29 and u[3, 0] > 1e29
    bad_l, bad_u = l.copy(), u.copy(); bad_l[3, 0], bad_u[3, 0] = -1.0, 1.0
    with pytest.raises(oq.OSQPError, match=r"kind of a row.*instance 3, row 0"):
        sb.update(l=up(bad_l), u=up(bad_u))
    assert _same(sb.solve(), twin.solve())
    sb.close(); twin.close()


# ---- 7. the existing paths are untouched -------------------------------------------------------------------------------------
def test_existing_batched_paths_keep_their_bits(product_lib):
    lib = product_lib
    small, _ = F.instances(F.pattern("banded", (17, 23, 3)), 3, 5)
    large, _ = F.instances(F.pattern("banded", (129, 193, 4)), 3, 6)
    before = (batch.solve_batch(lib, *small, **F.OPTS), batch.solve_batch(lib, *large, large=True, **F.OPTS))
    assert lib.osqp_amd_batch_last_kernel() == -2
    base, q, l, u = S.boxed("banded-129-eq")
    _solve(lib, base, q, l, u, **OPTS)
    assert lib.osqp_amd_batch_last_kernel() == SHARED_KERNEL
    after = (batch.solve_batch(lib, *small, **F.OPTS), batch.solve_batch(lib, *large, large=True, **F.OPTS))
    assert lib.osqp_amd_batch_last_kernel() == -2
    assert _same(before[0], after[0]) and _same(before[1], after[1])
