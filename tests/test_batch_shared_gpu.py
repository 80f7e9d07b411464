"""The shared batch (batch.SharedBatch: one model, many right-hand sides on one KKT inverse; k_batch_solve_shared) on the GPU.
The families and the reference -- one oracle model per instance, set up on the base data and then updated -- are
tests/batch_shared_cases.py; tests/test_batch_shared_host.py holds them to what these tests rest on.  Comparison with the
reference is `batch_resident_ref.compare`: status equal, iteration count within one check, Solved solutions within
50 max(eps_abs, 1e-7) relative to max(1, |ref|), NaN rows where the reference has no solution.  On top of it, `test_shape`
holds info columns 2 to 4 of every Solved instance to the raw data in longdouble and to the stopping rule (`_check_figures`);
the iterates themselves, step by step, are tests/test_batch_shared_steps_gpu.py."""
import numpy as np
import pytest
import scipy.sparse as sp

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


def _check_figures(base, q, l, u, x, y, info, opts, tag):
    """pri_res, dua_res and obj_val of every Solved instance against the RAW data in longdouble (the default unscaled
    termination), and the stopping rule itself:
      dua_res = |P x + q + A' y|_inf and obj_val = 1/2 x' P x + q' x of the returned x, y, within 8 (r + 4) 2^-53 of their scale
        (r: the longest row of [P A'], n for the objective -- the rounding of the sums plus the un-scaling; the scales are those
        of tests/batch_shared_step_ref.py);
      pri_res between dist(A x, [l, u])_inf, less the same tolerance on the rows of A, and the eps_pri of the rule that let the
        instance stop, with |z| taken as |clip(A x, l, u)| + pri_res (z is not returned; its exact value is held by
        tests/test_batch_shared_steps_gpu.py);
      F.criteria_ratios <= 2.0, the margin of tests/test_batch_large_gpu.py."""
    LD, unit = F.LD, 2.0 ** -53
    Pf = (sp.triu(base[0]) + sp.triu(base[0], 1).T).tocsr()
    Ac = sp.csr_matrix(base[2])
    n, m = Ac.shape[1], Ac.shape[0]
    Pd, Ad = Pf.toarray().astype(LD), Ac.toarray().astype(LD).reshape(m, n)
    r_dua = int(np.max(np.diff(Pf.indptr) + np.diff(sp.csc_matrix(base[2]).indptr)))
    r_pri = int(np.max(np.diff(Ac.indptr))) if m else 0
    worst = np.zeros(3)
    for i in np.flatnonzero(info[:, 1] == 1):
        xi, yi, qi = x[i].astype(LD), y[i].astype(LD), q[i].astype(LD)
        px, aty, ax = Pd @ xi, Ad.T @ yi, Ad @ xi
        inf = lambda v: LD(np.max(np.abs(v))) if len(v) else LD(0)
        dua, dua_scale = inf(px + qi + aty), max(LD(1), inf(px), inf(qi), inf(aty))
        obj, obj_scale = LD(0.5) * (xi @ px) + qi @ xi, max(LD(1), LD(0.5) * (np.abs(xi) @ (np.abs(Pd) @ np.abs(xi))) + np.abs(qi) @ np.abs(xi))
        e_dua = float(abs(LD(info[i, 3]) - dua) / (8 * (r_dua + 4) * unit * dua_scale))
        e_obj = float(abs(LD(info[i, 4]) - obj) / (8 * (n + 4) * unit * obj_scale))
        e_pri = 0.0
        if m:
            li, ui = l[i].astype(LD), u[i].astype(LD)
            zc = np.clip(ax, li, ui)
            tol = 8 * (r_pri + 4) * unit * max(LD(1), inf(ax))
            dist, pri = inf(ax - zc), LD(info[i, 2])
            eps_pri = opts["eps_abs"] + opts["eps_rel"] * max(inf(ax), inf(zc) + pri)
            assert dist - tol <= pri <= eps_pri + tol, (tag, i, float(dist), float(pri), float(eps_pri))
            e_pri = float((dist - pri) / tol)
            ratios = F.criteria_ratios(base[0], q[i], base[2], l[i], u[i], x[i], y[i], opts["eps_abs"], opts["eps_rel"])
        else:
            assert info[i, 2] == 0.0
            ratios = (0.0, float(dua / (opts["eps_abs"] + opts["eps_rel"] * max(inf(px), inf(qi)))))
        worst = np.maximum(worst, [e_pri, e_dua, e_obj])
        assert e_dua <= 1.0 and e_obj <= 1.0, (tag, i, e_dua, e_obj)
        assert max(ratios) <= 2.0, (tag, i, ratios)
    print(f"{tag}: (dist - pri_res) / tol {worst[0]:.2e}, dua_res and obj_val errors / tolerance {worst[1]:.2e} {worst[2]:.2e}")


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
    _check_figures(base, q, l, u, x, y, info, OPTS, f"{name} T={T}")


# ---- 2. independence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["banded-17", "banded-129-eq", "banded-256", "banded-130-m400", "banded-241-eq", "banded-200-m460"])
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
@pytest.mark.parametrize("name", ["banded-33-eq", "banded-129-eq", "banded-176-eq"])
def test_life_cycle(product_lib, oracle_lib, name, warm):
    opts = dict(OPTS, warm_start=bool(warm))
    host = _life_cycle(product_lib, oracle_lib, name, False, **opts)
    dev = _life_cycle(product_lib, oracle_lib, name, True, **opts)
    for a, b in zip(host, dev):
        assert _same(a, b)  # host arrays and device arrays: the same bits


# ---- 5. rho update -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["banded-17", "banded-129-eq", "banded-176-eq"])
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
    # boxed families with equalities (T = 16 and T = 8): an inequality row of one instance turned into an equality, and l > u
    for name in ("banded-33-eq", "banded-176-eq"):
        base, q, l, u = S.boxed(name)
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
