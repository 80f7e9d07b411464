"""The duality gap as a stopping rule inside the batched solve kernels (`ResidentBatch.duality_gap_check`,
osqp_amd_batch_duality_gap_check) on the GPU.  Where every instance must stop with the rule off and on is
decided on the CPU, by the oracle plus numpy (batch_gap_cases.py); test_batch_gap_rule_host.py asserts the margins (no ratio of
a traced check within 5 % of 1) that let these tests demand exact iteration counts."""
import numpy as np
import pytest
from types import SimpleNamespace

import osqp_jl_amd as oq
from osqp_jl_amd import batch
from osqp_jl_amd.interface import OSQPError
import batch_gap_cases as cases
import batch_resident_ref as ref
import duality_ref

pytestmark = pytest.mark.gpu

SOLVED, SOLVED_INACCURATE, MAX_ITER = 1, 2, -2
STATUS = {"Solved": SOLVED, "Solved_inaccurate": SOLVED_INACCURATE, "Max_iter_reached": MAX_ITER}
KERNEL = {name: entry for name, (_, _, _, entry) in cases.PF.items()}


def _ratio(prob, x, y):
    return duality_ref.gap_ratio(cases.as_dict(prob), x, y, cases.RULE_EPS)


def _solve(product_lib, args, rule, **extra):
    rb = batch.ResidentBatch(product_lib, *args, **dict(cases.SETTINGS, **extra))
    if rule:
        rb.duality_gap_check()
    x, y, info = rb.solve()
    return rb, x, y, info


def _check_rule_on(name, tr, probs, x, y, info, refusals, tag):
    """Every instance at exactly its K_on, Solved, the refusals of the checks from K_off on, numpy's ratio below 1, and the
    iterate the oracle's at K_on within the tolerance of batch_resident_ref.compare."""
    for i, row in enumerate(tr):
        print(f"{tag} inst {i}: iter {int(info[i, 0])} status {int(info[i, 1])} refusals {refusals[i]:.0f} ratio {_ratio(probs[i], x[i], y[i]):.4f}"
              f" | K_off {row['K_off']} K_on {row['K_on']}")
    for i, row in enumerate(tr):
        assert int(info[i, 0]) == row["K_on"] and int(info[i, 1]) == SOLVED, (tag, i, info[i, :2], row["K_on"])
        assert refusals[i] == (row["K_on"] - row["K_off"]) // cases.CHECK, (tag, i, refusals[i])
        assert _ratio(probs[i], x[i], y[i]) < 1.0, (tag, i)
    refs = [SimpleNamespace(x=row["checks"][row["K_on"]]["x"], y=row["checks"][row["K_on"]]["y"],
                            info=SimpleNamespace(status_val=SOLVED, status="Solved", iter=row["K_on"])) for row in tr]
    ref.compare(x, y, info, refs, cases.SETTINGS, tag)


# ---- 1. rule on moves the right instances ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.PF))
def test_rule_on_moves_the_right_instances(product_lib, oracle_lib, monkeypatch, name):
    monkeypatch.delenv("OSQP_AMD_BATCH_QUAD_CFG", raising=False)
    args, probs = cases.pf_instances(name)
    tr = cases.rule_trace_batch(oq, oracle_lib, name)
    rb, x, y, info = _solve(product_lib, args, True)
    assert product_lib.osqp_amd_batch_last_kernel() == KERNEL[name] == batch.last_schedule(product_lib)["entry"]
    _check_rule_on(name, tr, probs, x, y, info, rb.gap_refusals(), name + "/on")
    rb.close()
    rb, x, y, info = _solve(product_lib, args, False)
    assert np.array_equal(rb.gap_refusals(), np.zeros(rb.count))
    for i, row in enumerate(tr):
        assert int(info[i, 0]) == row["K_off"] and int(info[i, 1]) == SOLVED, (i, info[i, :2], row["K_off"])
        if row["K_on"] > row["K_off"]:
            r = _ratio(probs[i], x[i], y[i])
            print(f"{name}/off inst {i}: stops at {int(info[i, 0])} with gap ratio {r:.4f}")
            assert r > 1.05, (i, r)
    rb.close()


# ---- 2. every quad entry -------------------------------------------------------------------------------------------------------
# OSQP_AMD_BATCH_QUAD_CFG is read by every setup of a handle (the host schedule is built there, not at load), so the entry is
# forced in this process, as test_batch_entries_gpu.py does
FORCED = [(name, num) for name in ("pf16", "pf24", "pf12") for num in cases.forced_entries(name)]


@pytest.mark.parametrize("name,num", FORCED, ids=["%s-e%d" % f for f in FORCED])
def test_every_quad_entry(product_lib, oracle_lib, monkeypatch, name, num):
    monkeypatch.setenv("OSQP_AMD_BATCH_QUAD_CFG", str(num))
    args, probs = cases.pf_instances(name)
    tr = cases.rule_trace_batch(oq, oracle_lib, name)
    rb, x, y, info = _solve(product_lib, args, True)
    assert product_lib.osqp_amd_batch_last_kernel() == num
    _check_rule_on(name, tr, probs, x, y, info, rb.gap_refusals(), "%s/e%d" % (name, num))
    rb.close()


# ---- 3. instances that do not move -----------------------------------------------------------------------------------------------
def _everything(rb):
    x, y, info = rb.solve()
    return [x, y, info, rb.polish_status()]


@pytest.mark.parametrize("name", cases.FIXED + tuple(cases.PF))
def test_instances_that_do_not_move_keep_their_bits(product_lib, oracle_lib, monkeypatch, name):
    monkeypatch.delenv("OSQP_AMD_BATCH_QUAD_CFG", raising=False)
    if name in cases.PF:
        args = cases.pf_instances(name)[0]
        tr = cases.rule_trace_batch(oq, oracle_lib, name)
        fixed = [i for i, row in enumerate(tr) if row["K_on"] == row["K_off"]]
    else:
        args = cases.fixed_family(name, oracle_lib)[0]
        fixed = list(range(args[4].shape[0]))
    assert len(fixed) >= 2
    res = []
    for rule in (False, True):
        rb = batch.ResidentBatch(product_lib, *args, **dict(cases.SETTINGS, polish=True))
        if rule:
            rb.duality_gap_check()
        res.append(_everything(rb) + [rb.gap_refusals()])
        rb.close()
    off, on = res
    for a, b in zip(off[:4], on[:4]):
        assert np.array_equal(a[fixed], b[fixed], equal_nan=True)
    assert np.array_equal(on[4][fixed], np.zeros(len(fixed))) and np.array_equal(off[4], np.zeros(len(off[4])))
    if name == "mpc":
        assert product_lib.osqp_amd_batch_last_kernel() == 0  # the fixed entry


# ---- 4. life cycle ---------------------------------------------------------------------------------------------------------------
def test_life_cycle(product_lib, oracle_lib, monkeypatch):
    monkeypatch.delenv("OSQP_AMD_BATCH_QUAD_CFG", raising=False)
    name = "pf24"
    args, probs = cases.pf_instances(name)
    tr = cases.rule_trace_batch(oq, oracle_lib, name)
    moving = next(i for i, row in enumerate(tr) if row["K_on"] > row["K_off"])
    fixed = next(i for i, row in enumerate(tr) if row["K_on"] == row["K_off"])
    others = [i for i in range(len(tr)) if i not in (moving, fixed)]
    # cold solves throughout (warm_start off, and the rho of every record put back before a re-solve), so that where a
    # re-solve must stop is what the CPU trace says, not what the device reports
    rho0 = cases.SETTINGS.get("rho", 0.1)
    a = batch.ResidentBatch(product_lib, *args, **dict(cases.SETTINGS, warm_start=False))
    xa, ya, ia = a.solve()
    assert [int(v) for v in ia[:, 0]] == [row["K_off"] for row in tr]
    assert _ratio(probs[moving], xa[moving], ya[moving]) > 1.05 and _ratio(probs[fixed], xa[fixed], ya[fixed]) < 1.0
    d0 = a.duality()
    a.duality_gap_check()
    a.update_settings(rho=rho0)
    assert np.array_equal(a.duality(), d0)  # the switch drops nothing: every instance is still current, at the same point
    assert np.array_equal(a.gap_refusals(), np.zeros(a.count))
    rows = [moving, fixed]
    xs, ys, infos = a.solve(rows=rows)
    refusals = a.gap_refusals(rows=rows)
    print("rows=", rows, "iter", infos[:, 0], "refusals", refusals, "ratio", [_ratio(probs[i], xs[j], ys[j]) for j, i in enumerate(rows)])
    assert [int(v) for v in infos[:, 0]] == [tr[moving]["K_on"], tr[fixed]["K_off"]] and np.all(infos[:, 1] == SOLVED)
    assert np.array_equal(refusals, [(tr[moving]["K_on"] - tr[moving]["K_off"]) // cases.CHECK, 0])
    assert _ratio(probs[moving], xs[0], ys[0]) < 1.0
    assert np.array_equal(xs[1], xa[fixed]) and np.array_equal(ys[1], ya[fixed]) and np.array_equal(infos[1], ia[fixed])
    # those records only: the others still hold the point and the count (zero) they had
    d1 = a.duality()
    assert np.array_equal(d1[others], d0[others]) and np.array_equal(d1[fixed], d0[fixed]) and not np.array_equal(d1[moving], d0[moving])
    assert np.array_equal(a.gap_refusals()[others], np.zeros(len(others)))
    a.update_settings(rho=rho0)
    xr, yr, ir = a.solve(rows=others)
    assert [int(v) for v in ir[:, 0]] == [tr[i]["K_on"] for i in others]
    assert np.array_equal(a.gap_refusals(rows=others), [(tr[i]["K_on"] - tr[i]["K_off"]) // cases.CHECK for i in others])
    assert np.array_equal(a.gap_refusals(rows=rows), refusals)  # and that solve left the first two alone
    a.close()

    # a warm re-solve with the rule on; then off again, from the same warm start as a handle that never had the rule
    wa = batch.ResidentBatch(product_lib, *args, **cases.SETTINGS)
    wb = batch.ResidentBatch(product_lib, *args, **cases.SETTINGS)
    x0, y0, _ = wa.solve()
    wb.solve()
    q2 = args[4] * 1.02
    wa.duality_gap_check()
    wa.update(q=q2)
    x1, y1, i1 = wa.solve()
    probs2 = ref.with_vectors(probs, q=q2)
    for i in range(wa.count):
        r = _ratio(probs2[i], x1[i], y1[i])
        print(f"warm/on inst {i}: iter {int(i1[i, 0])} status {int(i1[i, 1])} ratio {r:.4f} refusals {wa.gap_refusals()[i]:.0f}")
        assert int(i1[i, 1]) == SOLVED and r < 1.0, (i, i1[i, :2], r)
    wa.duality_gap_check(False)
    assert np.array_equal(wa.gap_refusals(), np.zeros(wa.count))
    for h in (wa, wb):  # the same data, the same rho (written into every record), the same iterate
        h.update(q=args[4])
        h.update_settings(rho=cases.SETTINGS.get("rho", 0.1))
        h.warm_start(x=x0, y=y0)
    for u, v in zip(wa.solve(), wb.solve()):
        assert np.array_equal(u, v)
    wa.close(); wb.close()


@pytest.mark.parametrize("extra", [dict(scaled_termination=1), dict(scaling=0)], ids=["scaled_termination", "unscaled"])
def test_variants_against_a_cpu_trace_with_the_same_settings(product_lib, oracle_lib, monkeypatch, extra):
    monkeypatch.delenv("OSQP_AMD_BATCH_QUAD_CFG", raising=False)
    args, probs = cases.pf_instances("pf24")
    tr = cases.rule_trace_batch(oq, oracle_lib, "pf24", **extra)
    rb, x, y, info = _solve(product_lib, args, True, **extra)
    refusals = rb.gap_refusals()
    for i, row in enumerate(tr):
        print(f"{extra} inst {i}: iter {int(info[i, 0])} status {int(info[i, 1])} refusals {refusals[i]:.0f} | K_off {row['K_off']} K_on {row['K_on']}")
    for i, row in enumerate(tr):
        assert int(info[i, 0]) == row["K_on"] and int(info[i, 1]) == SOLVED, (i, info[i, :2], row["K_on"])
        assert refusals[i] == (row["K_on"] - row["K_off"]) // cases.CHECK, (i, refusals[i])
    rb.close()


# ---- 5. approximate pass ---------------------------------------------------------------------------------------------------------
def test_approximate_pass(product_lib, oracle_lib, monkeypatch):
    monkeypatch.delenv("OSQP_AMD_BATCH_QUAD_CFG", raising=False)
    name, inst = cases.APPROX
    args, probs = cases.pf_instances(name)
    row = cases.rule_trace_batch(oq, oracle_lib, name)[inst]
    for limit in cases.approximate_limits(row):
        status, exact, approx = cases.approximate_verdict(oq, oracle_lib, name, inst, limit)
        rb, x, y, info = _solve(product_lib, args, True, max_iter=limit)
        print(f"limit {limit}: CPU {status} (ratios {exact} / at 10 eps {approx}); kernel iter {int(info[inst, 0])} status {int(info[inst, 1])}")
        assert int(info[inst, 1]) == STATUS[status] and int(info[inst, 0]) == limit, (limit, info[inst, :2], status)
        rb.close()


# ---- 6. torch layer --------------------------------------------------------------------------------------------------------------
def test_torch_layer(product_lib, oracle_lib, monkeypatch):
    import torch

    from osqp_jl_amd import qp_layer

    monkeypatch.delenv("OSQP_AMD_BATCH_QUAD_CFG", raising=False)
    name = "pf16"
    args, probs = cases.pf_instances(name)
    tr = cases.rule_trace_batch(oq, oracle_lib, name)
    rb = batch.ResidentBatch(product_lib, *args, **dict(cases.SETTINGS, warm_start=False))
    layer = qp_layer.BatchQPLayer(rb, duality_gap_check=True)
    q = torch.tensor(args[4], dtype=torch.float64, device="cuda", requires_grad=True)
    x, y = layer(q=q)
    info = layer.info.cpu().numpy() if hasattr(layer.info, "cpu") else np.asarray(layer.info)
    assert [int(v) for v in info[:, 0]] == [row["K_on"] for row in tr]
    assert np.array_equal(rb.gap_refusals(), [(row["K_on"] - row["K_off"]) // cases.CHECK for row in tr])
    out = torch.empty(rb.count, dtype=torch.float64, device="cuda")  # the device form
    assert rb.gap_refusals(out=out) is out and np.array_equal(out.cpu().numpy(), rb.gap_refusals())
    part = torch.empty(2, dtype=torch.float64, device="cuda")
    rb.gap_refusals(out=part, rows=[rb.count - 1, 0])
    assert np.array_equal(part.cpu().numpy(), rb.gap_refusals()[[rb.count - 1, 0]])
    (x.sum() + y.sum()).backward()
    assert q.grad is not None and q.grad.shape == q.shape and bool(torch.isfinite(q.grad).all())
    rb.close()


def test_the_handle_is_checked(product_lib):
    assert product_lib.osqp_amd_batch_duality_gap_check(None, 1) == 1
    assert product_lib.osqp_amd_batch_gap_refusals(None, None, 0) == 1
    # a handle that osqp_amd_batch_setup did not create: refused by all three calls, with its message
    mpc_handle = batch.MpcBatch(product_lib, 4, seed=2, **cases.SETTINGS)
    out = np.zeros(4)
    sel = np.zeros(1, dtype=np.int64)
    for rc in (product_lib.osqp_amd_batch_duality_gap_check(mpc_handle.handle, 1),
               product_lib.osqp_amd_batch_gap_refusals(mpc_handle.handle, out.ctypes.data, 0),
               product_lib.osqp_amd_batch_gap_refusals_rows(mpc_handle.handle, batch._iptr(sel), 1, out.ctypes.data, 0)):
        assert rc == 1 and b"osqp_amd_batch_setup" in product_lib.osqp_amd_last_error()
    mpc_handle.close()
    args, _ = cases.pf_instances("pf16")
    rb = batch.ResidentBatch(product_lib, *args, **cases.SETTINGS)
    assert product_lib.osqp_amd_batch_gap_refusals(rb.handle, None, 0) == 1
    with pytest.raises((OSQPError, ValueError)):
        rb.gap_refusals(rows=[rb.count])
    assert np.array_equal(rb.gap_refusals(), np.zeros(rb.count))  # before any solve
    rb.close()
