"""The derivative factor of a single model kept across solves while the active set holds (osqp_amd_adjoint_retain:
csrc/direct_adjoint.hpp; `interface.adjoint_retain`, `qp_layer.QPLayer(retain_factor=True)`).

Every comparison is against a TWIN model set up identically, left at the default life cycle and driven through the same
calls: the twin rebuilds its factor after every solve, so it is the reference.  The relation is BIT EQUALITY of `act`, of
the five gradients and of the JVP with all five tangents: the retained path runs the same kernels on the same values in
the same structure.  `test_the_reference_is_reproducible` establishes first that two default twins give equal bits at
these shapes.  Each test takes its precondition (the active set held / moved) from the twin's returned `act` and FAILS
when it does not hold.

lasso_data: the kept factor is the one rebuilt without its dense top block after the probe (tests/test_dense_probe_gpu.py),
so its refactorisation runs on that form.

test_life_cycle: a solve that does not end Solved cannot be produced by `max_iter=1` while a stale state is held -- every
settings update drops the state, stale or not -- so the test reaches a status other than Solved through a data update
(every row an equality A x = 1: 136 equations in 80 unknowns) and then checks that the settings update drops the state."""
import numpy as np
import pytest

import osqp_jl_amd as oq
import batch_adjoint_ref as adj
import model_adjoint_ref as mar
import model_jvp_ref as mjr
from batch_resident_ref import OPTS
from test_model_device_gpu import _dev, _values

pytestmark = pytest.mark.gpu

NO_CHECKS = dict(mode=1, checks=0, reused=0, refactorised=0, rebuilt_active_set=0, rebuilt_failed=0, last_rows_changed=0, stale=0)


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def _same(a, b):
    return np.array_equal(_np(a), _np(b), equal_nan=True)


def _model(product_lib, p, retain=False, **opts):
    mdl = oq.Model(product_lib)
    oq.setup(mdl, **mar.setup_args(p), **dict(OPTS, polish=True, **opts))
    if retain:
        oq.adjoint_retain(mdl)
    return mdl


def _change(p, what, factor):
    """{name: new array} of one perturbation of the table: "q", "Px" or "Ax" times `factor`."""
    if what == "q":
        return dict(q=p["q"] * factor)
    Px, Ax = _values(p)
    return dict(Px=Px * factor) if what == "Px" else dict(Ax=Ax * factor)


def _step(mdl, case, p, change=None, dev=False):
    """(update,) solve, adjoint with all five gradients, JVP with all five tangents; host forms or device forms."""
    put = _dev if dev else (lambda a: a)
    if change:
        oq.update(mdl, **{k: put(v) for k, v in change.items()})
    r = oq.solve(mdl)
    assert r.info.status == "Solved", (case, r.info.status)
    n, m = len(p["q"]), len(p["l"])
    gx, gy = (g[0] for g in mar.incoming(case, 0, n, m))
    a = oq.adjoint(mdl, dx=put(gx), dy=put(gy) if m else None)
    t = oq.jvp(mdl, **{k: put(v) for k, v in mjr.direction(mjr.tangents(case, 0, p), 0).items()})
    return r, a, t


def _act(step):
    return _np(step[1]["act"]).astype(int)


def _assert_equal_steps(got, want, what):
    (rg, ag, tg), (rw, aw, tw) = got, want
    assert _same(rg.x, rw.x) and _same(rg.y, rw.y) and rg.info.iter == rw.info.iter, what
    assert set(ag) == set(aw) == set(adj.GRADS) | {"act"}
    for k in ag:
        assert _same(ag[k], aw[k]), (what, k)
    for k in ("x", "y", "act"):
        assert _same(tg[k], tw[k]), (what, "jvp", k)


REPRODUCIBLE = [("grid2d", "Ax"), ("svm", "Px"), ("lasso_data", "Ax"), ("control6_unsorted", "Ax"), ("spd7", "Px")]


@pytest.mark.parametrize("case,what", REPRODUCIBLE)
def test_the_reference_is_reproducible(product_lib, oracle_lib, case, what):
    """Two default twins through solve, derivatives, a matrix and a q update, solve, derivatives: equal bits."""
    p = mar.problems(oracle_lib, case)[0]
    A, B = _model(product_lib, p), _model(product_lib, p)
    _assert_equal_steps(_step(A, case, p), _step(B, case, p), case)
    change = dict(_change(p, what, 1.01), q=p["q"] * 1.001)
    _assert_equal_steps(_step(A, case, p, change), _step(B, case, p, change), case)
    assert oq.adjoint_stats(A)["builds"] == oq.adjoint_stats(B)["builds"] == 2
    oq.clean(A); oq.clean(B)


@pytest.mark.parametrize("case,dev", [("grid2d", False), ("svm", False), ("grid2d", True)])
def test_reused_as_it_is(product_lib, oracle_lib, case, dev):
    p = mar.problems(oracle_lib, case)[0]
    R, T = _model(product_lib, p, retain=True), _model(product_lib, p)
    r1, t1 = _step(R, case, p, dev=dev), _step(T, case, p, dev=dev)
    _assert_equal_steps(r1, t1, "first solve")
    held = oq.adjoint_stats(R)
    assert oq.adjoint_retain_stats(R) == NO_CHECKS and oq.adjoint_retain_stats(T) == dict(NO_CHECKS, mode=0)
    change = _change(p, "q", 1.001)
    r2, t2 = _step(R, case, p, change, dev=dev), _step(T, case, p, change, dev=dev)
    assert np.array_equal(_act(t1), _act(t2)), "precondition: q x 1.001 leaves the twin's active set as it was"
    st, rt = oq.adjoint_stats(R), oq.adjoint_retain_stats(R)
    print(f"{case} dev={dev}: {rt}")
    assert rt == dict(NO_CHECKS, checks=1, reused=1)
    assert st["builds"] == 1 and st["kept"] == 1 and st["bytes"] == held["bytes"] and (st["n_low"], st["n_upp"]) == (held["n_low"], held["n_upp"])
    assert oq.adjoint_stats(T)["builds"] == 2 and oq.adjoint_retain_stats(T) == dict(NO_CHECKS, mode=0)
    _assert_equal_steps(r2, t2, "second solve")
    if dev:
        calls = oq.device_form_calls(R)
        assert calls == oq.device_form_calls(T) and (calls["update_vectors"], calls["adjoint"], calls["jvp"]) == (1, 2, 2)
    oq.clean(R); oq.clean(T)


@pytest.mark.parametrize("case,what,dev", [("svm", "Px", False), ("lasso_data", "Ax", False), ("control6_unsorted", "Ax", True)])
def test_numeric_refactorisation(product_lib, oracle_lib, case, what, dev):
    """A matrix update with the active set unchanged: the kept structure is factorised numerically again, nothing is
    built.  Then a matrix update followed by a vector update before one solve: the dirty mark survives the second update."""
    p = mar.problems(oracle_lib, case)[0]
    R, T = _model(product_lib, p, retain=True), _model(product_lib, p)
    r1, t1 = _step(R, case, p, dev=dev), _step(T, case, p, dev=dev)
    _assert_equal_steps(r1, t1, "first solve")
    change = _change(p, what, 1.01)
    r2, t2 = _step(R, case, p, change, dev=dev), _step(T, case, p, change, dev=dev)
    assert np.array_equal(_act(t1), _act(t2)), f"precondition: {what} x 1.01 leaves the twin's active set as it was"
    rt = oq.adjoint_retain_stats(R)
    print(f"{case} {what} dev={dev}: {rt}")
    assert rt == dict(NO_CHECKS, checks=1, refactorised=1)
    assert oq.adjoint_stats(R)["builds"] == 1 and oq.adjoint_stats(T)["builds"] == 2
    _assert_equal_steps(r2, t2, "after the matrix update")
    put = _dev if dev else (lambda a: a)
    for mdl in (R, T):
        oq.update(mdl, **{k: put(v) for k, v in change.items()})
        assert oq.adjoint_retain_stats(mdl)["stale"] == (1 if mdl is R else 0)
    vec = _change(p, "q", 1.001)
    r3, t3 = _step(R, case, p, vec, dev=dev), _step(T, case, p, vec, dev=dev)
    assert np.array_equal(_act(t2), _act(t3)), "precondition: q x 1.001 on top leaves the twin's active set as it was"
    assert oq.adjoint_retain_stats(R) == dict(NO_CHECKS, checks=2, refactorised=2)
    assert oq.adjoint_stats(R)["builds"] == 1 and oq.adjoint_stats(T)["builds"] == 3
    _assert_equal_steps(r3, t3, "after the matrix and the vector update")
    oq.clean(R); oq.clean(T)


@pytest.mark.parametrize("what,factor", [("q", 1.1), ("Ax", 1.01)])
def test_active_set_moved(product_lib, oracle_lib, what, factor):
    case = "grid2d"
    p = mar.problems(oracle_lib, case)[0]
    R, T = _model(product_lib, p, retain=True), _model(product_lib, p)
    r1, t1 = _step(R, case, p), _step(T, case, p)
    change = _change(p, what, factor)
    r2, t2 = _step(R, case, p, change), _step(T, case, p, change)
    moved = int(np.sum(_act(t1) != _act(t2)))
    rt = oq.adjoint_retain_stats(R)
    print(f"grid2d {what} x {factor}: rows that changed side {moved}: {rt}")
    assert moved > 0, "precondition: the twin's active set moved"
    assert int(np.sum(_act(r1) != _act(r2))) == moved
    assert rt == dict(NO_CHECKS, checks=1, rebuilt_active_set=1, last_rows_changed=moved)
    assert oq.adjoint_stats(R)["builds"] == 2 and oq.adjoint_stats(T)["builds"] == 2
    _assert_equal_steps(r1, t1, "first solve")
    _assert_equal_steps(r2, t2, "second solve")
    oq.clean(R); oq.clean(T)


def test_life_cycle(product_lib, oracle_lib):
    case = "control6_unsorted"
    p = mar.problems(oracle_lib, case)[0]
    n, m = len(p["q"]), len(p["l"])
    gx, gy = (g[0] for g in mar.incoming(case, 0, n, m))
    mdl = _model(product_lib, p, retain=True)
    kept = lambda: (oq.adjoint_stats(mdl)["kept"], oq.adjoint_retain_stats(mdl)["stale"])
    derive = lambda: oq.adjoint(mdl, dx=gx, dy=gy)

    def refused(match="osqp_solve"):
        held = oq.adjoint_stats(mdl)
        with pytest.raises(oq.OSQPError, match=match):
            derive()
        assert kept() == (1, 1) and oq.adjoint_stats(mdl) == held and held["bytes"] > 0

    def make_stale():
        oq.update(mdl, q=p["q"], l=p["l"], u=p["u"])
        assert oq.solve(mdl).info.status == "Solved"
        derive()
        assert kept() == (1, 0)
        oq.update(mdl, q=p["q"] * 1.001)
        assert kept() == (1, 1)

    r = oq.solve(mdl)
    assert kept() == (0, 0)
    derive()
    assert kept() == (1, 0) and oq.adjoint_retain_stats(mdl) == NO_CHECKS
    # an update, a warm start: stale, refused until the next solve, and still held afterwards
    oq.update(mdl, q=p["q"] * 1.001)
    assert kept() == (1, 1)
    refused()
    oq.warm_start(mdl, x=r.x, y=r.y)
    refused()
    # two solves in a row, then one derivative call: one check
    oq.solve(mdl); oq.solve(mdl)
    assert kept() == (1, 1) and oq.adjoint_retain_stats(mdl)["checks"] == 0
    derive()
    assert kept() == (1, 0) and oq.adjoint_retain_stats(mdl)["checks"] == 1 and oq.adjoint_stats(mdl)["builds"] == 1
    derive()
    assert oq.adjoint_retain_stats(mdl)["checks"] == 1
    # a solve that does not end Solved (see the module's docstring): refused with 1, the state stays stale
    oq.update(mdl, l=np.ones(m), u=np.ones(m))
    status = oq.solve(mdl).info.status
    print(f"every row an equality: {status}")
    assert status != "Solved"
    refused(match="Solved")
    f = oq.interface._fptr
    out = np.full(n, np.nan)
    assert product_lib.osqp_amd_adjoint(mdl.workspace, 1, f(gx), f(gy), f(out), None, None, None, None, None) == 1 and np.all(np.isnan(out))
    assert kept() == (1, 1) and oq.adjoint_retain_stats(mdl)["checks"] == 1
    # a settings update drops a stale state
    oq.update_settings(mdl, max_iter=4000)
    assert kept() == (0, 0)
    for drop in (lambda: oq.update_settings(mdl, delta=2e-6), lambda: oq.adjoint_release(mdl), lambda: oq.derivative_method(mdl, "auto")):
        make_stale()
        drop()
        assert kept() == (0, 0) and oq.adjoint_stats(mdl)["bytes"] == 0
    oq.update_settings(mdl, delta=1e-6)
    oq.derivative_method(mdl, "direct")
    # mode 0 drops a stale state and leaves a current one
    make_stale()
    oq.adjoint_retain(mdl, False)
    assert kept() == (0, 0) and oq.adjoint_retain_stats(mdl)["mode"] == 0
    oq.adjoint_retain(mdl, True)
    oq.solve(mdl)
    derive()
    oq.adjoint_retain(mdl, False)
    assert kept() == (1, 0)
    oq.update(mdl, q=p["q"])  # ... and from then on the default's life cycle
    assert kept() == (0, 0)
    # the C boundary
    assert product_lib.osqp_amd_adjoint_retain(mdl.workspace, 2) == 1 and b"mode" in product_lib.osqp_amd_last_error()
    assert oq.adjoint_retain_stats(mdl)["mode"] == 0
    assert product_lib.osqp_amd_adjoint_retain(None, 1) == 7
    buf = np.full(8, np.nan)
    assert product_lib.osqp_amd_adjoint_retain_stats(mdl.workspace, f(buf), 3) == 3 and not np.any(np.isnan(buf[:3])) and np.all(np.isnan(buf[3:]))
    assert product_lib.osqp_amd_adjoint_retain_stats(None, f(buf), 8) == 0
    oq.clean(mdl)


def test_nothing_else_moves(product_lib, oracle_lib):
    """grid2d: solve, adjoint, update q, solve, adjoint (a check and a reuse), solve gives the x, y, iteration counts and
    ADMM factorisations of the same sequence without derivative calls."""
    case = "grid2d"
    p = mar.problems(oracle_lib, case)[0]
    n, m = len(p["q"]), len(p["l"])
    gx, gy = (g[0] for g in mar.incoming(case, 0, n, m))
    runs = []
    for derivatives in (False, True):
        mdl = _model(product_lib, p, retain=derivatives)
        out = [oq.solve(mdl)]
        if derivatives:
            oq.adjoint(mdl, dx=gx, dy=gy)
        oq.update(mdl, q=p["q"] * 1.001)
        out.append(oq.solve(mdl))
        if derivatives:
            oq.adjoint(mdl, dx=gx, dy=gy)
            assert oq.adjoint_retain_stats(mdl) == dict(NO_CHECKS, checks=1, reused=1)
        out.append(oq.solve(mdl))
        runs.append((out, oq.stats(mdl)[8]))
        oq.clean(mdl)
    (plain, fact_plain), (derived, fact_derived) = runs
    for a, b in zip(plain, derived):
        assert _same(a.x, b.x) and _same(a.y, b.y) and a.info.iter == b.info.iter and a.info.status == b.info.status == "Solved"
    assert fact_plain == fact_derived


def test_no_constraints(product_lib, oracle_lib):
    """spd7 (m = 0): nothing to classify -- a q update reuses, a Px update refactorises."""
    case = "spd7"
    p = mar.problems(oracle_lib, case)[0]
    R, T = _model(product_lib, p, retain=True), _model(product_lib, p)
    _assert_equal_steps(_step(R, case, p), _step(T, case, p), "first solve")
    change = _change(p, "q", 1.001)
    _assert_equal_steps(_step(R, case, p, change), _step(T, case, p, change), "q update")
    assert oq.adjoint_retain_stats(R) == dict(NO_CHECKS, checks=1, reused=1)
    change = _change(p, "Px", 1.01)
    _assert_equal_steps(_step(R, case, p, change), _step(T, case, p, change), "Px update")
    assert oq.adjoint_retain_stats(R) == dict(NO_CHECKS, checks=2, reused=1, refactorised=1)
    assert oq.adjoint_stats(R)["builds"] == 1 and oq.adjoint_stats(T)["builds"] == 3
    oq.clean(R); oq.clean(T)


def test_the_iterative_state_is_not_retained(product_lib, oracle_lib):
    case = "grid2d"
    p = mar.problems(oracle_lib, case)[0]
    n, m = len(p["q"]), len(p["l"])
    gx, gy = (g[0] for g in mar.incoming(case, 0, n, m))
    mdl = _model(product_lib, p, retain=True, linsys_solver="pcg")
    oq.derivative_method(mdl, "iterative")
    assert oq.solve(mdl).info.status == "Solved"
    oq.adjoint(mdl, dx=gx, dy=gy)
    assert oq.derivative_iter_stats(mdl)["builds"] == 1 and oq.adjoint_stats(mdl)["kept"] == 1
    oq.update(mdl, q=p["q"] * 1.001)
    assert oq.adjoint_stats(mdl)["kept"] == 0 and oq.adjoint_retain_stats(mdl)["stale"] == 0
    assert oq.solve(mdl).info.status == "Solved"
    oq.adjoint(mdl, dx=gx, dy=gy)
    assert oq.derivative_iter_stats(mdl)["builds"] == 2
    assert oq.adjoint_retain_stats(mdl) == NO_CHECKS
    oq.clean(mdl)


@pytest.mark.parametrize("cuda", [False, True])
def test_torch_layer(product_lib, oracle_lib, cuda):
    """Four steps of q <- q - 1e-3 grad on svm through QPLayer(retain_factor=True) and through a twin layer without it:
    equal gradients step by step, one check per later step, and as many reuses as steps whose `act` (the twin's) equals
    the step's before -- a layer that silently rebuilt every time fails."""
    import torch

    from osqp_jl_amd.qp_layer import QPLayer

    case = "svm"
    p = mar.problems(oracle_lib, case)[0]
    n, m = len(p["q"]), len(p["l"])
    where = dict(device="cuda:0") if cuda else {}
    w, v = (torch.tensor(g[0], **where) for g in mar.incoming(case, 0, n, m))
    R, T = _model(product_lib, p), _model(product_lib, p)
    layers = QPLayer(R, retain_factor=True), QPLayer(T)
    assert oq.adjoint_retain_stats(R)["mode"] == 1 and oq.adjoint_retain_stats(T)["mode"] == 0
    q = [p["q"].copy(), p["q"].copy()]
    acts = []
    for step in range(4):
        grads = []
        for k, layer in enumerate(layers):
            t = torch.tensor(q[k], requires_grad=True, **where)
            x, y = layer(q=t)
            assert layer.info.status == "Solved" and x.is_cuda == cuda
            ((w * x).sum() + (v * y).sum()).backward()
            grads.append(t.grad.cpu().numpy())
            q[k] = q[k] - 1e-3 * grads[k]
        assert _same(grads[0], grads[1]), step
        acts.append(oq.adjoint(T, want=())["act"])
    same_as_before = sum(int(np.array_equal(acts[k], acts[k - 1])) for k in range(1, 4))
    rt = oq.adjoint_retain_stats(R)
    print(f"cuda={cuda}: steps with the active set of the step before {same_as_before} of 3: {rt}")
    assert rt["checks"] == 3 and rt["reused"] + rt["refactorised"] + rt["rebuilt_active_set"] + rt["rebuilt_failed"] == 3
    assert rt["reused"] == same_as_before and rt["refactorised"] == 0 and rt["rebuilt_failed"] == 0
    assert oq.adjoint_stats(R)["builds"] == 1 + rt["rebuilt_active_set"] and oq.adjoint_stats(T)["builds"] == 4
    oq.clean(R); oq.clean(T)
