"""Forward sensitivities of a single model on the GPU (osqp_amd_jvp: csrc/direct_jvp.hpp; `interface.jvp`,
`interface.jacobian`; `qp_layer.QPFunction.jvp`).  The reference is `batch_jvp_ref.exact` -- a dense solve with the KKT matrix
of the active set in the caller's units -- on the engine's OWN returned x, y and act, which isolates the sensitivities from
ADMM noise.  Directions are given in the caller's nnz order and translated for the reference (model_jvp_ref).

Bound against `exact`, `batch_jvp_ref.rel_err` (relative to max(1, max|exact|) per output), per case:
max(1000 x MEASURED_JVP[case], 1000 x cond_2(K) x 2.2e-16) -- the rule of tests/test_model_adjoint_gpu.py; MEASURED_JVP and
MEASURED_DUALITY: the numpy models' own figures (tests/test_model_jvp_host.py); cond_2 from the dense K of the returned act.
Duality with the device adjoint on the same kept factor, `duality_gap`: max(1000 x MEASURED_DUALITY[case], 1000 x cond_2(K) x 2.2e-16).
Not forced here, as in the adjoint's test: a row-sharded workspace, a reduced factor that is too large (both 6) and a failed
factorisation (4) do not occur at test sizes; their branches are the adjoint's own (direct_adjoint.hpp: adjoint_build).
FIGURES (MI355X; the tests print them), achieved / bound:
  against `exact`: tiny (8 instances) 1.9e-16 .. 1.7e-15 / 9.1e-13 .. 1.3e-11   grid2d 4.4e-15 / 1.2e-11   control 1.2e-14 / 8.5e-10
  control, scaling 0 6.7e-15 / 8.5e-10   svm 9.5e-16 / 8.7e-11   lasso_data 1.5e-14 / 1.7e-10   equality_qp 6.4e-15 / 7.9e-11
  spd7 5.6e-17 / 7.9e-13   control6_unsorted 4.7e-15 / 2.9e-10
  duality with the device adjoint: 0 .. 1.1e-16 on every case / 7.8e-13 (spd7, tiny) .. 8.5e-10 (control)
  one Ax entry of the reversed column: 0 (its row is inactive) and 2.8e-15 / 2.9e-10; read in the sorted order instead: 1.0 and 81
  refinement, 0 steps against the model at 0 steps: 4.3e-15 (scaling 10), 2.8e-15 (scaling 0) / 8.5e-10; 1.4e-4 and 1.7e-4 from `exact`
  central differences through the engine's solves: 3.5e-12 (x), 1.2e-10 (y) / 1.0e-2
  tiny, forward against reverse Jacobians: 3.5e-16 / 1.3e-11"""
import numpy as np
import pytest
import scipy.sparse as sp

import osqp_jl_amd as oq
import batch_jvp_ref as jv
import model_adjoint_ref as mar
import model_jvp_ref as mjr
import qp_cases
from test_model_adjoint_host import MEASURED as MEASURED_ADJ
from test_model_jvp_host import MEASURED_JVP, MEASURED_DUALITY
from test_batch_polish_gpu import TOL as POLISH_TOL
from test_model_adjoint_gpu import _info_bytes, _model, _same, _sign_pattern

pytestmark = pytest.mark.gpu

EPS = 2.2e-16


def _bound(table, case, p, act):
    cond = np.linalg.cond(mar.dense_K(p["P"], p["A"], act))
    return max(1000 * table[case], 1000 * cond * EPS), cond


def _against_exact(p, r, t, d):
    want = jv.exact(p["P"], p["A"], r.x, r.y, t["act"], mjr.reference_direction(p, d))
    return jv.rel_err(t["x"], t["y"], *want)


@pytest.mark.parametrize("case,scaling", [(c, 10) for c in mar.CASES] + [("control", 0)])
def test_against_exact(product_lib, oracle_lib, case, scaling):
    """Every case: Solved, the returned act equal to the sign pattern of the returned y, K non-singular under it, and
    (tx, ty) of one direction in all five arrays within the bound of `exact` on the returned x, y, act."""
    for k, p in enumerate(mar.problems(oracle_lib, case)):
        n, m = len(p["q"]), len(p["l"])
        mdl = _model(product_lib, p, scaling=scaling)
        r = oq.solve(mdl)
        assert r.info.status == "Solved", r.info.status
        d = mjr.direction(mjr.tangents(case, k, p), 0)
        t = oq.jvp(mdl, **d)
        st = oq.adjoint_stats(mdl)
        oq.clean(mdl)
        assert t["x"].shape == (n,) and t["y"].shape == (m,)
        assert np.array_equal(t["act"], _sign_pattern(p, r.y)), (case, k)
        assert (st["n_low"], st["n_upp"], st["kept"], st["builds"]) == (int(np.sum(t["act"] < 0)), int(np.sum(t["act"] > 0)), 1, 1)
        assert mar.adj.nondegenerate(p["A"], t["act"], n), (case, k)
        assert np.all(t["y"][t["act"] == 0] == 0.0)
        bound, cond = _bound(MEASURED_JVP, case, p, t["act"])
        err = _against_exact(p, r, t, d)
        print(f"{case}[{k}] scaling {scaling}: n {n} m {m} active {st['n_low']} / {st['n_upp']}  cond K {cond:.2e}  vs exact {err:.2e}  bound {bound:.2e}")
        assert err <= bound, (case, k, err, bound)


@pytest.mark.parametrize("case", mar.CASES)
def test_duality_with_the_device_adjoint(product_lib, oracle_lib, case):
    """gx . tx + gy . ty = sum_k <gradient_k, direction_k>, both sides from the device on ONE kept factor."""
    for k, p in enumerate(mar.problems(oracle_lib, case)):
        n, m = len(p["q"]), len(p["l"])
        mdl = _model(product_lib, p)
        assert oq.solve(mdl).info.status == "Solved"
        gx, gy = mar.incoming(case, k, n, m)
        d = mjr.direction(mjr.tangents(case, k, p), 0)
        g = oq.adjoint(mdl, dx=gx[0], dy=gy[0] if m else None)
        t = oq.jvp(mdl, **d)
        st = oq.adjoint_stats(mdl)
        oq.clean(mdl)
        assert st["builds"] == 1 and st["solves"] == 8
        bound, cond = _bound(MEASURED_DUALITY, case, p, t["act"])
        gap = jv.duality_gap(gx[0], gy[0], t["x"], t["y"], g, d)  # both in the caller's nnz order: the inner products agree
        print(f"{case}[{k}]: duality gap {gap:.2e}  bound {bound:.2e}  (cond K {cond:.2e})")
        assert gap <= bound, (case, k, gap, bound)


@pytest.mark.parametrize("case", ["control6_unsorted", "svm", "equality_qp"])
def test_bits(product_lib, oracle_lib, case):
    """Direction d of an ndir = 3 call has the bits of the one-direction call; a None tangent those of a tangent of zeros;
    a repeated call is identical.  control6_unsorted: tAx is permuted first; svm / equality_qp: rows longer than one group."""
    p = mar.problems(oracle_lib, case)[0]
    n, m = len(p["q"]), len(p["l"])
    d = mjr.tangents(case, 0, p, ndir=3)
    mdl = _model(product_lib, p)
    assert oq.solve(mdl).info.status == "Solved"
    multi = oq.jvp(mdl, **d)
    s0 = oq.adjoint_stats(mdl)["solves"]
    assert multi["x"].shape == (3, n) and multi["y"].shape == (3, m) and multi["act"].shape == (m,) and s0 == 3 * 4
    again = oq.jvp(mdl, **d)
    assert all(_same(multi[k], again[k]) for k in multi)
    for i in range(3):
        one = oq.jvp(mdl, **mjr.direction(d, i))
        assert one["x"].shape == (n,) and _same(one["x"], multi["x"][i]) and _same(one["y"], multi["y"][i]), i
        assert np.array_equal(one["act"], multi["act"])
    zeros = {k: np.zeros_like(v) for k, v in d.items()}
    for names in (("q",), ("Ax",), ("Px", "l"), ("u", "q", "Ax")):
        some = oq.jvp(mdl, **{k: d[k] for k in names})
        full = oq.jvp(mdl, **dict(zeros, **{k: d[k] for k in names}))
        assert _same(some["x"], full["x"]) and _same(some["y"], full["y"]), names
    assert oq.adjoint_stats(mdl)["builds"] == 1
    oq.clean(mdl)


def test_tangent_order_on_unsorted_columns(product_lib, oracle_lib):
    """control6_unsorted: a direction that moves ONE Ax entry of the reversed column, named by the caller's index."""
    case = "control6_unsorted"
    p = mar.problems(oracle_lib, case)[0]
    moved = np.flatnonzero(p["to_sorted"] != np.arange(len(p["to_sorted"])))
    assert len(moved) >= 2
    mdl = _model(product_lib, p)
    r = oq.solve(mdl)
    assert r.info.status == "Solved"
    for k in (moved[0], moved[-1]):  # the first and the last entry of the column as the caller stored it
        d = dict(Ax=np.zeros(p["A"].nnz))
        d["Ax"][k] = 1.0
        t = oq.jvp(mdl, **d)
        bound, _ = _bound(MEASURED_JVP, case, p, t["act"])
        err = _against_exact(p, r, t, d)
        wrong = jv.rel_err(t["x"], t["y"], *jv.exact(p["P"], p["A"], r.x, r.y, t["act"], d))  # the same index read in the sorted order
        print(f"entry {k} of the reversed column: vs exact {err:.2e} (bound {bound:.2e}); against the untranslated index {wrong:.2e}")
        assert err <= bound
        assert wrong > bound  # the two orders are told apart
    oq.clean(mdl)


@pytest.mark.parametrize("scaling", [10, 0])
def test_refinement(product_lib, oracle_lib, scaling):
    """control(), polish_refine_iter = 0: the regularised answer -- equal, within the bound, to the numpy model at 0 steps on
    the engine's own solution (the scaled state as in tests/test_model_adjoint_gpu.py), and more than 1e-8 from `exact`."""
    case = "control"
    p = mar.problems(oracle_lib, case)[0]
    d = mjr.direction(mjr.tangents(case, 0, p), 0)
    mdl = _model(product_lib, p, scaling=scaling, polish_refine_iter=0)
    r = oq.solve(mdl)
    assert r.info.status == "Solved"
    t = oq.jvp(mdl, **d)
    assert oq.adjoint_stats(mdl)["solves"] == 2  # the regularised solve and its one step against the regularised matrix
    oq.clean(mdl)
    D, E, c = mar.oracle_solution(oracle_lib, case, 0, scaling)["state"][:3]
    _, _, As, ls, us = mar.pol.scale_data(p["P"], p["q"], p["A"], p["l"], p["u"], D, E, c)
    xs, ys = r.x / D, c * r.y / E
    zs = np.minimum(np.maximum(As @ xs + ys, ls), us)
    want0 = mjr.model(p["P"], p["q"], p["A"], p["l"], p["u"], D, E, c, xs, zs, ys, d, refine=0)
    assert np.array_equal(want0["act"], t["act"])
    bound, _ = _bound(MEASURED_JVP, case, p, t["act"])
    e_model, e_exact = jv.rel_err(t["x"], t["y"], want0["tx"], want0["ty"]), _against_exact(p, r, t, d)
    print(f"control scaling {scaling}, 0 refinement steps: vs model(0 steps) {e_model:.2e} (bound {bound:.2e})  vs exact {e_exact:.2e}")
    assert e_model <= bound
    assert e_exact > 1e-8


def _raw_call(lib, mdl, ndir, tangents=True, outputs=True):
    """The library called directly with NaN-filled outputs: (return code, message, outputs)."""
    n, m = oq.dimensions(mdl)
    nd = max(1, ndir)
    outs = dict(x=np.full(nd * n, np.nan), y=np.full(nd * max(1, m), np.nan), act=np.full(max(1, m), np.nan))
    tq, tl = np.ones(nd * n), np.ones(nd * max(1, m))
    f = oq.interface._fptr
    rc = lib.osqp_amd_jvp(mdl.workspace, ndir, f(tq) if tangents else None, f(tl) if tangents else None, None, None, None,
                          f(outs["x"]) if outputs else None, f(outs["y"]) if outputs else None, f(outs["act"]) if outputs else None)
    return rc, lib.osqp_amd_last_error().decode(), outs


def _assert_refused(lib, mdl, ndir, code, match, **kw):
    rc, msg, outs = _raw_call(lib, mdl, ndir, **kw)
    print(f"refused with {rc}: {msg}")
    assert rc == code and match in msg and msg.startswith("osqp_amd_jvp:"), (rc, msg)
    assert all(np.all(np.isnan(v)) for v in outs.values())
    assert oq.adjoint_stats(mdl)["kept"] == 0


def test_factor_life(product_lib, oracle_lib):
    case = "control6_unsorted"
    p = mar.problems(oracle_lib, case)[0]
    n, m = len(p["q"]), len(p["l"])
    gx, gy = mar.incoming(case, 0, n, m)
    d = mjr.direction(mjr.tangents(case, 0, p), 0)
    mdl = _model(product_lib, p)
    r = oq.solve(mdl)
    assert oq.adjoint_stats(mdl) == dict(builds=0, solves=0, n_low=0, n_upp=0, kept=0, bytes=0)
    t1 = oq.jvp(mdl, **d)
    s1 = oq.adjoint_stats(mdl)
    assert (s1["builds"], s1["kept"], s1["solves"]) == (1, 1, 4) and s1["bytes"] > 0
    assert s1["n_low"] + s1["n_upp"] == np.count_nonzero(t1["act"])
    a1 = oq.adjoint(mdl, dx=gx[0], dy=gy[0])  # reuses the factor the jvp built
    s2 = oq.adjoint_stats(mdl)
    assert (s2["builds"], s2["solves"], s2["bytes"]) == (1, 8, s1["bytes"])
    assert np.array_equal(a1["act"], t1["act"])
    # a data update: the factor goes, the call is refused until the next solve, and nothing is written
    oq.update(mdl, q=p["q"] * 1.01)
    assert oq.adjoint_stats(mdl)["kept"] == 0
    _assert_refused(product_lib, mdl, 1, 1, "osqp_solve")
    with pytest.raises(oq.OSQPError, match="osqp_solve"):
        oq.jvp(mdl, **d)
    oq.solve(mdl)
    oq.adjoint(mdl, dx=gx[0], dy=gy[0])  # and the other way round: the adjoint builds, the jvp reuses
    oq.jvp(mdl, **d)
    assert (oq.adjoint_stats(mdl)["builds"], oq.adjoint_stats(mdl)["kept"]) == (2, 1)
    # a settings update (delta is inside the matrix): the factor goes, the solution stays current, the call builds again
    oq.update_settings(mdl, delta=2e-6)
    assert oq.adjoint_stats(mdl)["kept"] == 0
    oq.jvp(mdl, **d)
    assert (oq.adjoint_stats(mdl)["builds"], oq.adjoint_stats(mdl)["kept"]) == (3, 1)
    oq.update_settings(mdl, delta=1e-6)
    # a warm start
    oq.warm_start(mdl, x=r.x, y=r.y)
    assert oq.adjoint_stats(mdl)["kept"] == 0
    _assert_refused(product_lib, mdl, 1, 1, "osqp_solve")
    # release
    oq.update(mdl, q=p["q"])
    oq.solve(mdl)
    t2 = oq.jvp(mdl, **d)
    assert (oq.adjoint_stats(mdl)["builds"], oq.adjoint_stats(mdl)["kept"]) == (4, 1)
    oq.adjoint_release(mdl)
    s = oq.adjoint_stats(mdl)
    assert (s["kept"], s["n_low"], s["n_upp"], s["bytes"], s["builds"]) == (0, 0, 0, 0, 4)
    t3 = oq.jvp(mdl, **d)
    assert oq.adjoint_stats(mdl)["builds"] == 5
    assert np.array_equal(t2["act"], t3["act"])
    oq.clean(mdl)


def test_nothing_else_moves(product_lib, oracle_lib):
    """grid2d(24): solve, jvp, solve (warm) gives the bits and the iteration count of solve, solve; the call changes neither
    info nor the stored solution, and the ADMM factor is not refactorised."""
    case = "grid2d"
    p = mar.problems(oracle_lib, case)[0]
    n, m = len(p["q"]), len(p["l"])
    d = mjr.direction(mjr.tangents(case, 0, p), 0)
    runs = []
    for with_jvp in (False, True):
        mdl = _model(product_lib, p)
        r1 = oq.solve(mdl)
        if with_jvp:
            info0, x0, y0 = _info_bytes(mdl), r1.x.copy(), r1.y.copy()
            fact0 = oq.stats(mdl)[8]
            oq.jvp(mdl, **d)
            sol = mdl.workspace.contents.solution.contents
            assert _info_bytes(mdl) == info0
            assert _same(np.ctypeslib.as_array(sol.x, (n,)), x0) and _same(np.ctypeslib.as_array(sol.y, (m,)), y0)
            assert oq.stats(mdl)[8] == fact0
        r2 = oq.solve(mdl)
        runs.append((r1, r2))
        oq.clean(mdl)
    (a1, a2), (b1, b2) = runs
    assert _same(a1.x, b1.x) and _same(a1.y, b1.y) and a1.info.iter == b1.info.iter
    assert _same(a2.x, b2.x) and _same(a2.y, b2.y) and a2.info.iter == b2.info.iter
    assert a2.info.status == b2.info.status == "Solved" and a2.info.rho_updates == b2.info.rho_updates


def test_refusals(product_lib, oracle_lib, monkeypatch):
    buf = np.full(4, np.nan)
    f = oq.interface._fptr
    assert product_lib.osqp_amd_jvp(None, 1, f(buf), None, None, None, None, f(buf), None, None) == 7 and np.all(np.isnan(buf))
    # primal infeasible
    mdl = qp_cases._setup(oq, product_lib, "qdldl", qp_cases._case_from(qp_cases.KA["G16"]), qp_cases.KA["prim_inf_options"])
    assert oq.solve(mdl).info.status == "Primal_infeasible"
    _assert_refused(product_lib, mdl, 1, 1, "Solved")
    oq.clean(mdl)
    # stopped at max_iter = 5
    p = mar.problems(oracle_lib, "control6_unsorted")[0]
    mdl = _model(product_lib, p, max_iter=5)
    assert oq.solve(mdl).info.status == "Max_iter_reached"
    _assert_refused(product_lib, mdl, 1, 1, "Solved")
    oq.clean(mdl)
    # no solve yet; ndir < 1; sensitivities wanted without a tangent; no output wanted
    mdl = _model(product_lib, p)
    _assert_refused(product_lib, mdl, 1, 1, "osqp_solve")
    assert oq.solve(mdl).info.status == "Solved"
    _assert_refused(product_lib, mdl, 0, 1, "ndir")
    _assert_refused(product_lib, mdl, -2, 1, "ndir")
    _assert_refused(product_lib, mdl, 1, 1, "all NULL", tangents=False)
    _assert_refused(product_lib, mdl, 1, 1, "no output", outputs=False)
    rc, msg, outs = _raw_call(product_lib, mdl, 1)  # and the same call goes through once it is well-formed
    assert rc == 0 and not np.any(np.isnan(outs["x"])) and not np.any(np.isnan(outs["y"])) and not np.any(np.isnan(outs["act"]))
    oq.clean(mdl)
    # a compact workspace, forced as tests/test_model_adjoint_gpu.py forces it
    monkeypatch.setenv("OSQP_AMD_PANEL", "2")
    monkeypatch.setenv("OSQP_AMD_COMPACT_NNZ", "0")
    mdl = oq.Model(product_lib)
    oq.setup_generated(mdl, 0, 40000, 96, 21, verbose=False, eps_abs=1e-5, eps_rel=1e-5, adaptive_rho_interval=25, linsys_solver="pcg")
    assert oq.stats(mdl)[18] == 1.0
    assert oq.solve(mdl).info.status == "Solved"
    _assert_refused(product_lib, mdl, 1, 6, "compact")
    oq.clean(mdl)


def test_end_to_end_finite_differences(product_lib, oracle_lib):
    """control(T=6): three polished solves of the engine, at the data and at +-h d along a random direction in (q, l, u),
    h = 1e-4 (the solution is piecewise affine in these).  Each polished x / y is within the polish tests' tolerance of the
    exact one, so the central difference is within POLISH_TOL / h of the tangent."""
    case, h = "control6_unsorted", 1e-4
    p = mar.problems(oracle_lib, case)[0]
    n, m = len(p["q"]), len(p["l"])
    rng = np.random.default_rng(11)
    dq, dl, du = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)
    du = np.where(p["l"] == p["u"], dl, du)  # an equality row moves as one
    runs = []
    for s in (0.0, 1.0, -1.0):
        mdl = _model(product_lib, dict(p, q=p["q"] + s * h * dq, l=p["l"] + s * h * dl, u=p["u"] + s * h * du))
        r = oq.solve(mdl)
        assert r.info.status == "Solved" and r.info.status_polish == 1
        runs.append((r, oq.jvp(mdl, q=dq, l=dl, u=du)))
        oq.clean(mdl)
    t0 = runs[0][1]
    assert all(np.array_equal(t["act"], t0["act"]) for _, t in runs)
    (rp, _), (rm, _) = runs[1:]
    ex = float(np.max(np.abs((rp.x - rm.x) / (2 * h) - t0["x"])))
    ey = float(np.max(np.abs((rp.y - rm.y) / (2 * h) - t0["y"])))
    print(f"|fd - tx| {ex:.2e}  |fd - ty| {ey:.2e}  bound {POLISH_TOL / h:.2e}")
    assert ex <= POLISH_TOL / h and ey <= POLISH_TOL / h


def test_torch_forward_mode(product_lib, oracle_lib):
    import torch
    import torch.autograd.forward_ad as fwAD

    from osqp_jl_amd.qp_layer import QPFunction, QPLayer

    case = "control6_unsorted"
    p = mar.problems(oracle_lib, case)[0]
    d = mjr.direction(mjr.tangents(case, 0, p), 0)
    mdl = _model(product_lib, p)
    layer = QPLayer(mdl)
    dev = torch.device("cuda:0")
    with fwAD.dual_level():
        dual = {k: fwAD.make_dual(torch.tensor(p[k], device=dev), torch.tensor(d[k], device=dev)) for k in ("q", "l", "u")}
        x, y = layer(**dual)
        assert layer.info.status == "Solved" and x.device.type == "cuda"
        tx, ty = fwAD.unpack_dual(x).tangent, fwAD.unpack_dual(y).tangent
        want = oq.jvp(mdl, q=d["q"], l=d["l"], u=d["u"])
        assert _same(tx.cpu().numpy(), want["x"]) and _same(ty.cpu().numpy(), want["y"])
        # host tensors, a matrix tangent in the caller's nnz order, an input without a tangent
        q2 = fwAD.make_dual(torch.tensor(p["q"]), torch.tensor(d["q"]))
        Ax2 = fwAD.make_dual(torch.tensor(p["A_given"].data), torch.tensor(d["Ax"]))
        x2, y2 = layer(q=q2, l=torch.tensor(p["l"]), Ax=Ax2)
        want = oq.jvp(mdl, q=d["q"], Ax=d["Ax"])
        assert _same(fwAD.unpack_dual(x2).tangent.numpy(), want["x"]) and _same(fwAD.unpack_dual(y2).tangent.numpy(), want["y"])
    # the model holds one solution: a jvp after a later forward raises on the stamp
    q3 = torch.tensor(p["q"], requires_grad=True)
    x3, _ = layer(q=q3)
    layer(q=q3.detach())
    with pytest.raises(RuntimeError, match="solved again"):
        QPFunction.jvp(x3.grad_fn, None, torch.tensor(d["q"]), None, None, None, None)
    oq.clean(mdl)


def test_jacobian(product_lib, oracle_lib):
    """tiny: forward and reverse mode agree within the sum of the two bounds; "auto" makes the smaller number of solves; the
    result does not depend on `chunk`, bit for bit."""
    case = "tiny"
    p = mar.problems(oracle_lib, case)[0]
    n, m = len(p["q"]), len(p["l"])
    mdl = _model(product_lib, p)
    r = oq.solve(mdl)
    assert r.info.status == "Solved"
    solves = lambda: oq.adjoint_stats(mdl)["solves"]
    of, wrt = ("x", "y"), ("q", "l", "u", "Px", "Ax")
    s0 = solves()
    fwd = oq.jacobian(mdl, of=of, wrt=wrt, mode="forward")
    s1 = solves()
    rev = oq.jacobian(mdl, of=of, wrt=wrt, mode="reverse")
    s2 = solves()
    nP, nA = sp.triu(sp.csc_matrix(p["P"]), format="csc").nnz, p["A"].nnz
    assert (s1 - s0, s2 - s1) == (4 * (n + 2 * m + nP + nA), 4 * (n + m))
    assert np.array_equal(fwd["act"], rev["act"])
    bf, _ = _bound(MEASURED_JVP, case, p, fwd["act"])
    br, _ = _bound(MEASURED_ADJ, case, p, fwd["act"])
    worst = 0.0
    for o in of:
        for w in wrt:
            a, b = fwd[(o, w)], rev[(o, w)]
            assert a.shape == b.shape == (dict(x=n, y=m)[o], dict(q=n, l=m, u=m, Px=nP, Ax=nA)[w])
            worst = max(worst, float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(b)))))
    print(f"tiny: forward against reverse Jacobians, worst rel {worst:.2e}  bound {bf + br:.2e}")
    assert worst <= bf + br
    # auto: the smaller number of solves
    s0 = solves()
    auto = oq.jacobian(mdl, of=of, wrt=wrt)  # n + m = 8 outputs against 11 + nnz columns: reverse
    assert solves() - s0 == 4 * (n + m) and all(_same(auto[k], rev[k]) for k in rev)
    s0 = solves()
    auto = oq.jacobian(mdl, of=of, wrt=("q",))  # n = 5 columns against 8 outputs: forward
    assert solves() - s0 == 4 * n and all(_same(auto[(o, "q")], fwd[(o, "q")]) for o in of)
    s0 = solves()
    auto = oq.jacobian(mdl, of=("x",), wrt=("q", "l"), out_rows=dict(x=[3, 0]))  # 2 outputs against 8 columns: reverse
    assert solves() - s0 == 4 * 2 and _same(auto[("x", "l")], rev[("x", "l")][[3, 0]])
    # chunk
    for mode, whole in (("forward", fwd), ("reverse", rev)):
        for chunk in (1, 3, 1000):
            part = oq.jacobian(mdl, of=of, wrt=wrt, mode=mode, chunk=chunk)
            assert all(_same(part[k], whole[k]) for k in whole), (mode, chunk)
    assert oq.adjoint_stats(mdl)["builds"] == 1
    oq.clean(mdl)
