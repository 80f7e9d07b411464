"""Adjoint derivatives of a single model on the GPU (osqp_amd_adjoint: csrc/direct_adjoint.hpp; `interface.adjoint`;
`qp_layer.QPLayer`).  The reference is `batch_adjoint_ref.exact` -- a dense solve with the KKT matrix of the active set in
the caller's units -- on the engine's OWN returned x, y and act, which isolates the adjoint from ADMM noise.

Bound against `exact`, `rel_err` (relative to max(1, max|exact|) per gradient), per case:
max(1000 x MEASURED[case], 1000 x cond_2(K) x 2.2e-16) -- MEASURED: the numpy model's own figure against `exact`
(tests/test_model_adjoint_host.py); cond_2 from the dense K of the returned act; 1000: the project's margin for "the kernel
sums in another order" (tests/test_batch_adjoint_gpu.py).
FIGURES (MI355X; test_against_exact prints them), achieved / bound:
  tiny (8 instances) 2.2e-16 .. 1.1e-15 / 7.8e-13 .. 1.3e-11   grid2d 3.7e-15 / 1.2e-11   control 1.7e-14 / 8.5e-10
  control, scaling 0 1.6e-14 / 8.5e-10   svm 8.5e-16 / 8.7e-11   equality_qp 1.1e-14 / 7.9e-11   spd7 2.8e-17 / 7.9e-13
  control6_unsorted 3.4e-15 / 2.9e-10
  refinement, 0 steps against the model at 0 steps: 4.0e-15 (scaling 10), 6.2e-15 (scaling 0), both 1.5e-4 from `exact`
  finite differences through the engine's solves: |fd - analytic| 2.6e-10 against a bound of 1.9
  lasso_data 1.4e-14 / 1.7e-10 -- on a factor WITHOUT the dense top block: the explicit inverse of that block (390 of the 720
  pivots; P has a zero diagonal block) fails the factor object's probe and the factor is built again without it
  (tests/test_dense_probe_gpu.py; before the probe this case ended at Max_iter_reached and the adjoint at 1.1e-7)"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_jl_amd as oq
from osqp_jl_amd import types as T
import batch_adjoint_ref as adj
import model_adjoint_ref as mar
import qp_cases
from batch_resident_ref import OPTS
from test_model_adjoint_host import MEASURED
from test_batch_polish_gpu import TOL as POLISH_TOL

pytestmark = pytest.mark.gpu

EPS = 2.2e-16


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _model(product_lib, p, **opts):
    mdl = oq.Model(product_lib)
    oq.setup(mdl, **mar.setup_args(p), **dict(OPTS, polish=True, **opts))
    return mdl


def _sign_pattern(p, y):
    """The active set read off the multipliers: y < 0 lower, y > 0 upper, and l == u counts as lower."""
    return np.where(p["l"] == p["u"], -1, np.where(y < 0, -1, np.where(y > 0, 1, 0)))


def _bound(case, p, act):
    cond = np.linalg.cond(mar.dense_K(p["P"], p["A"], act))
    return max(1000 * MEASURED[case], 1000 * cond * EPS), cond


def _against_exact(case, p, r, g, gx, gy):
    want = mar.caller_order(p, adj.exact(p["P"], p["A"], r.x, r.y, g["act"], gx, gy))
    return adj.rel_err(g, want)


@pytest.mark.parametrize("case,scaling", [(c, 10) for c in mar.CASES] + [("control", 0)])
def test_against_exact(product_lib, oracle_lib, case, scaling):
    """Every case: Solved, the returned act equal to the sign pattern of the returned y, K non-singular under
    it (no case is skipped), and the five gradients within the bound of `exact` on the returned x, y, act."""
    for k, p in enumerate(mar.problems(oracle_lib, case)):
        n, m = len(p["q"]), len(p["l"])
        mdl = _model(product_lib, p, scaling=scaling)
        r = oq.solve(mdl)
        assert r.info.status == "Solved", r.info.status
        gx, gy = mar.incoming(case, k, n, m)
        g = oq.adjoint(mdl, dx=gx[0], dy=gy[0] if m else None)
        st = oq.adjoint_stats(mdl)
        oq.clean(mdl)
        assert np.array_equal(g["act"], _sign_pattern(p, r.y)), (case, k)
        assert (st["n_low"], st["n_upp"], st["kept"]) == (int(np.sum(g["act"] < 0)), int(np.sum(g["act"] > 0)), 1)
        assert adj.nondegenerate(p["A"], g["act"], n), (case, k)
        bound, cond = _bound(case, p, g["act"])
        err = _against_exact(case, p, r, g, gx[0], gy[0])
        print(f"{case}[{k}] scaling {scaling}: polish {r.info.status_polish} n {n} m {m} active {st['n_low']} / {st['n_upp']}  cond K {cond:.2e}  "
              f"vs exact {err:.2e}  bound {bound:.2e}  factor bytes {st['bytes']}")
        assert err <= bound, (case, k, err, bound)


@pytest.mark.parametrize("scaling", [10, 0])
def test_refinement(product_lib, oracle_lib, scaling):
    """control(), polish_refine_iter = 0: the regularised answer -- equal, within the bound, to the numpy model at 0 steps on
    the engine's own solution (the model's scaled state: the oracle's D, E, c -- the engine's equilibration computes the same
    values -- with x~ = x / D, y~ = c y / E, z~ the projection of A~ x~ + y~), and more than 1e-8 from `exact`."""
    case = "control"
    p = mar.problems(oracle_lib, case)[0]
    n, m = len(p["q"]), len(p["l"])
    gx, gy = mar.incoming(case, 0, n, m)
    mdl = _model(product_lib, p, scaling=scaling, polish_refine_iter=0)
    r = oq.solve(mdl)
    assert r.info.status == "Solved"
    g = oq.adjoint(mdl, dx=gx[0], dy=gy[0])
    assert oq.adjoint_stats(mdl)["solves"] == 2  # the regularised solve and its one step against the regularised matrix
    oq.clean(mdl)
    D, E, c = mar.oracle_solution(oracle_lib, case, 0, scaling)["state"][:3]
    _, _, As, ls, us = mar.pol.scale_data(p["P"], p["q"], p["A"], p["l"], p["u"], D, E, c)
    xs, ys = r.x / D, c * r.y / E
    zs = np.minimum(np.maximum(As @ xs + ys, ls), us)
    want0 = mar.model(p["P"], p["q"], p["A"], p["l"], p["u"], D, E, c, xs, zs, ys, gx[0], gy[0], refine=0)
    assert np.array_equal(want0["act"], g["act"])
    bound, cond = _bound(case, p, g["act"])
    e_model, e_exact = adj.rel_err(g, want0), _against_exact(case, p, r, g, gx[0], gy[0])
    print(f"control scaling {scaling}, 0 refinement steps: vs model(0 steps) {e_model:.2e} (bound {bound:.2e})  vs exact {e_exact:.2e}")
    assert e_model <= bound
    assert e_exact > 1e-8


def test_factor_life(product_lib, oracle_lib):
    p = mar.problems(oracle_lib, "control6_unsorted")[0]
    n, m = len(p["q"]), len(p["l"])
    gx, gy = mar.incoming("control6_unsorted", 0, n, m)
    mdl = _model(product_lib, p)
    r = oq.solve(mdl)
    assert oq.adjoint_stats(mdl) == dict(builds=0, solves=0, n_low=0, n_upp=0, kept=0, bytes=0)
    a1 = oq.adjoint(mdl, dx=gx[0], dy=gy[0])
    s1 = oq.adjoint_stats(mdl)
    assert (s1["builds"], s1["kept"], s1["solves"]) == (1, 1, 4) and s1["bytes"] > 0
    assert s1["n_low"] + s1["n_upp"] == np.count_nonzero(a1["act"])
    a2 = oq.adjoint(mdl, dx=gx[0], dy=gy[0])
    assert (oq.adjoint_stats(mdl)["builds"], oq.adjoint_stats(mdl)["solves"]) == (1, 8)
    assert all(_same(a1[k], a2[k]) for k in a1)
    builds = 1

    def refused():
        with pytest.raises(oq.OSQPError, match="osqp_solve"):
            oq.adjoint(mdl, dx=gx[0], dy=gy[0])
        assert oq.adjoint_stats(mdl)["kept"] == 0 and oq.adjoint_stats(mdl)["builds"] == builds

    # a data update: the factor goes, the call is refused until the next solve, which brings a new factor
    oq.update(mdl, q=p["q"] * 1.01)
    assert oq.adjoint_stats(mdl)["kept"] == 0
    refused()
    oq.solve(mdl)
    oq.adjoint(mdl, dx=gx[0], dy=gy[0]); builds += 1
    assert (oq.adjoint_stats(mdl)["builds"], oq.adjoint_stats(mdl)["kept"]) == (builds, 1) and builds == 2
    # a settings update (delta is inside the matrix): the factor goes, the solution stays current
    oq.update_settings(mdl, delta=2e-6)
    assert oq.adjoint_stats(mdl)["kept"] == 0
    oq.adjoint(mdl, dx=gx[0], dy=gy[0]); builds += 1
    assert (oq.adjoint_stats(mdl)["builds"], oq.adjoint_stats(mdl)["kept"]) == (builds, 1)
    oq.update_settings(mdl, delta=1e-6)
    # a warm start
    oq.warm_start(mdl, x=r.x, y=r.y)
    assert oq.adjoint_stats(mdl)["kept"] == 0
    refused()
    # a solve drops a kept factor as well
    oq.update(mdl, q=p["q"])
    oq.solve(mdl)
    b1 = oq.adjoint(mdl, dx=gx[0], dy=gy[0]); builds += 1
    assert oq.adjoint_stats(mdl)["kept"] == 1
    oq.solve(mdl)
    assert oq.adjoint_stats(mdl)["kept"] == 0 and oq.adjoint_stats(mdl)["builds"] == builds
    # release
    oq.adjoint(mdl, dx=gx[0], dy=gy[0]); builds += 1
    oq.adjoint_release(mdl)
    s = oq.adjoint_stats(mdl)
    assert (s["kept"], s["n_low"], s["n_upp"], s["bytes"], s["builds"]) == (0, 0, 0, 0, builds)
    oq.adjoint_release(mdl)  # nothing kept: still fine
    b2 = oq.adjoint(mdl, dx=gx[0], dy=gy[0]); builds += 1
    assert oq.adjoint_stats(mdl)["builds"] == builds == 6
    assert np.array_equal(b1["act"], b2["act"])
    oq.clean(mdl)


def test_several_cotangents(product_lib, oracle_lib):
    case = "control"
    p = mar.problems(oracle_lib, case)[0]
    n, m = len(p["q"]), len(p["l"])
    gx, gy = mar.incoming(case, 0, n, m, ncot=3)
    mdl = _model(product_lib, p)
    assert oq.solve(mdl).info.status == "Solved"
    s0 = oq.adjoint_stats(mdl)["solves"]
    multi = oq.adjoint(mdl, dx=gx, dy=gy)
    assert oq.adjoint_stats(mdl)["solves"] == s0 + 3 * 4
    assert multi["q"].shape == (3, n) and multi["Ax"].shape == (3, p["A"].nnz) and multi["act"].shape == (m,)
    for c in range(3):
        s0 = oq.adjoint_stats(mdl)["solves"]
        one = oq.adjoint(mdl, dx=gx[c], dy=gy[c])
        assert oq.adjoint_stats(mdl)["solves"] == s0 + 4
        assert one["q"].shape == (n,)
        for k in adj.GRADS:
            assert _same(one[k], multi[k][c]), (c, k)
        assert np.array_equal(one["act"], multi["act"])
    only_q = oq.adjoint(mdl, dx=gx, dy=gy, want=("q",))
    assert set(only_q) == {"q", "act"} and _same(only_q["q"], multi["q"])
    # one cotangent missing is a zero cotangent
    z = oq.adjoint(mdl, dx=gx[0], want=("q", "l"))
    z2 = oq.adjoint(mdl, dx=gx[0], dy=np.zeros(m), want=("q", "l"))
    assert _same(z["q"], z2["q"]) and _same(z["l"], z2["l"])
    assert oq.adjoint_stats(mdl)["builds"] == 1
    oq.clean(mdl)


def _info_bytes(mdl):
    ws = mdl.workspace.contents
    return C.string_at(C.addressof(ws.info.contents), C.sizeof(T.CInfo))


def test_nothing_else_moves(product_lib, oracle_lib):
    """grid2d(24): solve, adjoint, solve (warm) gives the bits and the iteration count of solve, solve; the call changes
    neither info nor the stored solution."""
    p = mar.problems(oracle_lib, "grid2d")[0]
    n, m = len(p["q"]), len(p["l"])
    gx, gy = mar.incoming("grid2d", 0, n, m)
    runs = []
    for with_adjoint in (False, True):
        mdl = _model(product_lib, p)
        r1 = oq.solve(mdl)
        if with_adjoint:
            info0, x0, y0 = _info_bytes(mdl), r1.x.copy(), r1.y.copy()
            fact0 = oq.stats(mdl)[8]
            oq.adjoint(mdl, dx=gx[0], dy=gy[0])
            ws = mdl.workspace.contents
            sol = ws.solution.contents
            assert _info_bytes(mdl) == info0
            assert _same(np.ctypeslib.as_array(sol.x, (n,)), x0) and _same(np.ctypeslib.as_array(sol.y, (m,)), y0)
            assert oq.stats(mdl)[8] == fact0  # the ADMM factor was not refactorised
        r2 = oq.solve(mdl)
        runs.append((r1, r2))
        oq.clean(mdl)
    (a1, a2), (b1, b2) = runs
    assert _same(a1.x, b1.x) and _same(a1.y, b1.y) and a1.info.iter == b1.info.iter
    assert _same(a2.x, b2.x) and _same(a2.y, b2.y) and a2.info.iter == b2.info.iter
    assert a2.info.status == b2.info.status == "Solved" and a2.info.rho_updates == b2.info.rho_updates


def _raw_call(lib, mdl, ncot, with_dx=True):
    """The library called directly with NaN-filled outputs: (return code, message, outputs)."""
    n, m = oq.dimensions(mdl)
    st = oq.stats(mdl, 4)
    sizes = dict(q=n, l=m, u=m, Px=int(st[3]), Ax=int(st[1]))
    nc = max(1, ncot)
    outs = {k: np.full(nc * max(1, v), np.nan) for k, v in sizes.items()}
    act = np.full(max(1, m), np.nan)
    dx, dy = np.ones(nc * n), np.ones(nc * max(1, m))
    f = oq.interface._fptr
    rc = lib.osqp_amd_adjoint(mdl.workspace, ncot, f(dx) if with_dx else None, f(dy) if with_dx else None,
                              *(f(outs[k]) for k in adj.GRADS), f(act))
    outs["act"] = act
    return rc, lib.osqp_amd_last_error().decode(), outs


def _assert_refused(lib, mdl, ncot, match, with_dx=True):
    rc, msg, outs = _raw_call(lib, mdl, ncot, with_dx)
    print(f"refused with {rc}: {msg}")
    assert rc != 0 and match in msg, (rc, msg)
    assert all(np.all(np.isnan(v)) for v in outs.values())
    assert oq.adjoint_stats(mdl)["kept"] == 0


def test_refusals(product_lib, oracle_lib, monkeypatch):
    # primal infeasible
    mdl = qp_cases._setup(oq, product_lib, "qdldl", qp_cases._case_from(qp_cases.KA["G16"]), qp_cases.KA["prim_inf_options"])
    assert oq.solve(mdl).info.status == "Primal_infeasible"
    _assert_refused(product_lib, mdl, 1, "Solved")
    oq.clean(mdl)
    # stopped at max_iter = 5
    p = mar.problems(oracle_lib, "control6_unsorted")[0]
    mdl = _model(product_lib, p, max_iter=5)
    assert oq.solve(mdl).info.status == "Max_iter_reached"
    _assert_refused(product_lib, mdl, 1, "Solved")
    oq.clean(mdl)
    # no solve yet; ncot = 0; a gradient wanted without a cotangent
    mdl = _model(product_lib, p)
    _assert_refused(product_lib, mdl, 1, "osqp_solve")
    assert oq.solve(mdl).info.status == "Solved"
    _assert_refused(product_lib, mdl, 0, "ncot")
    _assert_refused(product_lib, mdl, -2, "ncot")
    _assert_refused(product_lib, mdl, 1, "dx and dy", with_dx=False)
    rc, msg, outs = _raw_call(product_lib, mdl, 1)  # and the same call goes through once it is well-formed
    assert rc == 0 and not np.any(np.isnan(outs["q"])) and not np.any(np.isnan(outs["Ax"]))
    oq.clean(mdl)
    # a compact workspace (OSQP_AMD_COMPACT_NNZ=0 with the panels on, indirect back-end; the smallest
    # shape the existing tests force it at: tests/test_gpu_parity.py test_compact_mode)
    monkeypatch.setenv("OSQP_AMD_PANEL", "2")
    monkeypatch.setenv("OSQP_AMD_COMPACT_NNZ", "0")
    mdl = oq.Model(product_lib)
    oq.setup_generated(mdl, 0, 40000, 96, 21, verbose=False, eps_abs=1e-5, eps_rel=1e-5, adaptive_rho_interval=25, linsys_solver="pcg")
    assert oq.stats(mdl)[18] == 1.0
    assert oq.solve(mdl).info.status == "Solved"
    _assert_refused(product_lib, mdl, 1, "compact")
    oq.clean(mdl)


def test_end_to_end_finite_differences(product_lib, oracle_lib):
    """control(T=6): three polished solves of the engine, at the data and at +-h d along a random direction in (q, l, u),
    h = 1e-4 (the solution is piecewise affine in these).  Each polished x / y is within the polish tests' tolerance of the
    exact one, so |fd - analytic| <= POLISH_TOL / h * (|g_x|_1 + |g_y|_1)."""
    case, h = "control6_unsorted", 1e-4
    p = mar.problems(oracle_lib, case)[0]
    n, m = len(p["q"]), len(p["l"])
    gx, gy = (g[0] for g in mar.incoming(case, 0, n, m))
    rng = np.random.default_rng(11)
    dq, dl, du = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)
    du = np.where(p["l"] == p["u"], dl, du)  # an equality row moves as one
    runs = []
    for s in (0.0, 1.0, -1.0):
        mdl = _model(product_lib, dict(p, q=p["q"] + s * h * dq, l=p["l"] + s * h * dl, u=p["u"] + s * h * du))
        r = oq.solve(mdl)
        assert r.info.status == "Solved" and r.info.status_polish == 1
        runs.append((r, oq.adjoint(mdl, dx=gx, dy=gy, want=("q", "l", "u"))))
        oq.clean(mdl)
    (r0, g0) = runs[0]
    assert all(np.array_equal(g["act"], g0["act"]) for _, g in runs)
    loss = [gx @ r.x + gy @ r.y for r, _ in runs[1:]]
    fd, an = (loss[0] - loss[1]) / (2 * h), float(g0["q"] @ dq + g0["l"] @ dl + g0["u"] @ du)
    bound = POLISH_TOL / h * (np.sum(np.abs(gx)) + np.sum(np.abs(gy)))
    print(f"fd {fd:.12e} analytic {an:.12e} |diff| {abs(fd - an):.2e} bound {bound:.2e}")
    assert abs(fd - an) <= bound


def test_torch_layer(product_lib, oracle_lib):
    import torch

    from osqp_jl_amd.qp_layer import QPLayer

    case = "control6_unsorted"
    p = mar.problems(oracle_lib, case)[0]
    n, m = len(p["q"]), len(p["l"])
    w, v = (g[0] for g in mar.incoming(case, 0, n, m))
    mdl = _model(product_lib, p)
    layer = QPLayer(mdl)
    dev = torch.device("cuda:0")
    t = {k: torch.tensor(p[k], device=dev, requires_grad=True) for k in ("q", "l", "u")}
    x, y = layer(**t)
    assert layer.info.status == "Solved" and x.device.type == "cuda"
    ((torch.tensor(w, device=dev) * x).sum() + (torch.tensor(v, device=dev) * y).sum()).backward()
    want = oq.adjoint(mdl, dx=w, dy=v)
    for k in ("q", "l", "u"):
        assert _same(t[k].grad.cpu().numpy(), want[k]), k
    # only the inputs that require a gradient get one, through a call that asks for nothing else; host tensors work too
    q2, l2 = torch.tensor(p["q"], requires_grad=True), torch.tensor(p["l"])
    Ax2 = torch.tensor(p["A_given"].data, requires_grad=True)
    x2, y2 = layer(q=q2, l=l2, Ax=Ax2)
    ((torch.tensor(w) * x2).sum() + (torch.tensor(v) * y2).sum()).backward()
    ref = oq.adjoint(mdl, dx=w, dy=v, want=("q", "Ax"))
    assert l2.grad is None and _same(q2.grad.numpy(), ref["q"]) and _same(Ax2.grad.numpy(), ref["Ax"])
    # the model holds one solution: a backward after a further update raises, and so does one after a later forward
    q3 = torch.tensor(p["q"], requires_grad=True)
    x3, _ = layer(q=q3)
    oq.update(mdl, q=p["q"] * 1.5)
    with pytest.raises(oq.OSQPError, match="osqp_solve"):
        x3.sum().backward()
    q4 = torch.tensor(p["q"], requires_grad=True)
    x4, _ = layer(q=q4)
    layer(q=q3.detach())
    with pytest.raises(RuntimeError, match="solved again"):
        x4.sum().backward()
    oq.clean(mdl)
