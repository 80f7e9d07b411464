"""The iterative derivatives of a single model on the GPU (osqp_amd_derivative_method: csrc/pcg.hip kkt_iter_solve,
csrc/direct_adjoint.hpp, csrc/panel.hip k_sell_outer; `interface.derivative_method`).

References: `exact` of batch_adjoint_ref / batch_jvp_ref -- dense solves with the KKT matrix of the active set in the caller's
units -- on the engine's OWN returned x, y, act; on the compact shape (no factorisation possible) scipy products on the host
data.  Bound against `exact`, per case: max(1000 x MEASURED_ITER[case], 1000 x cond_2(K) x 2.2e-16) -- the rule of
tests/test_model_adjoint_gpu.py with the iterative numpy model's figure (tests/test_model_adjoint_iter_host.py) in place of
the direct one; duality likewise with MEASURED_ITER_DUALITY.

COMPACT_MODEL_RESIDUAL (test 6): the relative residual ||K s - b||inf / ||b||inf, caller units, that the numpy statement of
the solve (model_adjoint_iter_ref.kkt_iter, default constants) leaves on the compact instance itself -- oracle_generate(0,
40000, 96, 21), the oracle's own solve at eps 1e-5 with the indirect back-end and its scaled state, g_x, g_y from
default_rng(6) (1293 lower and 1240 upper active rows): run once on a CPU (90 s), 4 outer steps, 4340 CG iterations, reached
drop 5.5e-11, residual 2.553e-11.  The bound of 6(a) and 6(c) is 1000 times that (floor 1e-12).
FIGURES (MI355X; the tests print them), worse of adjoint and JVP / bound, then duality / bound, then outer steps:
  tiny (8 instances) 1.8e-15 .. 1.6e-12 / 1.6e-9, <= 1.5e-13 / 1.6e-10, 5-6   grid2d 1.4e-11 / 1.4e-8, 3.3e-14 / 3.3e-11, 6
  control 3.6e-8 / 3.7e-5, 2.7e-10 / 2.7e-7, 15   svm 1.7e-9 / 1.7e-6, 1.7e-11 / 1.7e-8, 8   lasso_data 1.1e-11 / 1.1e-8, 4.8e-15 / 1.7e-10, 5
  equality_qp 1.6e-11 / 1.7e-8, 3.6e-15 / 7.9e-11, 6   spd7 3.4e-15 / 3.5e-12, 4.2e-17 / 7.9e-13, 5
  control6_unsorted 2.6e-10 / 2.6e-7, 1.4e-11 / 1.4e-8, 10          control, direct against iterative on one workspace: 3.6e-8 / 3.7e-5
  the compact shape (n = m = 40000, 1293 + 1240 active rows): residual 3.8e-11 / 2.6e-8 in 4 outer steps (8546 CG iterations with
  the JVP's), every entry of dPx (1 958 824) and dAx (3 840 000) within 8 eps of its terms, duality gap 9.6e-16 / 2.6e-8
  small compact shapes: control6_unsorted (64 columns) 4.9e-10 / 2.6e-7   control (64 columns, 3 panels per group) 3.6e-8 / 3.7e-5
  svm (256 columns, 2 per group) 4.3e-10 / 1.7e-6   equality_qp (256 columns; A' keeps its CSR arrays) 1.8e-11 / 1.7e-8
  svm with only A' compact (512 columns): q, l, u, Px 4.3e-10 / 1.7e-6, dAx refused with 6"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_jl_amd as oq
import batch_adjoint_ref as adj
import batch_jvp_ref as jv
import model_adjoint_ref as mar
import model_jvp_ref as mjr
from batch_resident_ref import OPTS
from osqp_jl_amd.batch import DeviceArray
from test_gpu_parity import _data_to_scipy
from test_model_adjoint_host import MEASURED
from test_model_adjoint_iter_host import MEASURED_ITER, MEASURED_ITER_DUALITY, NOT_CONVERGED

pytestmark = pytest.mark.gpu

EPS = 2.2e-16
SENTINEL = -7.25
COMPACT_MODEL_RESIDUAL = 2.6e-11  # see the docstring
COMPACT_ENV = dict(OSQP_AMD_PANEL="2", OSQP_AMD_COMPACT_NNZ="0")
COMPACT_OPTS = dict(verbose=False, eps_abs=1e-5, eps_rel=1e-5, adaptive_rho_interval=25, linsys_solver="pcg")


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _model(product_lib, p, method="iterative", linsys="pcg", **opts):
    mdl = oq.Model(product_lib)
    oq.setup(mdl, **mar.setup_args(p), **{**OPTS, "polish": True, "linsys_solver": linsys, **opts})
    if method is not None:
        oq.derivative_method(mdl, method)
    return mdl


def _bounds(case, p, act):
    cond = np.linalg.cond(mar.dense_K(p["P"], p["A"], act))
    floor = 1000 * cond * EPS
    return max(1000 * MEASURED_ITER[case], floor), max(1000 * MEASURED_ITER_DUALITY[case], floor), cond


def _direction(case, k, p, i=0, ndir=1):
    """Direction i of the seeded tangents in the caller's order, arrays without entries left out."""
    return {name: v for name, v in mjr.direction(mjr.tangents(case, k, p, ndir), i).items() if len(v)}


def _check_against_exact(case, k, p, mdl, r, label=""):
    """Adjoint with all five gradients and JVP with all five tangents on a solved model, against `exact` and each other."""
    n, m = len(p["q"]), len(p["l"])
    gx, gy = (g[0] for g in mar.incoming(case, k, n, m))
    g = oq.adjoint(mdl, dx=gx, dy=gy if m else None)
    d = _direction(case, k, p)
    t = oq.jvp(mdl, **d)
    it = oq.derivative_iter_stats(mdl)
    assert np.array_equal(g["act"], t["act"]) and adj.nondegenerate(p["A"], g["act"], n), (case, k)
    b_exact, b_dual, cond = _bounds(case, p, g["act"])
    err_a = adj.rel_err(g, mar.caller_order(p, adj.exact(p["P"], p["A"], r.x, r.y, g["act"], gx, gy)))
    tx, ty = jv.exact(p["P"], p["A"], r.x, r.y, t["act"], mjr.reference_direction(p, d))
    err_j = jv.rel_err(t["x"], t["y"], tx, ty)
    gap = jv.duality_gap(gx, gy, t["x"], t["y"], g, d)
    print(f"{label}{case}[{k}]: n {n} m {m} cond K {cond:.2e}  adjoint {err_a:.2e} jvp {err_j:.2e} / {b_exact:.2e}  duality {gap:.2e} / {b_dual:.2e}  "
          f"outer {it['last_outer_steps']} drop {it['last_drop']:.1e} cg {it['cg_iters']}")
    assert err_a <= b_exact and err_j <= b_exact, (case, k, err_a, err_j, b_exact)
    assert gap <= b_dual, (case, k, gap, b_dual)
    assert it["kept"] == 1 and it["builds"] == 1 and oq.adjoint_stats(mdl)["kept"] == 1
    return g, t


# ---- 1: accuracy ----
@pytest.mark.parametrize("case", [c for c in mar.CASES if c not in NOT_CONVERGED])
def test_against_exact(product_lib, oracle_lib, case):
    for k, p in enumerate(mar.problems(oracle_lib, case)):
        mdl = _model(product_lib, p)
        r = oq.solve(mdl)
        assert r.info.status == "Solved" and oq.stats(mdl)[18] == 0.0
        g, _ = _check_against_exact(case, k, p, mdl, r)
        st = oq.adjoint_stats(mdl)
        assert (st["n_low"], st["n_upp"]) == (int(np.sum(g["act"] < 0)), int(np.sum(g["act"] > 0)))
        oq.clean(mdl)


# ---- 2: one workspace, both methods ----
def test_both_methods_on_one_workspace(product_lib, oracle_lib):
    case = "control"
    p = mar.problems(oracle_lib, case)[0]
    n, m = len(p["q"]), len(p["l"])
    gx, gy = (g[0] for g in mar.incoming(case, 0, n, m))
    mdl = _model(product_lib, p, method="direct")
    r = oq.solve(mdl)
    assert r.info.status == "Solved"
    a = oq.adjoint(mdl, dx=gx, dy=gy)
    st = oq.adjoint_stats(mdl)
    assert st["kept"] == 1 and st["bytes"] > 0 and oq.derivative_iter_stats(mdl)["kept"] == 0
    oq.derivative_method(mdl, "iterative")
    assert oq.adjoint_stats(mdl)["kept"] == 0  # the call drops the kept factor
    b = oq.adjoint(mdl, dx=gx, dy=gy)
    assert oq.derivative_iter_stats(mdl)["kept"] == 1 and oq.adjoint_stats(mdl)["kept"] == 1
    oq.clean(mdl)
    assert np.array_equal(a["act"], b["act"])
    cond = np.linalg.cond(mar.dense_K(p["P"], p["A"], a["act"]))
    b_direct, b_iter = max(1000 * MEASURED[case], 1000 * cond * EPS), _bounds(case, p, a["act"])[0]
    diff = adj.rel_err(b, a)
    print(f"control, direct against iterative on one workspace: {diff:.2e} / {b_direct + b_iter:.2e}")
    assert diff <= b_direct + b_iter


# ---- 3: bit contracts ----
def test_bit_contracts(product_lib, oracle_lib):
    case = "control6_unsorted"
    p = mar.problems(oracle_lib, case)[0]
    n, m = len(p["q"]), len(p["l"])
    gx, gy = mar.incoming(case, 0, n, m, ncot=3)
    mdl = _model(product_lib, p)
    assert oq.solve(mdl).info.status == "Solved"
    multi = oq.adjoint(mdl, dx=gx, dy=gy)
    for c in range(3):
        one = oq.adjoint(mdl, dx=gx[c], dy=gy[c])
        for k in adj.GRADS:
            assert _same(one[k], multi[k][c]), (c, k)
    builds = oq.adjoint_stats(mdl)["builds"]
    tan = {name: v for name, v in mjr.tangents(case, 0, p, 3).items() if v.shape[1]}
    tm = oq.jvp(mdl, **tan)
    assert oq.adjoint_stats(mdl)["builds"] == builds == 1 and oq.derivative_iter_stats(mdl)["builds"] == 1  # a JVP after an adjoint builds nothing
    for i in range(3):
        one = oq.jvp(mdl, **{name: v[i] for name, v in tan.items()})
        assert _same(one["x"], tm["x"][i]) and _same(one["y"], tm["y"][i]), i
    # a NULL tangent has the bits of zeros
    part = oq.jvp(mdl, q=tan["q"][0], Ax=tan["Ax"][0])
    full = oq.jvp(mdl, q=tan["q"][0], l=np.zeros(m), u=np.zeros(m), Px=np.zeros(tan["Px"].shape[1]), Ax=tan["Ax"][0])
    assert _same(part["x"], full["x"]) and _same(part["y"], full["y"])
    # the device form has the bits of the host form
    dev = lambda a: DeviceArray(product_lib, a.shape[0], a.shape[1]).upload(a)
    dg = oq.adjoint(mdl, dx=dev(gx), dy=dev(gy))
    for k in adj.GRADS:
        assert _same(dg[k].numpy(), multi[k]), k
    assert np.array_equal(dg["act"].numpy().reshape(-1), multi["act"])
    dt = oq.jvp(mdl, **{name: dev(v) for name, v in tan.items()})
    assert _same(dt["x"].numpy(), tm["x"]) and _same(dt["y"].numpy(), tm["y"])
    assert oq.adjoint_stats(mdl)["builds"] == 1
    oq.clean(mdl)


# ---- 4: nothing else changes ----
def _solve_update_solve(product_lib, p, derivatives, polish, gx, gy, **method_args):
    mdl = _model(product_lib, p, method=None, polish=polish)
    if derivatives:
        oq.derivative_method(mdl, "iterative", **method_args)
    r1 = oq.solve(mdl)
    rc = None
    if derivatives:
        try:
            oq.adjoint(mdl, dx=gx, dy=gy)
            oq.jvp(mdl, q=gx, l=gy)
        except oq.OSQPError as ex:
            rc = str(ex)
    oq.update(mdl, q=p["q"] * 1.02)
    r2 = oq.solve(mdl)
    cg = oq.stats(mdl)[6]
    oq.clean(mdl)
    return r1, r2, cg, rc


_B_runs = {}


def _plain(product_lib, oracle_lib, polish):
    """Model B of test 4 (solve, update(q), solve without a derivative call), once per polish setting."""
    if polish not in _B_runs:
        p = mar.problems(oracle_lib, "control")[0]
        _B_runs[polish] = _solve_update_solve(product_lib, p, False, polish, None, None)
    return _B_runs[polish]


@pytest.mark.parametrize("polish", [False, True])
def test_nothing_else_changes(product_lib, oracle_lib, polish):
    p = mar.problems(oracle_lib, "control")[0]
    gx, gy = (g[0] for g in mar.incoming("control", 0, len(p["q"]), len(p["l"])))
    a1, a2, cg_a, failed = _solve_update_solve(product_lib, p, True, polish, gx, gy)
    b1, b2, cg_b, _ = _plain(product_lib, oracle_lib, polish)
    assert failed is None
    assert _same(a1.x, b1.x) and _same(a1.y, b1.y) and a1.info.iter == b1.info.iter
    assert a2.info.status == b2.info.status == "Solved"
    assert _same(a2.x, b2.x) and _same(a2.y, b2.y) and a2.info.iter == b2.info.iter and a2.info.rho_updates == b2.info.rho_updates
    assert cg_a == cg_b  # the derivative's CG iterations are counted in derivative_iter_stats, not here


# ---- 5: the default is untouched ----
def _raw_adjoint(lib, mdl, n, m):
    """osqp_amd_adjoint called directly with sentinel-filled outputs: (return code, message, outputs)."""
    st = oq.stats(mdl, 4)
    sizes = dict(q=n, l=m, u=m, Px=int(st[3]), Ax=int(st[1]))
    outs = {k: np.full(max(1, v), SENTINEL) for k, v in sizes.items()}
    outs["act"] = np.full(max(1, m), SENTINEL)
    f = oq.interface._fptr
    rc = lib.osqp_amd_adjoint(mdl.workspace, 1, f(np.ones(n)), f(np.ones(max(1, m))), *(f(outs[k]) for k in adj.GRADS), f(outs["act"]))
    return rc, lib.osqp_amd_last_error().decode(), outs


@pytest.fixture(scope="module")
def compact_run(product_lib, oracle_lib):
    """The compact shape of the existing refusal tests, solved once: everything tests 5 and 6 read from it."""
    keep = {k: os.environ.get(k) for k in COMPACT_ENV}
    os.environ.update(COMPACT_ENV)
    try:
        mdl = oq.Model(product_lib)
        oq.setup_generated(mdl, 0, 40000, 96, 21, **COMPACT_OPTS)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    n, m = oq.dimensions(mdl)
    out = dict(n=n, m=m, stats18=oq.stats(mdl)[18], layouts=[oq.spmv_layout(mdl, w) for w in (0, 1, 2)])
    r = oq.solve(mdl)
    out["r"] = r
    out["default"] = _raw_adjoint(product_lib, mdl, n, m)
    oq.derivative_method(mdl, "direct")
    out["direct"] = _raw_adjoint(product_lib, mdl, n, m)
    oq.derivative_method(mdl, "auto")
    rng = np.random.default_rng(6)
    gx, gy = rng.standard_normal(n), rng.standard_normal(m)
    out.update(gx=gx, gy=gy)
    out["g"] = oq.adjoint(mdl, dx=gx, dy=gy)
    out["g2"] = oq.adjoint(mdl, dx=gx, dy=gy, want=("Px", "Ax"))
    out["iter_stats"] = oq.derivative_iter_stats(mdl)
    d = dict(q=rng.standard_normal(n), l=rng.standard_normal(m), u=rng.standard_normal(m))
    out["d"], out["t"] = d, oq.jvp(mdl, **d)
    out["builds"] = oq.adjoint_stats(mdl)["builds"]
    try:
        oq.jvp(mdl, q=d["q"], Ax=np.zeros(int(oq.stats(mdl, 4)[1])))
        out["matrix_tangent"] = "served"
    except oq.OSQPError as ex:
        out["matrix_tangent"] = str(ex)
    xd, yd = oq.solution(mdl)
    out["x_dev"], out["y_dev"] = np.array(xd.numpy()).reshape(-1), np.array(yd.numpy()).reshape(-1)
    oq.clean(mdl)
    d = oracle_lib.oracle_generate(0, 40000, 96, 21)
    out["data"] = _data_to_scipy(d.contents)
    oracle_lib.oracle_data_free(d)
    return out


def test_default_untouched(product_lib, oracle_lib, compact_run):
    c = compact_run
    assert c["stats18"] == 1.0 and all(l["compact"] == 1 for l in c["layouts"]) and c["r"].info.status == "Solved"
    for name in ("default", "direct"):
        rc, msg, outs = c[name]
        print(f"{name}: refused with {rc}: {msg}")
        assert rc == 6 and "compact" in msg and "osqp_amd_adjoint" in msg and "osqp_amd_derivative_method" in msg
        assert all(np.all(v == SENTINEL) for v in outs.values())
    assert c["iter_stats"]["kept"] == 1 and c["iter_stats"]["builds"] == 1  # "auto" on the compact workspace: served, iteratively
    # a small model on the direct back-end: "auto" keeps a factor, "iterative" is refused and names the back-end
    p = mar.problems(oracle_lib, "control6_unsorted")[0]
    gx, gy = (g[0] for g in mar.incoming("control6_unsorted", 0, len(p["q"]), len(p["l"])))
    mdl = _model(product_lib, p, method="auto", linsys="direct")
    assert oq.solve(mdl).info.status == "Solved"
    oq.adjoint(mdl, dx=gx, dy=gy)
    assert oq.derivative_iter_stats(mdl)["kept"] == 0 and oq.adjoint_stats(mdl)["kept"] == 1 and oq.adjoint_stats(mdl)["bytes"] > 0
    with pytest.raises(oq.OSQPError, match="direct back-end"):
        oq.derivative_method(mdl, "iterative")
    assert product_lib.osqp_amd_derivative_method(mdl.workspace, 2, 0, 0.0) == 6
    assert product_lib.osqp_amd_derivative_method(mdl.workspace, 3, 0, 0.0) == 1
    assert product_lib.osqp_amd_derivative_method(mdl.workspace, 1, -1, 0.0) == 1
    assert product_lib.osqp_amd_derivative_method(mdl.workspace, 1, 0, 1.5) == 1
    oq.clean(mdl)


# ---- 6: the compact shape, without a factorisation as reference ----
def test_compact_shape(compact_run):
    c = compact_run
    P, q, A, l, u = c["data"]
    n, m, g, gx, gy = c["n"], c["m"], c["g"], c["gx"], c["gy"]
    Pf, Ac = (sp.triu(P) + sp.triu(P, 1).T).tocsr(), sp.csr_matrix(A)
    act = g["act"]
    mask = act != 0
    # (a) the residual of K [r_x; r_a] = [g_x; (g_y)_a] from the returned dq, dl, du, act
    rx, ry = -g["q"], g["l"] + g["u"]
    assert np.all(ry[~mask] == 0.0) and np.all(g["l"][act >= 0] == 0.0) and np.all(g["u"][act <= 0] == 0.0)
    r1, r2 = Pf @ rx + Ac.T @ ry - gx, np.where(mask, Ac @ rx - gy, 0.0)
    res = max(np.max(np.abs(r1)), np.max(np.abs(r2))) / max(np.max(np.abs(gx)), np.max(np.abs(gy[mask])))
    bound = max(1000 * COMPACT_MODEL_RESIDUAL, 1e-12)
    it = c["iter_stats"]
    print(f"compact n {n} m {m} active {int(np.sum(act < 0))} / {int(np.sum(act > 0))}: residual {res:.2e} / {bound:.2e}  outer {it['last_outer_steps']} "
          f"drop {it['last_drop']:.1e} cg {it['cg_iters']} state bytes {it['bytes']}")
    assert res <= bound
    # (b) dPx, dAx recomputed from the returned vectors and solution() by the two formulas, entry by entry
    x, y = c["x_dev"], c["y_dev"]
    assert _same(x, c["r"].x) and _same(y, c["r"].y)
    (pi, pj), (ai, aj) = adj.patterns(P, A)
    t1, t2 = rx[pi] * x[pj], rx[pj] * x[pi]
    wantP = np.where(pi == pj, -t1, -(t1 + t2))
    tolP = 8 * EPS * np.where(pi == pj, np.abs(t1), np.abs(t1) + np.abs(t2))
    a1, a2 = y[ai] * rx[aj], ry[ai] * x[aj]
    wantA, tolA = -(a1 + a2), 8 * EPS * (np.abs(a1) + np.abs(a2))
    worstP, worstA = np.max(np.abs(g["Px"] - wantP) - tolP), np.max(np.abs(g["Ax"] - wantA) - tolA)
    print(f"dPx: {len(pi)} entries, worst excess {worstP:.2e}; dAx: {len(ai)} entries, worst excess {worstA:.2e} (<= 0: within 8 eps of the terms)")
    assert np.all(np.abs(g["Px"] - wantP) <= tolP) and np.all(np.abs(g["Ax"] - wantA) <= tolA)
    assert _same(c["g2"]["Px"], g["Px"]) and _same(c["g2"]["Ax"], g["Ax"])  # two calls, the same bits
    # (c) JVP with tq, tl, tu: duality with (a)'s adjoint; tPx / tAx are refused on a compact workspace
    t, d = c["t"], c["d"]
    gap = jv.duality_gap(gx, gy, t["x"], t["y"], g, d)
    print(f"duality gap {gap:.2e} / {bound:.2e}; matrix tangent: {c['matrix_tangent']}")
    assert gap <= bound and np.array_equal(t["act"], act) and c["builds"] == 1
    assert "compact" in c["matrix_tangent"] and "osqp_amd_jvp" in c["matrix_tangent"]


# ---- 7: small compact shapes for the kernel's edges ----
@pytest.mark.parametrize("case,shift,group", [("control6_unsorted", 6, 1), ("control", 6, 3), ("svm", 8, 2), ("equality_qp", 8, 1)])
def test_small_compact_shapes(product_lib, oracle_lib, monkeypatch, case, shift, group):
    """Panels of 64 / 256 columns: control6_unsorted goes through A_to_sorted; control at 3 panels per group has m = 616 rows
    (a last slice of 40 lanes) and ragged groups (6 and 10 panels); equality_qp at 256 columns compacts A and P but not A'."""
    for k, v in dict(COMPACT_ENV, OSQP_AMD_PANEL_SHIFT=shift, OSQP_AMD_PANEL_GROUP=group).items():
        monkeypatch.setenv(k, str(v))
    p = mar.problems(oracle_lib, case)[0]
    mdl = _model(product_lib, p, method="auto")
    lays = [oq.spmv_layout(mdl, w) for w in (0, 1, 2)]
    assert oq.stats(mdl)[18] == 1.0 and lays[0]["compact"] == 1 and lays[2]["compact"] == 1
    assert all(l["compact"] == 1 for l in lays) or case == "equality_qp"
    assert lays[0]["Gp"] == group
    r = oq.solve(mdl)
    assert r.info.status == "Solved"
    n, m = len(p["q"]), len(p["l"])
    gx, gy = (g[0] for g in mar.incoming(case, 0, n, m))
    g = oq.adjoint(mdl, dx=gx, dy=gy)
    d = {name: v for name, v in _direction(case, 0, p).items() if name in ("q", "l", "u")}
    t = oq.jvp(mdl, **d)
    it = oq.derivative_iter_stats(mdl)
    oq.clean(mdl)
    b_exact, b_dual, cond = _bounds(case, p, g["act"])
    err_a = adj.rel_err(g, mar.caller_order(p, adj.exact(p["P"], p["A"], r.x, r.y, g["act"], gx, gy)))
    tx, ty = jv.exact(p["P"], p["A"], r.x, r.y, t["act"], d)
    err_j, gap = jv.rel_err(t["x"], t["y"], tx, ty), jv.duality_gap(gx, gy, t["x"], t["y"], g, d)
    print(f"{case} shift {shift} group {group}: B {[l['B'] for l in lays]} tiles {[l['tiles'] for l in lays]}  adjoint {err_a:.2e} jvp {err_j:.2e} / {b_exact:.2e}  "
          f"duality {gap:.2e} / {b_dual:.2e}  outer {it['last_outer_steps']}")
    assert it["kept"] == 1 and err_a <= b_exact and err_j <= b_exact and gap <= b_dual


def test_only_the_transpose_compact(product_lib, oracle_lib, monkeypatch):
    """svm (n = 320, m = 600) at panels of 512 columns: only A' (600 columns) gets panels and goes compact.  dPx goes the CSR
    way on a workspace that counts as compact; dAx has neither A's slices nor the column array of A' and is refused with 6
    before anything is written."""
    for k, v in dict(COMPACT_ENV, OSQP_AMD_PANEL_SHIFT=9).items():
        monkeypatch.setenv(k, str(v))
    case = "svm"
    p = mar.problems(oracle_lib, case)[0]
    n, m = len(p["q"]), len(p["l"])
    mdl = _model(product_lib, p, method="auto")
    assert [oq.spmv_layout(mdl, w)["compact"] for w in (0, 1, 2)] == [0, 1, 0] and oq.stats(mdl)[18] == 1.0
    r = oq.solve(mdl)
    assert r.info.status == "Solved"
    gx, gy = (g[0] for g in mar.incoming(case, 0, n, m))
    g = oq.adjoint(mdl, dx=gx, dy=gy, want=("q", "l", "u", "Px"))
    rc, msg, outs = _raw_adjoint(product_lib, mdl, n, m)
    oq.clean(mdl)
    print(f"dAx: returned {rc}: {msg}")
    assert rc == 6 and "dAx" in msg and all(np.all(v == SENTINEL) for v in outs.values())
    want = adj.exact(p["P"], p["A"], r.x, r.y, g["act"], gx, gy)
    err = adj.rel_err(dict(g, Ax=want["Ax"]), want)
    bound = _bounds(case, p, g["act"])[0]
    print(f"svm, only A' compact: q, l, u, Px against exact {err:.2e} / {bound:.2e}")
    assert err <= bound


# ---- 8: non-convergence ----
def test_non_convergence(product_lib, oracle_lib):
    p = mar.problems(oracle_lib, "control")[0]
    n, m = len(p["q"]), len(p["l"])
    gx, gy = (g[0] for g in mar.incoming("control", 0, n, m))
    mdl = _model(product_lib, p, method=None, polish=False, polish_refine_iter=0)
    oq.derivative_method(mdl, "iterative", max_outer=1)
    r1 = oq.solve(mdl)
    rc, msg, outs = _raw_adjoint(product_lib, mdl, n, m)
    print(f"returned {rc}: {msg}")
    assert rc == 4 and "osqp_amd_adjoint" in msg and "1.000e+00" in msg and "rn / first_norm" in msg
    assert all(np.all(v == SENTINEL) for v in outs.values())
    it = oq.derivative_iter_stats(mdl)
    assert it["last_outer_steps"] == 1 and it["last_drop"] == 1.0
    with pytest.raises(oq.OSQPError, match="did not converge"):
        oq.jvp(mdl, q=gx)
    # the workspace is still usable: update, solve gives the bits of the model that never differentiated
    oq.update(mdl, q=p["q"] * 1.02)
    r2 = oq.solve(mdl)
    cg = oq.stats(mdl)[6]
    oq.clean(mdl)
    ref = oq.Model(product_lib)
    oq.setup(ref, **mar.setup_args(p), **dict(OPTS, polish=False, linsys_solver="pcg", polish_refine_iter=0))
    b1 = oq.solve(ref)
    oq.update(ref, q=p["q"] * 1.02)
    b2 = oq.solve(ref)
    cg_b = oq.stats(ref)[6]
    oq.clean(ref)
    assert _same(r1.x, b1.x) and _same(r2.x, b2.x) and _same(r2.y, b2.y) and r2.info.iter == b2.info.iter and cg == cg_b
