"""Dual objective, duality gap and the gap stopping rule of a single model on the GPU (osqp_amd_duality,
osqp_amd_duality_gap_check).

Values are compared with the numpy statement (duality_ref.py) on the pair the engine returned, at the derived rounding
bound 4 (N + 8) 2^-53 S.  Where the rule moves the end of a solve is decided by the CPU procedure of duality_cases.rule_trace
(the oracle's iterates and numpy), never by the engine."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import osqp_jl_amd as oq
import duality_cases
import duality_ref
import qp_cases

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ITERATE_TOL = 1e-9  # test_gpu_parity.test_iterates_match_oracle_early


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def model(lib, prob, **settings):
    m = oq.Model(lib)
    oq.setup(m, **prob, **settings)
    return m


def check_values(prob, x, y, d, what=""):
    ref = duality_ref.duality(prob["P"], prob["q"], prob["A"], prob["l"], prob["u"], x, y)
    tol = duality_ref.tolerance(ref)
    for key in ("prim_obj", "dual_obj", "gap"):
        err = abs(d[key] - ref[key])
        print(f"{what} {key}: engine {d[key]:.17g} numpy {ref[key]:.17g} |diff| {err:.3e} tol {tol:.3e} (N {ref['N']}, S {ref['S']:.6g})")
    for key in ("prim_obj", "dual_obj", "gap"):
        assert abs(d[key] - ref[key]) <= tol, (what, key, d[key], ref[key], tol)
    return ref


# ---- 1. values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled_termination", [0, 1])
@pytest.mark.parametrize("scaling", [0, 10])
@pytest.mark.parametrize("linsys", ["direct", "pcg"])
@pytest.mark.parametrize("name", list(duality_cases.VALUE_CASES))
def test_values_against_numpy(product_lib, name, linsys, scaling, scaled_termination):
    prob = duality_cases.VALUE_CASES[name]()
    m = model(product_lib, prob, verbose=False, adaptive_rho_interval=25, linsys_solver=linsys, scaling=scaling,
              scaled_termination=bool(scaled_termination), polish=name in duality_cases.POLISHED)
    r = oq.solve(m)
    assert r.info.status in ("Solved", "Solved_inaccurate", "Max_iter_reached"), r.info.status
    d = oq.duality(m)
    assert d["rule"] is False and d["gap_refusals"] == 0 and np.isnan(d["eps_gap"])
    ref = check_values(prob, r.x, r.y, d, f"{name}/{linsys}/s{scaling}/t{scaled_termination} ({r.info.status}, polish {r.info.status_polish})")
    assert abs(d["prim_obj"] - r.info.obj_val) <= duality_ref.tolerance(ref)  # info.obj_val: the same terms, summed by another kernel
    oq.clean(m)


# ---- 2. the rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(duality_cases.RULE_CASES))
def test_rule_moves_the_end_of_the_solve(product_lib, oracle_lib, name):
    t = duality_cases.rule_trace(oq, oracle_lib, name)
    settings = dict(duality_cases.RULE_SETTINGS, linsys_solver="direct", **t["extra"])
    off = model(product_lib, t["prob"], **settings)
    r = oq.solve(off)
    print(f"{name}: rule off {r.info.status} at {r.info.iter} (oracle {t['K_off']})")
    assert r.info.status == "Solved" and r.info.iter == t["K_off"]
    oq.clean(off)
    on = model(product_lib, t["prob"], **settings)
    oq.duality_gap_check(on, True)
    r = oq.solve(on)
    d = oq.duality(on)
    print(f"{name}: rule on {r.info.status} at {r.info.iter} (procedure {t['K_on']}), refusals {d['gap_refusals']}, gap {d['gap']:.3e} eps_gap {d['eps_gap']:.3e}")
    assert r.info.status == "Solved" and r.info.iter == t["K_on"]
    assert d["rule"] is True and d["gap_refusals"] >= 1
    assert d["gap_refusals"] <= (t["K_on"] - t["K_off"]) // duality_cases.CHECK  # the gap can refuse only where it is above its bound
    assert abs(d["gap"]) < d["eps_gap"]
    ora = t["checks"][t["K_on"]]
    ex, ey = np.max(np.abs(r.x - ora["x"])), np.max(np.abs(r.y - ora["y"]))
    print(f"{name}: max|x - oracle| {ex:.3e} max|y - oracle| {ey:.3e}")
    assert ex <= ITERATE_TOL and ey <= ITERATE_TOL
    oq.clean(on)


# ---- 3. the approximate pass ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["one_check_short_of_K_on", "K_off"])
@pytest.mark.parametrize("name", list(duality_cases.RULE_CASES))
def test_approximate_pass_at_the_iteration_limit(product_lib, oracle_lib, name, where):
    t = duality_cases.rule_trace(oq, oracle_lib, name)
    k = t["K_on"] - duality_cases.CHECK if where == "one_check_short_of_K_on" else t["K_off"]
    ratio = t["checks"][k]["gap"]  # |gap| / eps_gap at eps: the 10 eps test holds iff it is below 10
    assert abs(ratio - 10.0) > 0.1 and ratio > 1.0
    m = model(product_lib, t["prob"], **dict(duality_cases.RULE_SETTINGS, linsys_solver="direct", max_iter=k, **t["extra"]))
    oq.duality_gap_check(m, True)
    r = oq.solve(m)
    print(f"{name}: max_iter {k} gap ratio {ratio:.3f} -> {r.info.status}")
    assert r.info.iter == k
    assert r.info.status == ("Solved_inaccurate" if ratio < 10.0 else "Max_iter_reached")
    oq.clean(m)


# ---- 4. off is the parent ------------------------------------------------------------------------------------------------
def _same(a, b):
    return a.info.iter == b.info.iter and a.info.status == b.info.status and np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y)


@pytest.mark.parametrize("linsys", ["direct", "pcg"])
def test_off_is_bitwise_the_model_that_never_heard_of_the_rule(product_lib, oracle_lib, linsys):
    t = duality_cases.rule_trace(oq, oracle_lib, "huber")
    settings = dict(duality_cases.RULE_SETTINGS, linsys_solver=linsys)
    rng = np.random.default_rng(3)
    a = model(product_lib, t["prob"], **settings)
    b = model(product_lib, t["prob"], **settings)
    oq.duality_gap_check(b, False)
    a1, b1 = oq.solve(a), oq.solve(b)
    assert _same(a1, b1)
    x0, y0 = a1.x + 1e-2 * rng.standard_normal(a1.x.size), a1.y.copy()
    oq.duality_gap_check(b, True); oq.duality_gap_check(b, False)  # on -> off between solves
    oq.warm_start(a, x=x0, y=y0); oq.warm_start(b, x=x0, y=y0)
    a2, b2 = oq.solve(a), oq.solve(b)
    assert _same(a2, b2)
    oq.duality_gap_check(b, True)
    oq.update_settings(a, eps_abs=1e-4, eps_rel=1e-4); oq.update_settings(b, eps_abs=1e-4, eps_rel=1e-4)
    assert oq.duality(b)["rule"] is True  # survives a settings update
    oq.duality_gap_check(b, False)
    a3, b3 = oq.solve(a), oq.solve(b)
    assert _same(a3, b3) and a3.info.iter > 0
    oq.clean(a); oq.clean(b)


def test_toggling_and_settings_updates_keep_the_rule_working(product_lib, oracle_lib):
    t = duality_cases.rule_trace(oq, oracle_lib, "huber")
    settings = dict(duality_cases.RULE_SETTINGS, linsys_solver="direct")
    # each from a fresh model: a solve leaves its adapted rho behind, so a second solve of one model counts differently
    for toggles, update, expect in (((True, False, True), False, "K_on"), ((True,), True, "K_on"), ((True, False), True, "K_off")):
        m = model(product_lib, t["prob"], **settings)
        for on in toggles:
            oq.duality_gap_check(m, on)
        if update:
            oq.update_settings(m, max_iter=3000)
        r = oq.solve(m)
        assert r.info.status == "Solved" and r.info.iter == t[expect], (toggles, update, r.info.status, r.info.iter)
        assert oq.duality(m)["rule"] is toggles[-1]
        oq.clean(m)


# ---- 5. osqp_amd_iterate, then duality -----------------------------------------------------------------------------------
@pytest.mark.parametrize("linsys", ["direct", "pcg"])
def test_duality_of_the_current_iterate(product_lib, linsys):
    prob = duality_cases.VALUE_CASES["svm"]()
    m = model(product_lib, prob, verbose=False, adaptive_rho_interval=25, linsys_solver=linsys)
    assert product_lib.osqp_amd_iterate(m.workspace, 30) == 0
    n, mm = oq.dimensions(m)
    x, y = np.zeros(n), np.zeros(mm)
    assert product_lib.osqp_amd_get_iterate(m.workspace, fptr(x), fptr(y)) == 0
    check_values(prob, x, y, oq.duality(m), f"iterate/{linsys}")
    oq.clean(m)


# ---- 6. read-only --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [False, True])
@pytest.mark.parametrize("linsys", ["direct", "pcg"])
def test_duality_changes_nothing(product_lib, linsys, rule):
    prob = duality_cases.VALUE_CASES["portfolio"]()
    res = []
    for ask in (True, False):
        m = model(product_lib, prob, verbose=False, adaptive_rho_interval=25, eps_abs=1e-5, eps_rel=1e-5, linsys_solver=linsys)
        if rule:
            oq.duality_gap_check(m, True)
        first = oq.solve(m)
        if ask:
            d1, d2 = oq.duality(m), oq.duality(m)
            assert d1["prim_obj"] == d2["prim_obj"] and d1["dual_obj"] == d2["dual_obj"] and d1["gap"] == d2["gap"]  # the same bits on every call
        oq.update_q(m, prob["q"] * 1.01)
        second = oq.solve(m)
        res.append((first, second, oq.stats(m).copy()))
        oq.clean(m)
    assert _same(res[0][0], res[1][0]) and _same(res[0][1], res[1][1])
    assert np.array_equal(res[0][2][6:9], res[1][2][6:9])  # CG iterations, ADMM iterations, factorisations


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(product_lib):
    buf = np.zeros(6)
    assert product_lib.osqp_amd_duality_gap_check(None, 1) == 7
    assert product_lib.osqp_amd_duality(None, fptr(buf), 6) == 7
    m = model(product_lib, duality_cases.VALUE_CASES["unconstrained"](), verbose=False)
    assert product_lib.osqp_amd_duality(m.workspace, fptr(buf), 6) == 1 and b"osqp_solve" in product_lib.osqp_amd_last_error()
    assert product_lib.osqp_amd_duality_gap_check(m.workspace, 2) == 1 and product_lib.osqp_amd_duality_gap_check(m.workspace, -1) == 1
    with pytest.raises(oq.OSQPError):
        oq.duality(m)
    with pytest.raises(ValueError):
        oq.duality_gap_check(m, 1)
    assert product_lib.osqp_amd_duality_gap_check(m.workspace, 1) == 0 and product_lib.osqp_amd_duality_gap_check(m.workspace, 0) == 0
    oq.clean(m)


def test_a_row_sharded_workspace_is_refused(tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = str(s.getsockname()[1]); s.close()
    out = str(tmp_path / "out.json")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_duality_sharded_worker.py"), str(r), "2", port, out],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode(errors="replace"))
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, logs[r][-4000:])
    for r in range(2):
        rec = json.load(open("%s.%d" % (out, r)))
        assert rec["check"] == 6 and "row-sharded" in rec["check_msg"] and "osqp_amd_duality_gap_check" in rec["check_msg"], rec
        assert rec["duality"] == 6 and "row-sharded" in rec["duality_msg"] and "osqp_amd_duality:" in rec["duality_msg"], rec


# ---- 8. statuses without a solution --------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [False, True])
@pytest.mark.parametrize("golden,options,status", [("G16", "prim_inf_options", "Primal_infeasible"), ("G13", "dual_inf_options", "Dual_infeasible")])
def test_no_solution_gives_nan(product_lib, golden, options, status, rule):
    m = model(product_lib, qp_cases._case_from(qp_cases.KA[golden]), linsys_solver="direct", **qp_cases.KA[options])
    if rule:
        oq.duality_gap_check(m, True)
    r = oq.solve(m)
    assert r.info.status == status
    d = oq.duality(m)
    assert np.isnan(d["dual_obj"]) and np.isnan(d["gap"]) and d["prim_obj"] == r.info.obj_val
    oq.clean(m)
