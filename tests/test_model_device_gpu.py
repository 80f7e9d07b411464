"""Device-pointer forms of a single model's life cycle (osqp_amd_update_vectors_dev, _update_values_dev, _warm_start_dev,
_solution_dev, _adjoint_dev, _jvp_dev: include/osqp_amd.h; `interface.update` / `warm_start` /
`solution` / `adjoint` / `jvp` with device arrays).

Every comparison is `array_equal`: a device form is its host twin with the copy removed -- the same kernels in the same
order on the same operands -- so there is no tolerance anywhere.  The reference of every test is the host form on a twin
model (or on the same model, for the derivatives, which share one kept factor)."""
import numpy as np
import pytest
import scipy.sparse as sp

import osqp_jl_amd as oq
import model_adjoint_ref as mar
from batch_resident_ref import OPTS
from test_gpu_parity import _data_to_scipy

pytestmark = pytest.mark.gpu

GRADS = ("q", "l", "u", "Px", "Ax")
NO_CALLS = dict(update_vectors=0, update_values=0, warm_start=0, solution=0, adjoint=0, jvp=0)
SENTINEL = -7.25


def _torch():
    import torch

    return torch


def _dev(a):
    torch = _torch()
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), dtype=torch.float64, device="cuda:0")


def _host(t):
    return t.cpu().numpy()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _model(product_lib, p, **opts):
    mdl = oq.Model(product_lib)
    oq.setup(mdl, **mar.setup_args(p), **dict(OPTS, polish=True, **opts))
    return mdl


def _values(p):
    """(Px, Ax) in the nnz order `update` takes: the sorted upper triangle of P, the caller's own arrays of A."""
    Pt = sp.triu(sp.csc_matrix(p["P"]), format="csc")
    Pt.sort_indices()
    A = p["A_given"] if "A_given" in p else p["A"]
    return np.array(Pt.data, dtype=np.float64), np.array(A.data, dtype=np.float64)


def _perturbed(p):
    """The fixed perturbation of the life-cycle test: values x 1.01, q + 0.1, bounds widened by 0.05."""
    Px, Ax = _values(p)
    return dict(q=p["q"] + 0.1, l=p["l"] - 0.05, u=p["u"] + 0.05, Px=Px * 1.01, Ax=Ax * 1.01)


def _iterate(lib, mdl):
    n, m = oq.dimensions(mdl)
    x, y = np.full(n, np.nan), np.full(max(1, m), np.nan)
    f = oq.interface._fptr
    assert lib.osqp_amd_get_iterate(mdl.workspace, f(x), f(y)) == 0
    return x, y[:m]


def _equal_results(a, b):
    return _same(a.x, b.x) and _same(a.y, b.y) and a.info.iter == b.info.iter and a.info.status == b.info.status


LIFE = [("control6_unsorted", 10), ("control6_unsorted", 0), ("tiny", 10), ("spd7", 10), ("grid2d", 10)]


@pytest.mark.parametrize("case,scaling", LIFE)
def test_life_cycle_bit_for_bit(product_lib, oracle_lib, case, scaling):
    """Twin models: A takes new q, l, u, Px, Ax through the host forms, B the same numbers as tensors; the solves that follow
    are equal bit for bit, `solution(B)` is B's result, and only B has served device-form calls."""
    p = mar.problems(oracle_lib, case)[0]
    new = _perturbed(p)
    A, B = _model(product_lib, p, scaling=scaling), _model(product_lib, p, scaling=scaling)
    assert _equal_results(oq.solve(A), oq.solve(B))
    oq.update(A, **new)
    oq.update(B, **{k: _dev(v) for k, v in new.items()})
    ra, rb = oq.solve(A), oq.solve(B)
    print(f"{case} scaling {scaling}: {ra.info.status} in {ra.info.iter} / {rb.info.status} in {rb.info.iter} iterations")
    assert ra.info.status == "Solved"
    assert _same(ra.x, rb.x) and _same(ra.y, rb.y)
    assert ra.info.iter == rb.info.iter and ra.info.status == rb.info.status
    x, y = oq.solution(B, x=_dev(np.full(len(p["q"]), np.nan)), y=_dev(np.full(len(p["l"]), np.nan)))
    assert _same(_host(x), rb.x) and _same(_host(y), rb.y)
    x2, y2 = oq.solution(B, x=x)  # y allocated beside x
    assert x2 is x and _same(_host(y2), rb.y)
    assert oq.device_form_calls(B) == dict(NO_CALLS, update_vectors=1, update_values=1, solution=2)
    assert oq.device_form_calls(A) == NO_CALLS
    oq.clean(A); oq.clean(B)


def test_solution_before_a_solve_and_after_an_update(product_lib, oracle_lib):
    p = mar.problems(oracle_lib, "control6_unsorted")[0]
    mdl = _model(product_lib, p)
    x = _dev(np.full(len(p["q"]), SENTINEL))
    with pytest.raises(oq.OSQPError, match="osqp_solve"):
        oq.solution(mdl, x=x)
    oq.solve(mdl)
    oq.update(mdl, q=_dev(p["q"] * 1.5))
    with pytest.raises(oq.OSQPError, match="osqp_solve"):
        oq.solution(mdl, x=x)
    assert np.all(_host(x) == SENTINEL)
    oq.clean(mdl)


def test_warm_start(product_lib, oracle_lib):
    """Host form and device form from the same (x, y): the same iterate bits and the same next solve; the x-only and y-only
    rules (the other block is zeroed) as well."""
    case = "control6_unsorted"
    p = mar.problems(oracle_lib, case)[0]
    A, B = _model(product_lib, p), _model(product_lib, p)
    r = oq.solve(A)
    assert _equal_results(r, oq.solve(B))
    x0, y0 = 0.9 * r.x, 1.1 * r.y
    for k, given in enumerate((dict(x=x0, y=y0), dict(x=x0), dict(y=y0))):
        oq.warm_start(A, **given)
        oq.warm_start(B, **{name: _dev(v) for name, v in given.items()})
        (xa, ya), (xb, yb) = _iterate(product_lib, A), _iterate(product_lib, B)
        assert _same(xa, xb) and _same(ya, yb), sorted(given)
        if "x" not in given:
            assert not np.any(xb)
        if "y" not in given:
            assert not np.any(yb)
        ra, rb = oq.solve(A), oq.solve(B)
        print(f"warm start {sorted(given)}: {ra.info.iter} / {rb.info.iter} iterations")
        assert _equal_results(ra, rb), sorted(given)
        assert oq.device_form_calls(B)["warm_start"] == k + 1
    assert oq.device_form_calls(A) == NO_CALLS
    oq.clean(A); oq.clean(B)


def test_bounds_are_validated_on_the_device_and_the_mirror_stays_truthful(product_lib, oracle_lib):
    case = "control6_unsorted"
    p = mar.problems(oracle_lib, case)[0]
    l, u = p["l"], p["u"]
    i = int(np.flatnonzero(np.isfinite(l) & np.isfinite(u))[0])

    def one(v, at, value):
        w = v.copy()
        w[at] = value
        return w

    # a device l with one entry above the STORED u: refused, and nothing has changed
    A, B = _model(product_lib, p), _model(product_lib, p)
    with pytest.raises(oq.OSQPError):
        oq.update(B, l=_dev(one(l, i, u[i] + 1.0)))
    with pytest.raises(oq.OSQPError):  # l and u together, q with them: q is not touched either
        oq.update(B, q=_dev(p["q"] * 3.0), l=_dev(one(l, i, u[i] + 1.0)), u=_dev(u))
    assert oq.device_form_calls(B) == NO_CALLS
    assert _equal_results(oq.solve(A), oq.solve(B))
    oq.clean(A); oq.clean(B)
    # device u, then host l: validated against the NEW u
    B = _model(product_lib, p)
    oq.update(B, u=_dev(u + 1.0))
    with pytest.raises(oq.OSQPError):
        oq.update_l(B, one(l, i, u[i] + 1.5))
    oq.update_l(B, one(l, i, u[i] + 0.5))  # violates only the old u
    # ... and the host-given l is what the next device-form u is held against
    with pytest.raises(oq.OSQPError):
        oq.update(B, u=_dev(one(u + 1.0, i, u[i] + 0.25)))
    oq.update(B, u=_dev(one(u + 1.0, i, u[i] + 0.75)))
    oq.clean(B)
    # the other way round: device l, then host u
    B = _model(product_lib, p)
    oq.update(B, l=_dev(l - 1.0))
    with pytest.raises(oq.OSQPError):
        oq.update_u(B, one(u, i, l[i] - 1.5))
    oq.update_u(B, one(u, i, l[i] - 0.5))  # violates only the old l
    with pytest.raises(oq.OSQPError):
        oq.update(B, l=_dev(one(l - 1.0, i, l[i] - 0.25)))
    oq.update(B, l=_dev(one(l - 1.0, i, l[i] - 0.75)))
    # the mixture ends in the state the host forms alone reach
    A = _model(product_lib, p)
    oq.update_l(A, l - 1.0); oq.update_u(A, one(u, i, l[i] - 0.5)); oq.update_l(A, one(l - 1.0, i, l[i] - 0.75))
    assert _equal_results(oq.solve(A), oq.solve(B))
    oq.clean(A); oq.clean(B)


def _raw_adjoint(lib, mdl, dx, outs, act):
    rc = lib.osqp_amd_adjoint_dev(mdl.workspace, 1, dx.data_ptr(), None, *(outs[k].data_ptr() if k in outs else None for k in GRADS), act.data_ptr())
    return rc, lib.osqp_amd_last_error().decode()


def test_compact_workspace(product_lib, oracle_lib, monkeypatch):
    """The shape tests/test_model_adjoint_gpu.py forces a compact workspace at: the life-cycle calls serve it through the slot
    maps, the derivative calls refuse it with 6 and have written nothing."""
    torch = _torch()
    monkeypatch.setenv("OSQP_AMD_PANEL", "2")
    monkeypatch.setenv("OSQP_AMD_COMPACT_NNZ", "0")
    n, per_row, seed = 40000, 96, 21
    d = oracle_lib.oracle_generate(0, n, per_row, seed)
    P, q, Amat, l, u = _data_to_scipy(d.contents)
    oracle_lib.oracle_data_free(d)
    Amat = sp.csc_matrix(Amat); Amat.sort_indices()
    new = dict(q=q + 0.1, l=np.maximum(l - 0.05, -oq.OSQP_INFTY), u=np.minimum(u + 0.05, oq.OSQP_INFTY), Ax=np.array(Amat.data) * 1.01)
    models = []
    for _ in range(2):
        mdl = oq.Model(product_lib)
        oq.setup_generated(mdl, 0, n, per_row, seed, verbose=False, eps_abs=1e-5, eps_rel=1e-5, adaptive_rho_interval=25, linsys_solver="pcg")
        assert oq.stats(mdl)[18] == 1.0
        assert int(oq.stats(mdl, 4)[1]) == Amat.nnz
        models.append(mdl)
    A, B = models
    oq.update(A, **new)
    oq.update(B, **{k: _dev(v) for k, v in new.items()})
    ra, rb = oq.solve(A), oq.solve(B)
    print(f"compact: {ra.info.status} in {ra.info.iter} / {rb.info.status} in {rb.info.iter} iterations")
    assert ra.info.status == "Solved" and _equal_results(ra, rb)
    m = oq.dimensions(B)[1]
    cols = oq.interface._data_cols(B)
    outs = {k: torch.full((cols[k],), SENTINEL, dtype=torch.float64, device="cuda:0") for k in GRADS}
    act = torch.full((m,), SENTINEL, dtype=torch.float64, device="cuda:0")
    rc, msg = _raw_adjoint(product_lib, B, _dev(np.ones(n)), outs, act)
    print(f"refused with {rc}: {msg}")
    assert rc == 6 and "compact" in msg
    assert "osqp_amd_adjoint_dev" in msg  # the refusal names the symbol that was called
    with pytest.raises(oq.OSQPError, match="compact"):
        oq.adjoint(B, dx=_dev(np.ones(n)), out=dict(outs, act=act))
    with pytest.raises(oq.OSQPError, match="compact"):
        oq.jvp(B, q=_dev(np.ones(n)))
    assert all(bool(torch.all(v == SENTINEL)) for v in outs.values()) and bool(torch.all(act == SENTINEL))
    oq.clean(A); oq.clean(B)


@pytest.mark.parametrize("case", ["control6_unsorted", "tiny", "spd7", "grid2d"])
def test_adjoint_and_jvp_equal_their_host_forms(product_lib, oracle_lib, case):
    """On ONE solved model the host form, then the device form: the same bits, one factor build, the same number of solves."""
    for k, p in enumerate(mar.problems(oracle_lib, case)):
        n, m = len(p["q"]), len(p["l"])
        mdl = _model(product_lib, p)
        assert oq.solve(mdl).info.status == "Solved"
        cols = oq.interface._data_cols(mdl)
        gx, gy = mar.incoming(case, k, n, m, ncot=3)
        rng = np.random.default_rng(1000 + k)
        tang = {w: rng.standard_normal((3, cols[w])) for w in GRADS}

        def solves():
            return oq.adjoint_stats(mdl)["solves"]

        def adjoint_pair(dx, dy, want=GRADS):
            s0 = solves()
            h = oq.adjoint(mdl, dx=dx, dy=dy, want=want)
            s1 = solves()
            d = oq.adjoint(mdl, dx=None if dx is None else _dev(dx), dy=None if dy is None else _dev(dy), want=want)
            assert solves() - s1 == s1 - s0 > 0
            assert set(d) == set(want) | {"act"} == set(h)
            for w in want:
                assert d[w].is_cuda and tuple(d[w].shape) == h[w].shape and _same(_host(d[w]), h[w]), (case, k, w)
            assert np.array_equal(_host(d["act"]), h["act"])
            return d

        def jvp_pair(**t):
            s0 = solves()
            h = oq.jvp(mdl, **t)
            s1 = solves()
            d = oq.jvp(mdl, **{w: _dev(v) for w, v in t.items()})
            assert solves() - s1 == s1 - s0 > 0
            for o in ("x", "y"):
                assert d[o].is_cuda and tuple(d[o].shape) == h[o].shape and _same(_host(d[o]), h[o]), (case, k, o)
            assert d["act"].is_cuda and np.array_equal(_host(d["act"]), h["act"])
            return d

        adjoint_pair(gx[0], gy[0] if m else None)  # ncot = 1
        adjoint_pair(gx, gy if m else None)        # ncot = 3
        adjoint_pair(gx[0], None)                  # dx only
        if m:
            adjoint_pair(None, gy[0])              # dy only
        adjoint_pair(gx[0], gy[0] if m else None, want=("q",))
        have = {w: v for w, v in tang.items() if cols[w] > 0}
        jvp_pair(**{w: v[0] for w, v in have.items()})  # ndir = 1
        jvp_pair(**have)                                # ndir = 3
        only_q = jvp_pair(q=tang["q"][0])
        if m:  # a NULL tangent is a zero tangent
            with_zero = oq.jvp(mdl, q=_dev(tang["q"][0]), l=_dev(np.zeros(m)), Ax=_dev(np.zeros(cols["Ax"])))
            assert _same(_host(only_q["x"]), _host(with_zero["x"])) and _same(_host(only_q["y"]), _host(with_zero["y"]))
        # out=: the arrays given are the arrays written
        dq = _dev(np.full(n, np.nan))
        res = oq.adjoint(mdl, dx=_dev(gx[0]), want=("q",), out=dict(q=dq))
        assert res["q"] is dq and _same(_host(dq), oq.adjoint(mdl, dx=gx[0], want=("q",))["q"])
        assert oq.adjoint_stats(mdl)["builds"] == 1
        calls = oq.device_form_calls(mdl)
        assert calls["adjoint"] == (6 if m else 5) and calls["jvp"] == (4 if m else 3)
        oq.clean(mdl)


def test_nothing_else_moves(product_lib, oracle_lib):
    """grid2d(24): solve, device adjoint, device jvp, solve has the bits and the iteration count of solve, solve."""
    p = mar.problems(oracle_lib, "grid2d")[0]
    n, m = len(p["q"]), len(p["l"])
    gx, gy = mar.incoming("grid2d", 0, n, m)
    runs = []
    for derivatives in (False, True):
        mdl = _model(product_lib, p)
        r1 = oq.solve(mdl)
        if derivatives:
            oq.adjoint(mdl, dx=_dev(gx[0]), dy=_dev(gy[0]))
            oq.jvp(mdl, q=_dev(gx[0]), l=_dev(gy[0]))
        runs.append((r1, oq.solve(mdl)))
        oq.clean(mdl)
    (a1, a2), (b1, b2) = runs
    assert _equal_results(a1, b1) and _equal_results(a2, b2)
    assert a2.info.status == "Solved" and a2.info.rho_updates == b2.info.rho_updates


def test_refusals_write_nothing(product_lib, oracle_lib):
    """No current solution (a device update after the solve): return 1, the message names osqp_solve, and the outputs,
    prefilled with a sentinel, are untouched."""
    torch = _torch()
    p = mar.problems(oracle_lib, "control6_unsorted")[0]
    n, m = len(p["q"]), len(p["l"])
    mdl = _model(product_lib, p)
    assert oq.solve(mdl).info.status == "Solved"
    oq.update(mdl, q=_dev(p["q"] * 1.01))
    cols = oq.interface._data_cols(mdl)
    outs = {k: torch.full((cols[k],), SENTINEL, dtype=torch.float64, device="cuda:0") for k in GRADS}
    act = torch.full((m,), SENTINEL, dtype=torch.float64, device="cuda:0")
    rc, msg = _raw_adjoint(product_lib, mdl, _dev(np.ones(n)), outs, act)
    print(f"refused with {rc}: {msg}")
    assert rc == 1 and "osqp_solve" in msg
    tx = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda:0")
    with pytest.raises(oq.OSQPError, match="osqp_solve"):
        oq.jvp(mdl, q=_dev(np.ones(n)), out=dict(x=tx))
    assert all(bool(torch.all(v == SENTINEL)) for v in outs.values()) and bool(torch.all(act == SENTINEL)) and bool(torch.all(tx == SENTINEL))
    assert oq.adjoint_stats(mdl)["kept"] == 0 and oq.device_form_calls(mdl)["adjoint"] == 0
    oq.clean(mdl)
