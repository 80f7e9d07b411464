"""Adjoint of the resident batch without a GPU (tests/batch_adjoint_ref.py):
(a) `exact` against central finite differences of the exact active-set solution, moving all five data arrays at once;
(b) `exact` against central finite differences through the oracle's own polished solves, along q, l, u;
(c) `model` -- the kernel's algorithm from the scaled record -- against `exact`;
(d) the symbols, the NULL handle, and the argument checks of `ResidentBatch.adjoint` without a device.

Figures are relative to max(1, |reference|); every test prints its worst case per family before it asserts, and the bounds
are 100 times the values measured when this file was written (the residue is rounding times cond K, which varies by a few
decades across seeds and not more).  Measured, (non-degenerate / all instances in brackets):
  family    (a) h = 1e-7   (b) h = 1e-4      (c)
  tiny      1.3e-8 [8/8]  2.7e-11 (8 of 8)  1.0e-15
  ineq      5.5e-9 [6/6]  6.0e-12 (6 of 6)  8.9e-15
  wide300   1.5e-8 [6/6]                    3.3e-12
  tri128    4.5e-9 [3/3]                    8.7e-15
  eq100     1.1e-8 [4/6]                    3.0e-15
  mpc       3.4e-8 [25/64]                  4.3e-15
In (a) the step is h = 1e-7: the loss is not affine in Px and Ax, the truncation error of the central difference falls as
h^2 cond(K)^2 and its rounding error grows as eps cond(K) / h; at h = 1e-5 the one eq100 instance with cond K = 3e6 shows
1e-4 of truncation, at 1e-7 both terms are below 2e-8 on every family."""
import numpy as np
import pytest

from osqp_jl_amd import batch
from osqp_jl_amd import types as T
import batch_adjoint_ref as adj
from test_batch_resident_host import _NoLibrary

MEASURED_A = dict(tiny=1.3e-8, ineq=5.5e-9, wide300=1.5e-8, tri128=4.5e-9, eq100=1.1e-8, mpc=3.4e-8)
MEASURED_B = dict(tiny=2.7e-11, ineq=6.0e-12)
MEASURED_C = dict(tiny=1.0e-15, ineq=8.9e-15, wide300=3.3e-12, tri128=8.7e-15, eq100=3.0e-15, mpc=4.3e-15)  # the GPU test's bounds derive from these


def _usable(oracle_lib, family):
    """[(i, problem, oracle solution)] of the Solved instances whose K is non-singular."""
    probs, sols = adj.problems(oracle_lib, family), adj.oracle_solutions(oracle_lib, family)
    return [(i, p, s) for i, (p, s) in enumerate(zip(probs, sols))
            if s["status"] == 1 and adj.nondegenerate(p[2], s["act"], len(p[1]))]


@pytest.mark.parametrize("family", adj.FAMILIES)
def test_exact_agrees_with_finite_differences_of_the_active_set_solution(oracle_lib, family):
    """loss = g_x . x + g_y . y of the solution of the fixed active set, data moved by +-h d along a random direction d in
    Px, Ax, q, l, u together: (loss(+) - loss(-)) / 2h against sum <gradient, d>."""
    use = _usable(oracle_lib, family)
    gx_all, gy_all = adj.incoming(family, len(adj.problems(oracle_lib, family)), len(use[0][1][1]), len(use[0][1][3]))
    rng = np.random.default_rng(5)
    h, worst = 1e-7, 0.0  # truncation falls as h^2 cond(K)^2, rounding grows as eps cond(K) / h: see the header
    for i, (P, q, A, l, u), s in use:
        act, gx, gy = s["act"], gx_all[i], gy_all[i]
        x, y = adj.active_set_solution(P, q, A, l, u, act)
        g = adj.exact(P, A, x, y, act, gx, gy)
        U = adj.sp.triu(adj.sp.csc_matrix(P), format="csc"); U.sort_indices()
        Ac = adj.sp.csc_matrix(A); Ac.sort_indices()
        d = {k: rng.standard_normal(len(g[k])) for k in adj.GRADS}
        loss = []
        for sign in (1.0, -1.0):
            Ud, Ad = U.copy(), Ac.copy()
            Ud.data = U.data + sign * h * d["Px"]; Ad.data = Ac.data + sign * h * d["Ax"]
            xp, yp = adj.active_set_solution(Ud, q + sign * h * d["q"], Ad, l + sign * h * d["l"], u + sign * h * d["u"], act)
            loss.append(gx @ xp + gy @ yp)
        fd, an = (loss[0] - loss[1]) / (2 * h), sum(float(g[k] @ d[k]) for k in adj.GRADS)
        worst = max(worst, abs(fd - an) / max(1.0, abs(an)))
    print(f"(a) {family}: {len(use)} instances, worst |fd - analytic| rel {worst:.2e}")
    assert len(use) >= adj.MIN_NONDEGENERATE[family]
    assert worst <= 100 * MEASURED_A[family], worst


@pytest.mark.parametrize("family,need", [("tiny", 7), ("ineq", 4)])
def test_exact_agrees_with_finite_differences_through_the_oracle(oracle_lib, family, need):
    """Three polished oracle solves at the data and at +-h d along (q, l, u), h = 1e-4: the solution is piecewise affine in
    these, so on one active set the central difference has no truncation error.  Compared: instances whose three solves were
    all polish-accepted with one active set."""
    probs, base = adj.problems(oracle_lib, family), adj.oracle_solutions(oracle_lib, family)
    count, n, m = len(probs), len(probs[0][1]), len(probs[0][3])
    gx_all, gy_all = adj.incoming(family, count, n, m)
    rng = np.random.default_rng(11)
    dq, dl, du = rng.standard_normal((count, n)), rng.standard_normal((count, m)), rng.standard_normal((count, m))
    q0, l0, u0 = (np.array([p[k] for p in probs]) for k in (1, 3, 4))
    du = np.where(l0 == u0, dl, du)  # an equality row moves as one
    h = 1e-4
    moved = [adj.oracle_solve(oracle_lib, probs, q=q0 + s * h * dq, l=l0 + s * h * dl, u=u0 + s * h * du) for s in (1.0, -1.0)]
    worst, used = 0.0, 0
    for i, (P, q, A, l, u) in enumerate(probs):
        three = (base[i], moved[0][i], moved[1][i])
        if not all(t["status"] == 1 and t["polish"] == 1 and np.array_equal(t["act"], base[i]["act"]) for t in three):
            continue
        if not adj.nondegenerate(A, base[i]["act"], n):
            continue
        used += 1
        g = adj.exact(P, A, base[i]["x"], base[i]["y"], base[i]["act"], gx_all[i], gy_all[i])
        loss = [gx_all[i] @ t["x"] + gy_all[i] @ t["y"] for t in three[1:]]
        fd, an = (loss[0] - loss[1]) / (2 * h), float(g["q"] @ dq[i] + g["l"] @ dl[i] + g["u"] @ du[i])
        worst = max(worst, abs(fd - an) / max(1.0, abs(an)))
    print(f"(b) {family}: {used} of {count} instances compared, worst rel {worst:.2e}")
    assert used >= need
    assert worst <= 100 * MEASURED_B[family], worst


@pytest.mark.parametrize("family", adj.FAMILIES)
def test_model_agrees_with_exact(oracle_lib, family):
    use = _usable(oracle_lib, family)
    gx_all, gy_all = adj.incoming(family, len(adj.problems(oracle_lib, family)), len(use[0][1][1]), len(use[0][1][3]))
    worst = 0.0
    for i, (P, q, A, l, u), s in use:
        got = adj.model(P, q, A, l, u, *s["state"], gx_all[i], gy_all[i])
        assert got["status"] == 1 and np.array_equal(got["act"], s["act"])
        worst = max(worst, adj.rel_err(got, adj.exact(P, A, got["x"], got["y"], got["act"], gx_all[i], gy_all[i])))
    print(f"(c) {family}: {len(use)} instances, model vs exact worst rel {worst:.2e}")
    assert len(use) >= adj.MIN_NONDEGENERATE[family]
    assert worst <= 100 * MEASURED_C[family], worst


def test_the_adjoint_symbols_are_bound_and_exported(product_lib):
    for name, nargs in (("osqp_amd_batch_adjoint", 11), ("osqp_amd_batch_adjoint_launches", 0)):
        assert name in T.EXT_SYMBOLS, name
        res, args = T.EXT_SYMBOLS[name]
        assert res is T.c_int and len(args) == nargs
        fn = getattr(product_lib, name)  # AttributeError: not exported
        assert fn.restype is T.c_int and list(fn.argtypes or []) == list(args)


def test_adjoint_refuses_a_null_handle(product_lib):
    buf = np.zeros(4)
    before = product_lib.osqp_amd_batch_adjoint_launches()
    assert product_lib.osqp_amd_batch_adjoint(None, buf.ctypes.data, None, buf.ctypes.data, None, None, None, None, None, None, 0) == 1
    assert b"handle" in product_lib.osqp_amd_last_error()
    assert product_lib.osqp_amd_batch_adjoint_launches() == before


def test_adjoint_checks_its_arguments_in_python():
    rb = batch.ResidentBatch.__new__(batch.ResidentBatch)  # the checks of a live handle, without a device
    rb.lib, rb.handle, rb.device = _NoLibrary(), None, 0
    rb.count, rb.n, rb.m, rb.nnzP, rb.nnzA = 3, 2, 3, 2, 4

    class Dev:  # a device array as far as the checks can tell
        def __init__(self, *shape, dtype="float64"):
            self.shape, self.dtype = shape, dtype

        def data_ptr(self):
            return 4096

    with pytest.raises(ValueError, match="dx and dy"):
        rb.adjoint()
    with pytest.raises(ValueError, match="dx"):
        rb.adjoint(dx=np.ones((3, 3)))
    with pytest.raises(ValueError, match="dy"):
        rb.adjoint(dy=np.ones((2, 3)))
    with pytest.raises(ValueError, match="dx"):
        rb.adjoint(dx=np.array([["a", "b"]] * 3))
    with pytest.raises(ValueError, match="want"):
        rb.adjoint(dx=np.ones((3, 2)), want=("q", "z"))
    with pytest.raises(ValueError, match="both"):  # host and device mixed
        rb.adjoint(dx=np.ones((3, 2)), dy=Dev(3, 3))
    with pytest.raises(ValueError, match="out"):  # host inputs take no out
        rb.adjoint(dx=np.ones((3, 2)), out=dict(q=Dev(3, 2)))
    with pytest.raises(ValueError, match="out"):  # device inputs need one
        rb.adjoint(dx=Dev(3, 2))
    with pytest.raises(ValueError, match="'l'"):  # a wanted gradient without its array
        rb.adjoint(dx=Dev(3, 2), want=("q", "l"), out=dict(q=Dev(3, 2)))
    with pytest.raises(ValueError, match="Px"):  # wrong width
        rb.adjoint(dx=Dev(3, 2), want=("Px",), out=dict(Px=Dev(3, 3)))
    with pytest.raises(ValueError, match="float64"):
        rb.adjoint(dx=Dev(3, 2), want=("q",), out=dict(q=Dev(3, 2, dtype="float32")))
    with pytest.raises(ValueError, match="device array"):
        rb.adjoint(dx=Dev(3, 2), want=("q",), out=dict(q=np.zeros((3, 2))))
    with pytest.raises(ValueError, match="unknown"):
        rb.adjoint(dx=Dev(3, 2), want=("q",), out=dict(q=Dev(3, 2), x=Dev(3, 2)))
    rb.handle = None
