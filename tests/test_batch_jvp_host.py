"""Forward sensitivities of the resident batch without a GPU (tests/batch_jvp_ref.py):
(a) `exact` against central finite differences of the exact active-set solution, moving all five data arrays at once;
(b) duality: g_x . tx + g_y . ty of `exact` equals sum <batch_adjoint_ref.exact gradient, direction>;
(c) `model` -- the kernel's algorithm from the scaled record -- against `exact`;
(d) duality of the two models (batch_adjoint_ref.model and `model`): the CPU figure the GPU duality test scales;
(e) the symbols, the NULL handle, and the argument checks of `ResidentBatch.jvp` without a device.

(a) and (c) are relative to max(1, max|reference|) per output, (b) and (d) are |difference| / max(1, sum |terms|).  Every test
prints its worst case per family before it asserts, and the bounds are 100 times the values measured when this file was
written -- the convention and the margin of tests/test_batch_adjoint_host.py, whose header explains the step h = 1e-7 of (a).
Measured (non-degenerate instances of all in brackets, three directions each in (b), (c), (d), one in (a)):
  family    (a) h = 1e-7      (b)      (c)      (d)
  tiny      2.2e-9 [8/8]      1.5e-16  1.3e-15  1.9e-16
  ineq      7.1e-9 [6/6]      1.1e-15  1.3e-14  6.9e-17
  wide300   1.7e-8 [6/6]      1.1e-15  3.1e-12  2.1e-16
  tri128    7.8e-9 [3/3]      6.3e-16  1.6e-14  5.3e-17
  eq100     9.3e-9 [4/6]      2.6e-16  2.8e-15  2.0e-16
  mpc       4.9e-9 [25/64]    1.4e-16  5.2e-15  6.7e-17
The refined solve is a symmetric operator (a polynomial in K and the factor's inverse), applied once to the gradient and once
to the direction: (d) sits at rounding level even where (c) shows the operator 3e-12 away from K^-1.
"""
import numpy as np
import pytest

from osqp_jl_amd import batch
from osqp_jl_amd import types as T
import batch_adjoint_ref as adj
import batch_jvp_ref as jv
from test_batch_resident_host import _NoLibrary

MEASURED_A = dict(tiny=2.2e-9, ineq=7.1e-9, wide300=1.7e-8, tri128=7.8e-9, eq100=9.3e-9, mpc=4.9e-9)
MEASURED_B = dict(tiny=1.5e-16, ineq=1.1e-15, wide300=1.1e-15, tri128=6.3e-16, eq100=2.6e-16, mpc=1.4e-16)
MEASURED_C = dict(tiny=1.3e-15, ineq=1.3e-14, wide300=3.1e-12, tri128=1.6e-14, eq100=2.8e-15, mpc=5.2e-15)  # the GPU test's bounds against `exact` derive from these
MEASURED_D = dict(tiny=1.9e-16, ineq=6.9e-17, wide300=2.1e-16, tri128=5.3e-17, eq100=2.0e-16, mpc=6.7e-17)  # the GPU test's duality bounds derive from these
NDIR = 3


def _usable(oracle_lib, family):
    """[(i, problem, oracle solution)] of the Solved instances whose K is non-singular."""
    probs, sols = jv.problems(oracle_lib, family), jv.oracle_solutions(oracle_lib, family)
    return [(i, p, s) for i, (p, s) in enumerate(zip(probs, sols))
            if s["status"] == 1 and jv.nondegenerate(p[2], s["act"], len(p[1]))]


@pytest.mark.parametrize("family", jv.FAMILIES)
def test_exact_agrees_with_finite_differences_of_the_active_set_solution(oracle_lib, family):
    """The solution of the fixed active set with the data moved by +-h d along a random direction d in Px, Ax, q, l, u
    together: (x(+) - x(-)) / 2h, (y(+) - y(-)) / 2h against (tx, ty)."""
    use = _usable(oracle_lib, family)
    d_all = jv.tangents(family, 1, jv.problems(oracle_lib, family))
    h, worst = 1e-7, 0.0
    for i, (P, q, A, l, u), s in use:
        act, d = s["act"], jv.direction(d_all, 0, i)
        x, y = adj.active_set_solution(P, q, A, l, u, act)
        tx, ty = jv.exact(P, A, x, y, act, d)
        U = adj.sp.triu(adj.sp.csc_matrix(P), format="csc"); U.sort_indices()
        Ac = adj.sp.csc_matrix(A); Ac.sort_indices()
        moved = []
        for sign in (1.0, -1.0):
            Ud, Ad = U.copy(), Ac.copy()
            Ud.data = U.data + sign * h * d["Px"]; Ad.data = Ac.data + sign * h * d["Ax"]
            moved.append(adj.active_set_solution(Ud, q + sign * h * d["q"], Ad, l + sign * h * d["l"], u + sign * h * d["u"], act))
        fdx, fdy = (moved[0][0] - moved[1][0]) / (2 * h), (moved[0][1] - moved[1][1]) / (2 * h)
        worst = max(worst, jv.rel_err(fdx, fdy, tx, ty))
    print(f"(a) {family}: {len(use)} instances, worst |fd - analytic| rel {worst:.2e}")
    assert len(use) >= jv.MIN_NONDEGENERATE[family]
    assert worst <= 100 * MEASURED_A[family], worst


@pytest.mark.parametrize("family", jv.FAMILIES)
def test_exact_is_dual_to_the_exact_adjoint(oracle_lib, family):
    use = _usable(oracle_lib, family)
    probs = jv.problems(oracle_lib, family)
    gx_all, gy_all = adj.incoming(family, len(probs), len(probs[0][1]), len(probs[0][3]))
    d_all = jv.tangents(family, NDIR, probs)
    worst = 0.0
    for i, (P, q, A, l, u), s in use:
        g = adj.exact(P, A, s["x"], s["y"], s["act"], gx_all[i], gy_all[i])
        for k in range(NDIR):
            d = jv.direction(d_all, k, i)
            tx, ty = jv.exact(P, A, s["x"], s["y"], s["act"], d)
            worst = max(worst, jv.duality_gap(gx_all[i], gy_all[i], tx, ty, g, d))
    print(f"(b) {family}: {len(use)} instances, duality gap of exact worst rel {worst:.2e}")
    assert len(use) >= jv.MIN_NONDEGENERATE[family]
    assert worst <= 100 * MEASURED_B[family], worst


@pytest.mark.parametrize("family", jv.FAMILIES)
def test_model_agrees_with_exact_and_is_dual_to_the_adjoint_model(oracle_lib, family):
    use = _usable(oracle_lib, family)
    probs = jv.problems(oracle_lib, family)
    gx_all, gy_all = adj.incoming(family, len(probs), len(probs[0][1]), len(probs[0][3]))
    d_all = jv.tangents(family, NDIR, probs)
    worst, gap = 0.0, 0.0
    for i, (P, q, A, l, u), s in use:
        g = adj.model(P, q, A, l, u, *s["state"], gx_all[i], gy_all[i])
        for k in range(NDIR):
            d = jv.direction(d_all, k, i)
            got = jv.model(P, q, A, l, u, *s["state"], d)
            assert got["status"] == 1 and np.array_equal(got["act"], s["act"])
            worst = max(worst, jv.rel_err(got["tx"], got["ty"], *jv.exact(P, A, got["x"], got["y"], got["act"], d)))
            gap = max(gap, jv.duality_gap(gx_all[i], gy_all[i], got["tx"], got["ty"], g, d))
    print(f"(c) {family}: {len(use)} instances, model vs exact worst rel {worst:.2e}; (d) duality gap of the models {gap:.2e}")
    assert len(use) >= jv.MIN_NONDEGENERATE[family]
    assert worst <= 100 * MEASURED_C[family], worst
    assert gap <= 100 * MEASURED_D[family], gap


def test_the_jvp_symbols_are_bound_and_exported(product_lib):
    for name, nargs in (("osqp_amd_batch_jvp", 12), ("osqp_amd_batch_jvp_launches", 0)):
        assert name in T.EXT_SYMBOLS, name
        res, args = T.EXT_SYMBOLS[name]
        assert res is T.c_int and len(args) == nargs
        fn = getattr(product_lib, name)  # AttributeError: not exported
        assert fn.restype is T.c_int and list(fn.argtypes or []) == list(args)


def test_jvp_refuses_a_null_handle(product_lib):
    buf = np.zeros(4)
    before = product_lib.osqp_amd_batch_jvp_launches()
    assert product_lib.osqp_amd_batch_jvp(None, 1, buf.ctypes.data, None, None, None, None, buf.ctypes.data, None, None, None, 0) == 1
    assert b"handle" in product_lib.osqp_amd_last_error()
    assert product_lib.osqp_amd_batch_jvp_launches() == before


def test_jvp_checks_its_arguments_in_python():
    rb = batch.ResidentBatch.__new__(batch.ResidentBatch)  # the checks of a live handle, without a device
    rb.lib, rb.handle, rb.device = _NoLibrary(), None, 0
    rb.count, rb.n, rb.m, rb.nnzP, rb.nnzA = 3, 2, 3, 2, 4

    class Dev:  # a device array as far as the checks can tell
        def __init__(self, *shape, dtype="float64"):
            self.shape, self.dtype = shape, dtype

        def data_ptr(self):
            return 4096

    with pytest.raises(ValueError, match="at least one tangent"):
        rb.jvp()
    with pytest.raises(ValueError, match="q"):  # wrong width
        rb.jvp(q=np.ones((3, 3)))
    with pytest.raises(ValueError, match="l"):  # wrong count
        rb.jvp(l=np.ones((2, 3)))
    with pytest.raises(ValueError, match="Ax"):  # wrong width under a direction axis
        rb.jvp(Ax=np.ones((2, 3, 5)))
    with pytest.raises(ValueError, match="q"):
        rb.jvp(q=np.array([["a", "b"]] * 3))
    with pytest.raises(ValueError, match="dimensions"):  # one direction and several, mixed
        rb.jvp(q=np.ones((3, 2)), l=np.ones((2, 3, 3)))
    with pytest.raises(ValueError, match="dimensions"):
        rb.jvp(q=np.ones(2))
    with pytest.raises(ValueError, match="u"):  # another ndir
        rb.jvp(q=np.ones((2, 3, 2)), u=np.ones((4, 3, 3)))
    with pytest.raises(ValueError, match="all be host arrays or all device"):
        rb.jvp(q=np.ones((3, 2)), l=Dev(3, 3))
    with pytest.raises(ValueError, match="out"):  # host inputs take no out
        rb.jvp(q=np.ones((3, 2)), out=dict(x=Dev(3, 2), y=Dev(3, 3)))
    with pytest.raises(ValueError, match="out"):  # device inputs need one
        rb.jvp(q=Dev(3, 2))
    with pytest.raises(ValueError, match="'y'"):
        rb.jvp(q=Dev(3, 2), out=dict(x=Dev(3, 2)))
    with pytest.raises(ValueError, match="'x'"):
        rb.jvp(q=Dev(3, 2), out=dict(y=Dev(3, 3)))
    with pytest.raises(ValueError, match="x"):  # the outputs follow the direction axis
        rb.jvp(q=Dev(2, 3, 2), out=dict(x=Dev(3, 2), y=Dev(2, 3, 3)))
    with pytest.raises(ValueError, match="float64"):
        rb.jvp(q=Dev(3, 2), out=dict(x=Dev(3, 2, dtype="float32"), y=Dev(3, 3)))
    with pytest.raises(ValueError, match="device array"):
        rb.jvp(q=Dev(3, 2), out=dict(x=np.zeros((3, 2)), y=Dev(3, 3)))
    with pytest.raises(ValueError, match="unknown"):
        rb.jvp(q=Dev(3, 2), out=dict(x=Dev(3, 2), y=Dev(3, 3), q=Dev(3, 2)))
    with pytest.raises(ValueError, match="status"):
        rb.jvp(q=Dev(3, 2), out=dict(x=Dev(3, 2), y=Dev(3, 3), status=Dev(3)))
    rb.handle = None
