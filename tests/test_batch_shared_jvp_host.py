"""The forward sensitivities of the shared batch without a GPU (tests/batch_shared_jvp_cases.py):
(a) `batch_jvp_ref.model` -- the kernel's algorithm from the scaled state of an instance that carries the scaling of the BASE
    data, with the matrix tangents shared by the instances -- against `exact`, on the Solved, well-conditioned oracle instances
    of each family: the figures MEASURED_C, from which the GPU test takes its bounds (1000 x);
(b) the duality of `batch_jvp_ref.model` with `batch_adjoint_ref.model` on the same states (`batch_jvp_ref.duality_gap`): the
    figure MEASURED_D, from which the GPU test takes the bound of its duality test (1000 x);
(c) the two symbols in the header, types.py, batch.py and the Julia file, the NULL handle, and the argument checks of
    `SharedBatch.jvp` and `SharedBatch.jacobian` without a device.

Measured when this file was written (oracle states, default S.OPTS, direction 0 of `tangents(name, 1)` and cotangent 0 of
`cotangents(name, 1, ...)`), well-conditioned / all:
  family          (a) model vs exact   (b) duality   compared
  banded-17       9.2e-15              1.5e-16       35 / 35
  banded-33-eq    1.7e-14              9.5e-17       35 / 35
  banded-128      5.9e-14              8.0e-17       35 / 35
  random-129-eq   6.3e-14              3.9e-17       35 / 35
  banded-256      2.1e-13              8.9e-17       10 / 11   (instance 1: cond K 1.3e14, what the filter is for)
  banded-240      9.9e-14              3.6e-17       19 / 19
The bounds of (a) and (b) are 100 times these, the convention of tests/test_batch_shared_adjoint_host.py: the residue of (a) is
rounding times cond K; (b) compares two solves with the same symmetric matrix, and is relative to the sum of the magnitudes of
the terms."""
import os
import re

import numpy as np
import pytest

from osqp_jl_amd import batch
from osqp_jl_amd import types as T
import batch_adjoint_ref as adj
import batch_jvp_ref as jref
import batch_shared_jvp_cases as SJ
from test_batch_resident_host import _NoLibrary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED_C = {"banded-17": 9.2e-15, "banded-33-eq": 1.7e-14, "banded-128": 5.9e-14, "random-129-eq": 6.3e-14, "banded-256": 2.1e-13,
              "banded-240": 9.9e-14}  # the GPU test's bounds derive from these
MEASURED_D = 1.5e-16  # the worst family of (b); the GPU test takes the bound of its duality test from it
COMPARED = {"banded-17": 35, "banded-33-eq": 35, "banded-128": 35, "random-129-eq": 35, "banded-256": 10, "banded-240": 19}
ENTRY_POINTS = {"osqp_amd_shared_batch_jvp": 12, "osqp_amd_shared_batch_jvp_launches": 0}


def _usable(oracle_lib, name):
    """[(i, oracle solution)] of the Solved, well-conditioned instances."""
    base = SJ.family(name)[0]
    return [(i, s) for i, s in enumerate(SJ.oracle_states(oracle_lib, name)) if s["status"] == 1 and SJ.well_conditioned(base[0], base[2], s["act"])]


@pytest.mark.parametrize("name", list(SJ.CASES))
def test_model_agrees_with_exact_and_with_the_adjoint_model(oracle_lib, name):
    base, q, l, u = SJ.family(name)
    P, A = base[0], base[2]
    t = SJ.tangents(name, 1)
    gx, gy = SJ.cotangents(name, 1, *q.shape, l.shape[1])
    use = _usable(oracle_lib, name)
    worst, gap = 0.0, 0.0
    for i, s in use:
        d = SJ.direction(t, 0, i)
        got = jref.model(P, q[i], A, l[i], u[i], *s["state"], d)
        assert got["status"] == 1 and np.array_equal(got["act"], s["act"])
        want = jref.exact(P, A, got["x"], got["y"], got["act"], d)
        worst = max(worst, jref.rel_err(got["tx"], got["ty"], *want))
        g = adj.model(P, q[i], A, l[i], u[i], *s["state"], gx[0, i], gy[0, i])
        gap = max(gap, jref.duality_gap(gx[0, i], gy[0, i], got["tx"], got["ty"], g, d))
    print(f"(a) {name}: {len(use)} of {q.shape[0]} instances, model vs exact worst rel {worst:.2e}; (b) duality with the adjoint model {gap:.2e}")
    assert len(use) == COMPARED[name] and len(use) >= SJ.count_of(name) - 3
    assert worst <= 100 * MEASURED_C[name], worst
    assert gap <= 100 * MEASURED_D, gap


@pytest.mark.parametrize("name", ["banded-33-eq", "random-129-eq"])
def test_tangents_are_per_instance_shared_and_tied_on_equalities(name):
    base, q, l, u = SJ.family(name)
    a, b = SJ.tangents(name, 3), SJ.tangents(name, 3, 5)
    assert a["q"].shape == (3,) + q.shape and a["l"].shape == a["u"].shape == (3,) + l.shape
    assert a["Px"].ndim == 2 and a["Ax"].ndim == 2 and a["Px"].shape[0] == 3
    for k in ("q", "l", "u"):
        assert np.array_equal(a[k][:, :5], b[k]), k  # instance i has the same tangent whatever count is
    for k in ("Px", "Ax"):
        assert np.array_equal(a[k], b[k]), k  # drawn from the name alone
    eq = l == u
    assert eq.any() and np.array_equal(a["u"][:, eq], a["l"][:, eq]) and not np.array_equal(a["u"][:, ~eq], a["l"][:, ~eq])


def test_the_symbols_are_declared_bound_and_wrapped(product_lib):
    header = open(os.path.join(ROOT, "include", "osqp_amd.h")).read()
    py = open(os.path.join(ROOT, "osqp.jl_amd", "batch.py")).read()
    jl = open(os.path.join(ROOT, "osqp.jl_amd", "julia", "OSQPAMD.jl")).read()
    for name, nargs in ENTRY_POINTS.items():
        assert re.search(r"\b%s\s*\(" % name, header), name
        res, args = T.EXT_SYMBOLS[name]
        assert res is T.c_int and len(args) == nargs
        fn = getattr(product_lib, name)  # AttributeError: not exported
        assert fn.restype is T.c_int and list(fn.argtypes or []) == list(args)
        assert name in py and ":" + name in jl, name
    assert callable(batch.SharedBatch.jvp) and callable(batch.SharedBatch.jacobian) and callable(batch.shared_jvp_launches)
    assert "has no polish, certificates" in header  # forward sensitivities have left the list of what the handle lacks


def test_jvp_refuses_a_null_handle(product_lib):
    buf = np.zeros(4)
    before = product_lib.osqp_amd_shared_batch_jvp_launches()
    assert product_lib.osqp_amd_shared_batch_jvp(None, 1, buf.ctypes.data, None, None, None, None, buf.ctypes.data, None, None, None, 0) == 1
    assert b"null" in product_lib.osqp_amd_last_error()
    assert product_lib.osqp_amd_shared_batch_jvp_launches() == before


class _Dev:  # a device array as far as the checks can tell
    def __init__(self, *shape, dtype="float64"):
        self.shape, self.dtype = shape, dtype

    def data_ptr(self):
        return 4096


def _handle():
    sb = batch.SharedBatch.__new__(batch.SharedBatch)  # the checks of a live handle, without a device
    sb.lib, sb.handle, sb.device = _NoLibrary(), None, 0
    sb.count, sb.n, sb.m, sb.nnzP, sb.nnzA = 3, 2, 3, 2, 4
    return sb


def test_jvp_checks_its_arguments_in_python():
    sb, Dev = _handle(), _Dev
    with pytest.raises(ValueError, match="at least one tangent"):
        sb.jvp()
    with pytest.raises(ValueError, match="q"):  # wrong width
        sb.jvp(q=np.ones((3, 3)))
    with pytest.raises(ValueError, match="l"):  # wrong count
        sb.jvp(l=np.ones((2, 3)))
    with pytest.raises(ValueError, match="Px"):  # the shared tangent is one row, not one per instance
        sb.jvp(q=np.ones((3, 2)), Px=np.ones((3, 2)))
    with pytest.raises(ValueError, match="leading axis"):  # mixed ranks: q with directions, Px without
        sb.jvp(q=np.ones((2, 3, 2)), Px=np.ones(2))
    with pytest.raises(ValueError, match="leading axis"):
        sb.jvp(q=np.ones((3, 2)), Ax=np.ones((1, 4)))
    with pytest.raises(ValueError, match="leading axis"):
        sb.jvp(q=np.ones(2))
    with pytest.raises(ValueError, match="Px"):
        sb.jvp(Px=np.ones(3))
    with pytest.raises(ValueError, match="same number of directions"):
        sb.jvp(q=np.ones((2, 3, 2)), Ax=np.ones((4, 4)))
    with pytest.raises(ValueError, match="all be host arrays or all device arrays"):
        sb.jvp(q=np.ones((3, 2)), Px=Dev(2))
    with pytest.raises(ValueError, match="out"):  # host inputs take no out
        sb.jvp(q=np.ones((3, 2)), out=dict(x=Dev(3, 2)))
    with pytest.raises(ValueError, match="out"):  # device inputs need one
        sb.jvp(q=Dev(3, 2))
    with pytest.raises(ValueError, match="'x' or 'y'"):
        sb.jvp(q=Dev(3, 2), out=dict(act=Dev(3, 3)))
    with pytest.raises(ValueError, match="unknown"):
        sb.jvp(q=Dev(3, 2), out=dict(x=Dev(3, 2), q=Dev(3, 2)))
    with pytest.raises(ValueError, match=r"out\['x'\]"):  # one row per direction
        sb.jvp(Px=Dev(2, 2), out=dict(x=Dev(3, 2)))
    with pytest.raises(ValueError, match="float64"):
        sb.jvp(q=Dev(3, 2, dtype="float32"), out=dict(x=Dev(3, 2)))
    sb.m = sb.nnzA = 0  # tangents of width 0 are left out: nothing remains
    with pytest.raises(ValueError, match="width 0"):
        sb.jvp(l=np.ones((3, 0)), u=np.ones((3, 0)), Ax=np.ones(0))
    sb.handle = None


def test_jacobian_checks_its_arguments_in_python():
    sb = _handle()
    with pytest.raises(ValueError, match="of"):
        sb.jacobian(of=())
    with pytest.raises(ValueError, match="of"):
        sb.jacobian(of=("x", "x"))
    with pytest.raises(ValueError, match="of"):
        sb.jacobian(of=("q",))
    with pytest.raises(ValueError, match="wrt"):
        sb.jacobian(wrt=("x",))
    with pytest.raises(ValueError, match="wrt"):
        sb.jacobian(wrt=("Px_sum",))
    with pytest.raises(ValueError, match="mode"):
        sb.jacobian(mode="both")
    with pytest.raises(ValueError, match="chunk"):
        sb.jacobian(chunk=0)
    with pytest.raises(ValueError, match="chunk"):
        sb.jacobian(chunk=True)
    with pytest.raises(TypeError):  # host arrays only: no out_rows, no device option
        sb.jacobian(device=True)
    with pytest.raises(TypeError):
        sb.jacobian(out_rows=dict(x=[0]))
    sb.m = 0
    with pytest.raises(ValueError, match="no output component or no data column"):
        sb.jacobian(of=("y",))
    sb.handle = None
