"""The adjoint of the shared batch without a GPU (tests/batch_shared_adjoint_cases.py):
(a) the families: every instance Solved by the oracle, the coverage the GPU comparison needs after the `well_conditioned` filter,
    and T of the shape as the table states it;
(b) `batch_adjoint_ref.model` -- the kernel's algorithm from the scaled state of an instance that carries the scaling of the BASE
    data -- against `exact`: the figures MEASURED_C, from which the GPU test takes its bounds (1000 x);
(c) `block_sum`, the summation order of the contract, against math.fsum;
(d) the two symbols in the header, types.py, batch.py and the Julia file, the NULL handle, and the argument checks of
    `SharedBatch.adjoint` without a device.

Measured when this file was written (oracle states, default S.OPTS, ncot = 1 of `cotangents`), well-conditioned / all:
  family          (b) model vs exact   compared
  banded-17       4.4e-15              35 / 35
  banded-33-eq    7.5e-15              35 / 35
  banded-128      6.1e-14              35 / 35
  random-129-eq   5.4e-14              35 / 35
  banded-256      2.1e-13              10 / 11   (instance 1: cond K 1.3e14, what the filter is for)
  banded-240      9.0e-14              19 / 19   (T = 8; seed 280 also keeps 19 of 19, at 2.1e-10: the worse-conditioned draw)
The bounds of (b) are 100 times these, the convention of tests/test_batch_adjoint_host.py: the residue is rounding times cond K."""
import math
import os
import re

import numpy as np
import pytest

from osqp_jl_amd import batch
from osqp_jl_amd import types as T
import batch_adjoint_ref as adj
import batch_shared_adjoint_cases as SA
from test_batch_resident_host import _NoLibrary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED_C = {"banded-17": 4.4e-15, "banded-33-eq": 7.5e-15, "banded-128": 6.1e-14, "random-129-eq": 5.4e-14, "banded-256": 2.1e-13,
              "banded-240": 9.0e-14}  # the GPU test's bounds derive from these
COMPARED = {"banded-17": 35, "banded-33-eq": 35, "banded-128": 35, "random-129-eq": 35, "banded-256": 10, "banded-240": 19}
ENTRY_POINTS = {"osqp_amd_shared_batch_adjoint": 14, "osqp_amd_shared_batch_adjoint_launches": 0}


def _usable(oracle_lib, name):
    """[(i, oracle solution)] of the Solved, well-conditioned instances."""
    base = SA.family(name)[0]
    return [(i, s) for i, s in enumerate(SA.oracle_states(oracle_lib, name)) if s["status"] == 1 and SA.well_conditioned(base[0], base[2], s["act"])]


@pytest.mark.parametrize("name", list(SA.CASES))
def test_families_are_solved_and_cover_the_comparison(oracle_lib, product_lib, name):
    base, q, l, u = SA.family(name)
    sols = SA.oracle_states(oracle_lib, name)
    use = _usable(oracle_lib, name)
    print(f"{name}: count {len(sols)}, Solved {sum(s['status'] == 1 for s in sols)}, well-conditioned {len(use)}")
    assert len(sols) == SA.count_of(name) and all(s["status"] == 1 for s in sols)
    assert len(use) == COMPARED[name] and len(use) >= SA.count_of(name) - 3
    assert batch.shared_plan(product_lib, base[0], base[2])["T"] == SA.CASES[name][4]  # host only: no device is touched


@pytest.mark.parametrize("name", list(SA.CASES))
def test_model_agrees_with_exact(oracle_lib, name):
    base, q, l, u = SA.family(name)
    P, A = base[0], base[2]
    gx, gy = SA.cotangents(name, 1, *q.shape, l.shape[1])
    use = _usable(oracle_lib, name)
    worst = 0.0
    for i, s in use:
        got = adj.model(P, q[i], A, l[i], u[i], *s["state"], gx[0, i], gy[0, i])
        assert got["status"] == 1 and np.array_equal(got["act"], s["act"])
        worst = max(worst, adj.rel_err(got, adj.exact(P, A, got["x"], got["y"], got["act"], gx[0, i], gy[0, i])))
    print(f"(b) {name}: {len(use)} instances, model vs exact worst rel {worst:.2e}")
    assert worst <= 100 * MEASURED_C[name], worst


@pytest.mark.parametrize("count", [1, 15, 16, 17, 35, 100])
def test_block_sum_is_a_sum(count):
    """Against math.fsum (the correctly rounded sum): each of the count - 1 additions loses at most half an ulp of a partial
    sum, which is bounded by the sum of the magnitudes."""
    rng = np.random.default_rng(count)
    rows = rng.standard_normal((count, 7)) * 10.0 ** rng.integers(-3, 4, size=(count, 1))
    got = SA.block_sum(rows)
    for k in range(rows.shape[1]):
        assert abs(got[k] - math.fsum(rows[:, k])) <= count * np.finfo(float).eps * float(np.sum(np.abs(rows[:, k])))
    if count <= SA.BLOCK:  # one block: the plain left-to-right sum
        want = rows[0].copy()
        for r in rows[1:]:
            want = want + r
        assert np.array_equal(got, want)


def test_block_sum_order_is_blocks_of_16():
    """1 followed by 31 terms of 2^-53: left to right every small term vanishes against the 1; in blocks of 16 the second
    block adds up to 2^-49 first and survives."""
    rows = np.array([1.0] + [2.0 ** -53] * 31)[:, None]
    naive = rows[0].copy()
    for r in rows[1:]:
        naive = naive + r
    assert naive[0] == 1.0
    assert SA.block_sum(rows)[0] == 1.0 + 2.0 ** -49


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
    assert callable(batch.SharedBatch.adjoint) and callable(batch.shared_adjoint_launches)
    assert "((s_0 + s_1)" in header  # the summation order is part of the contract


def test_adjoint_refuses_a_null_handle(product_lib):
    buf = np.zeros(4)
    before = product_lib.osqp_amd_shared_batch_adjoint_launches()
    assert product_lib.osqp_amd_shared_batch_adjoint(None, 1, buf.ctypes.data, None, buf.ctypes.data, *([None] * 8), 0) == 1
    assert b"null" in product_lib.osqp_amd_last_error()
    assert product_lib.osqp_amd_shared_batch_adjoint_launches() == before


def test_adjoint_checks_its_arguments_in_python():
    sb = batch.SharedBatch.__new__(batch.SharedBatch)  # the checks of a live handle, without a device
    sb.lib, sb.handle, sb.device = _NoLibrary(), None, 0
    sb.count, sb.n, sb.m, sb.nnzP, sb.nnzA = 3, 2, 3, 2, 4

    class Dev:  # a device array as far as the checks can tell
        def __init__(self, *shape, dtype="float64"):
            self.shape, self.dtype = shape, dtype

        def data_ptr(self):
            return 4096

    with pytest.raises(ValueError, match="dx and dy"):
        sb.adjoint()
    with pytest.raises(ValueError, match="sums"):
        sb.adjoint(dx=np.ones((3, 2)), sums=("q",))
    with pytest.raises(ValueError, match="sums"):
        sb.adjoint(dx=np.ones((3, 2)), sums=("Px_sum",))
    with pytest.raises(ValueError, match="want"):
        sb.adjoint(dx=np.ones((3, 2)), want=("q", "z"))
    with pytest.raises(ValueError, match="dx"):
        sb.adjoint(dx=np.ones((3, 3)))
    with pytest.raises(ValueError, match="dy"):
        sb.adjoint(dy=np.ones((2, 3)))
    with pytest.raises(ValueError, match="dimensions"):
        sb.adjoint(dx=np.ones((2, 3, 2)), dy=np.ones((3, 3)))
    with pytest.raises(ValueError, match="same number of cotangents"):
        sb.adjoint(dx=np.ones((2, 3, 2)), dy=np.ones((4, 3, 3)))
    with pytest.raises(ValueError, match="both"):  # host and device mixed
        sb.adjoint(dx=np.ones((3, 2)), dy=Dev(3, 3))
    with pytest.raises(ValueError, match="out"):  # host inputs take no out
        sb.adjoint(dx=np.ones((3, 2)), out=dict(q=Dev(3, 2)))
    with pytest.raises(ValueError, match="out"):  # device inputs need one
        sb.adjoint(dx=Dev(3, 2))
    with pytest.raises(ValueError, match="'Ax_sum'"):  # a wanted sum without its array
        sb.adjoint(dx=Dev(3, 2), want=("q",), sums=("Ax",), out=dict(q=Dev(3, 2)))
    with pytest.raises(ValueError, match="Px_sum"):  # wrong width
        sb.adjoint(dx=Dev(3, 2), want=(), sums=("Px",), out=dict(Px_sum=Dev(1, 3)))
    with pytest.raises(ValueError, match="Px_sum"):  # one row per cotangent
        sb.adjoint(dx=Dev(2, 3, 2), want=(), sums=("Px",), out=dict(Px_sum=Dev(1, 2)))
    with pytest.raises(ValueError, match="unknown"):
        sb.adjoint(dx=Dev(3, 2), want=("q",), out=dict(q=Dev(3, 2), x=Dev(3, 2)))
    sb.handle = None
