"""Polish, adjoint and JVP on resident handles with 128 < n <= 256 (osqp_amd_batch_large_factor)
without a GPU: the plan against the transcribed LDS layout, the refusals of the plan, the two symbols, and -- with the oracle
and numpy alone -- the conditions the GPU tests (test_batch_large_factor_gpu.py) rest on: every Solved instance of every shape
is polish-accepted under the three setting variants, the three numpy models agree with their references on these sizes, every
shape has enough non-degenerate active sets.

MEASURED[shape] = (polish model vs oracle, adjoint model vs `exact`, JVP model vs `exact`), worst over the seven instances
under default settings, relative to max(1, max|reference|), as measured when this file was written (the test prints the
figures of a run).  The GPU test's bounds derive from these: 1000 x the figure, never above 1e-9.  The bound of this file on a
model is 100 x the figure, as tests/test_batch_adjoint_host.py has it: the residue is rounding times the conditioning of the
active set."""
import os
import re

import numpy as np
import pytest

from osqp_jl_amd import batch
from osqp_jl_amd import types as T
import batch_adjoint_ref as adj
import batch_large_cases as L
import batch_large_factor_cases as C

MEASURED = {
    "banded-129x193x4": (1.4e-14, 9.6e-15, 6.7e-15),
    "random-144x200x7": (3.5e-15, 9.1e-15, 6.8e-15),
    "random-255x300x7": (3.7e-15, 8.0e-15, 1.6e-14),
    "random-256x384x7": (4.0e-15, 1.5e-14, 2.4e-14),
    "banded-256x512x6": (1.3e-14, 2.0e-14, 1.2e-14),
    "random-130x1x7": (7.8e-16, 7.2e-16, 9.9e-16),
    "nocon-130": (7.2e-16, 9.0e-16, 9.0e-16),
}
# Solved by the oracle and not polish-accepted, by name (shape, variant, instance): none.  (Instance 5 of random-255x300x7
# under scaling = 0 ends with status 2: it is not Solved, so nothing polishes it -- the GPU test's "left alone" case.)
NOT_ACCEPTED = set()
NOT_SOLVED = {("random-255x300x7", 1, 5): 2}
MIN_NONDEGENERATE = 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the plan --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(C.SHAPES)), ids=C.SHAPE_IDS)
def test_plan_is_the_transcribed_layout(product_lib, i):
    pat = C.pattern(i)
    n, m, nnzA, nnzF = L.pattern_counts(pat)
    plan = batch.large_factor_plan(product_lib, *pat)
    print(C.SHAPE_IDS[i], plan)
    assert plan == {"lds_bytes": C.lds_bytes(n, m, nnzA, nnzF), "scratch_bytes": 8 * n * n, "nb": C.NB}
    assert plan["lds_bytes"] <= C.LDS_LIMIT
    assert n % C.NB in ((1, 16, 31, 0, 0, 2, 2)[i],)  # n = 1 and n = 0 (mod NB) are among the shapes


def test_a_shape_over_the_limit_is_refused_with_its_bytes(product_lib):
    pat = L.dense_p_pattern(200, 300, 1)
    n, m, nnzA, nnzF = L.pattern_counts(pat)
    need = C.lds_bytes(n, m, nnzA, nnzF)
    assert need > C.LDS_LIMIT and nnzF < 65536
    out = np.full(3, -7, dtype=np.int64)
    assert product_lib.osqp_amd_batch_large_factor_plan(n, m, nnzA, nnzF, out.ctypes.data) == 1
    msg = product_lib.osqp_amd_last_error().decode()
    print(msg)
    assert msg.startswith("instance too large to polish") and f"needs {need} bytes of LDS" in msg
    assert np.all(out == -7)
    with pytest.raises(batch.OSQPError, match="instance too large to polish"):
        batch.large_factor_plan(product_lib, *pat)


@pytest.mark.parametrize("n", [1, 100, 128, 257, 300])
def test_sizes_outside_the_range_are_refused(product_lib, n):
    out = np.full(3, -7, dtype=np.int64)
    assert product_lib.osqp_amd_batch_large_factor_plan(n, 10, 40, 3 * n, out.ctypes.data) == 1
    assert b"128 < n <= 256" in product_lib.osqp_amd_last_error() and np.all(out == -7)
    assert product_lib.osqp_amd_batch_large_factor_plan(129, 10, 40, 387, None) == 0  # no output array: the verdict alone


# ---- the symbols -----------------------------------------------------------------------------------------------------------------
def test_the_two_symbols_are_declared_bound_and_exported(product_lib):
    header = open(os.path.join(ROOT, "include", "osqp_amd.h")).read()
    julia = open(os.path.join(ROOT, "osqp.jl_amd", "julia", "OSQPAMD.jl")).read()
    for name, nargs in (("osqp_amd_batch_large_factor", 2), ("osqp_amd_batch_large_factor_plan", 5)):
        assert re.search(r"^c_int %s\(" % name, header, re.M), name
        assert ":%s," % name in julia, name
        assert name in T.EXT_SYMBOLS, name
        res, args = T.EXT_SYMBOLS[name]
        assert res is T.c_int and len(args) == nargs
        fn = getattr(product_lib, name)  # AttributeError: not exported
        assert fn.restype is T.c_int and list(fn.argtypes) == list(args)


def test_a_null_handle_is_refused_and_launches_nothing(product_lib):
    lib = product_lib
    counts = lambda: (lib.osqp_amd_batch_polish_launches(), lib.osqp_amd_batch_adjoint_launches(), lib.osqp_amd_batch_jvp_launches())
    before = counts()
    for on in (0, 1):
        assert lib.osqp_amd_batch_large_factor(None, on) == -1
        assert b"handle" in lib.osqp_amd_last_error()
    assert counts() == before


# ---- what the GPU tests rest on ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", range(len(C.VARIANTS)), ids=C.VARIANT_IDS)
@pytest.mark.parametrize("i", range(len(C.SHAPES)), ids=C.SHAPE_IDS)
def test_every_solved_instance_is_polish_accepted(oracle_lib, i, variant):
    runs = C.oracle_runs(oracle_lib, i, variant)
    sid = C.SHAPE_IDS[i]
    status = [r["polished"].info.status_val for r in runs]
    accepted = [r["polished"].info.status_polish for r in runs]
    moved = [C.rel(r["polished"].x, r["plain"].x) for r in runs if r["polished"].info.status_polish == 1]
    print(f"{sid}/{C.VARIANT_IDS[variant]}: status {status} status_polish {accepted} polished vs unpolished x {min(moved):.1e} .. {max(moved):.1e}")
    for k, r in enumerate(runs):
        assert r["plain"].info.status_val == r["polished"].info.status_val == NOT_SOLVED.get((sid, variant, k), 1), (sid, variant, k)
        want = 0 if status[k] != 1 else (-1 if (sid, variant, k) in NOT_ACCEPTED else 1)
        assert accepted[k] == want, (sid, variant, k, accepted[k])


@pytest.mark.parametrize("i", range(len(C.SHAPES)), ids=C.SHAPE_IDS)
def test_the_models_agree_with_their_references(oracle_lib, i):
    got = C.model_figures(oracle_lib, i)
    sid = C.SHAPE_IDS[i]
    print(f"MEASURED[{sid!r}] = ({got[0]:.1e}, {got[1]:.1e}, {got[2]:.1e})   recorded {MEASURED[sid]}")
    for g, rec, what in zip(got, MEASURED[sid], ("polish", "adjoint", "jvp")):
        assert g <= 100 * rec, (sid, what, g, rec)


@pytest.mark.parametrize("i", range(len(C.SHAPES)), ids=C.SHAPE_IDS)
def test_every_shape_has_non_degenerate_active_sets(oracle_lib, i):
    probs, runs = C.problems(i)[1], C.oracle_runs(oracle_lib, i)
    good = [k for k, (p, r) in enumerate(zip(probs, runs)) if r["polished"].info.status_val == 1 and adj.nondegenerate(p[2], r["act"], len(p[1]))]
    active = [int(np.count_nonzero(r["act"])) for r in runs]
    print(f"{C.SHAPE_IDS[i]}: non-degenerate {good}, active rows {active}")
    assert len(good) >= MIN_NONDEGENERATE
