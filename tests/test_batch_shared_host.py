"""The shared batch (batch.SharedBatch, osqp_amd_shared_batch_*) without a GPU: the reference stays inside the conditions
the GPU tests rest on, the host-only plan, and the naming of every new entry point in the header, batch.py and the Julia file."""
import os
import re

import numpy as np
import pytest

from osqp_jl_amd import batch
from osqp_jl_amd import types as T
import osqp_jl_amd as oq
import batch_entry_families as F
import batch_shared_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["osqp_amd_shared_batch_plan", "osqp_amd_shared_batch_setup", "osqp_amd_shared_batch_update_lin_cost",
                "osqp_amd_shared_batch_update_bounds", "osqp_amd_shared_batch_warm_start", "osqp_amd_shared_batch_resolve",
                "osqp_amd_shared_batch_update_setting", "osqp_amd_shared_batch_launches", "osqp_amd_shared_batch_destroy"]


@pytest.mark.parametrize("name", list(S.BOXED))
def test_boxed_reference_is_solved_below_max_iter(oracle_lib, name):
    base, q, l, u = S.boxed(name)
    refs = S.reference(oracle_lib, ("boxed", name), base, q, l, u, **S.OPTS)
    its = [r.info.iter for r in refs]
    print(name, its)
    assert all(r.info.status_val == 1 for r in refs)
    assert max(its) < S.OPTS["max_iter"]
    assert len(set(its)) > 1  # the counts differ inside one tile: the masking test needs that


@pytest.mark.parametrize("shape", S.CHAINS)
@pytest.mark.parametrize("variant", [dict(), dict(rho=0.1), dict(scaling=0)], ids=["rho1", "rho0.1", "unscaled"])
def test_chain_reference_statuses(oracle_lib, shape, variant):
    base, q, l, u = S.chain(*shape)
    opts = dict(S.OPTS, **variant)
    refs = S.reference(oracle_lib, ("chain", shape, tuple(sorted(variant.items()))), base, q, l, u, **opts)
    assert [r.info.status_val for r in refs] == S.CHAIN_STATUS
    assert all(25 <= r.info.iter <= 175 for r in refs), [r.info.iter for r in refs]


@pytest.mark.parametrize("shape", S.CHAINS)
def test_chain_reference_statuses_at_30_iterations(oracle_lib, shape):
    """At the iteration limit the approximate pass decides: every instance ends at iteration 30 with a status of its own
    (Solved inaccurate, an infeasibility, Max_iter).  The list CHAIN_STATUS_30 is the oracle's at (17, 5); the larger shapes
    give other mixes, which the GPU test compares instance by instance."""
    base, q, l, u = S.chain(*shape)
    refs = S.reference(oracle_lib, ("chain30", shape), base, q, l, u, **dict(S.OPTS, max_iter=30))
    got = [r.info.status_val for r in refs]
    print(shape, got, [r.info.iter for r in refs])
    if shape == S.CHAINS[0]:
        assert got == S.CHAIN_STATUS_30
    assert all(r.info.iter <= 30 for r in refs) and len(set(got)) >= 3


def test_unconstrained_reference_is_solved(oracle_lib):
    base, q, l, u = S.unconstrained()
    refs = S.reference(oracle_lib, ("m0",), base, q, l, u, **S.OPTS)
    assert all(r.info.status_val == 1 for r in refs)


def test_plan_depends_on_the_shape_alone(product_lib):
    shapes = [S.boxed(name, 1)[0] for name in S.BOXED] + [S.unconstrained()[0]] + [S.chain(*s, count=1)[0] for s in S.CHAINS]
    for P, _, A, _, _ in shapes:
        plan = batch.shared_plan(product_lib, P, A)
        print(A.shape, plan)
        assert plan["T"] in (4, 8, 16)
        assert plan["lds_bytes"] <= 160 * 1024
        assert plan == batch.shared_plan(product_lib, P, A)  # no argument carries a count: T cannot depend on one
        ldm = 16 * ((A.shape[1] + 15) // 16)
        assert plan["model_bytes"] >= 8 * ldm * ldm
    # the entry point itself takes (n, m, nnzA, nnzF, out): nothing about the number of instances
    assert len(T.EXT_SYMBOLS["osqp_amd_shared_batch_plan"][1]) == 5


def test_plan_refuses_what_does_not_fit(product_lib):
    out = np.zeros(4, dtype=np.int64)
    assert product_lib.osqp_amd_shared_batch_plan(257, 300, 1000, 700, out.ctypes.data) != 0
    assert b"n <= 256" in product_lib.osqp_amd_last_error()
    assert product_lib.osqp_amd_shared_batch_plan(256, 4000, 30000, 700, out.ctypes.data) != 0
    msg = product_lib.osqp_amd_last_error().decode()
    assert re.search(r"needs \d+ bytes of LDS", msg), msg
    P, A = F.pattern("banded", (256, 512, 6))
    assert batch.shared_plan(product_lib, P, A)["T"] >= 4


def test_null_handle_is_refused(product_lib):
    assert product_lib.osqp_amd_shared_batch_update_setting(None, b"eps_abs", 1e-4) == 1
    assert b"null" in product_lib.osqp_amd_last_error()
    assert product_lib.osqp_amd_shared_batch_destroy(None) == 0


def test_every_entry_point_is_named_in_header_python_and_julia():
    header = open(os.path.join(ROOT, "include", "osqp_amd.h")).read()
    py = open(os.path.join(ROOT, "osqp.jl_amd", "batch.py")).read()
    jl = open(os.path.join(ROOT, "osqp.jl_amd", "julia", "OSQPAMD.jl")).read()
    for sym in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in T.EXT_SYMBOLS, sym
        assert sym in py, sym
        assert ":" + sym in jl, sym
    for name in ("SharedBatch", "shared_plan"):
        assert hasattr(batch, name)
    for method in ("update", "warm_start", "solve", "update_settings", "close"):
        assert callable(getattr(batch.SharedBatch, method))
    assert hasattr(oq, "load_library")
