"""Polish of the resident batch without a GPU: the numpy model of the kernel's linear algebra (tests/batch_polish_ref.py:
the condensed regularised KKT system, Cholesky, refinement against the unregularised matrix) held to the oracle's polish on
the families of the resident tests, the two new symbols, and the argument checks of `ResidentBatch.update_polish`."""
import numpy as np
import pytest

import osqp_jl_amd as oq
from osqp_jl_amd import batch
from osqp_jl_amd import types as T
import batch_polish_ref as pol
import batch_resident_ref as ref
from test_batch_gpu import _family
from test_batch_resident_host import _NoLibrary

VARIANTS = [dict(), dict(scaling=0), dict(scaled_termination=1)]
# Tolerances of the model against the oracle, relative to max(1, max|ref|).  Both sides solve the same regularised system
# and refine against the same unregularised one; the elimination of the constraint block is exact, so what remains is
# rounding amplified by the conditioning of the active set.  Measured (this file prints the figures): x <= 4e-13 on every
# family; y <= 3e-11 on mpc / quad64, and 1.9e-8 on rows300, where more rows are active than there are variables, the
# multipliers are fixed only by the delta-regularisation, and three refinement steps leave them at that level on BOTH sides.
# x: 1e-10.  y: 1e-6, the bound the GPU test may not exceed either (polished and unpolished solutions differ by ~1e-4).
TOL_X, TOL_Y = 1e-10, 1e-6


def _probs(oracle_lib, family):
    if family == "mpc":
        return ref.mpc_instances(oracle_lib, 0, 64, 2)
    return _family(64, 100, 6, 640100)[1] if family == "quad64" else _family(40, 300, 5, 40300)[1]


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("family", ["mpc", "quad64", "rows300"])
def test_model_reproduces_the_oracles_polish(oracle_lib, family, variant):
    """Input: the oracle's unpolished result (polish=False), its scaling and scaled iterate.  The model must give the
    oracle's status_polish on EVERY instance and its polished x, y, residuals on the accepted ones."""
    opts = dict(ref.OPTS, **VARIANTS[variant])
    scaling = opts.get("scaling", 10)
    unscaled = bool(scaling) and not opts.get("scaled_termination", 0)
    ex = ey = 0.0
    accepted = solved = 0
    for i, (P, q, A, l, u) in enumerate(_probs(oracle_lib, family)):
        plain, polished = oq.Model(oracle_lib), oq.Model(oracle_lib)
        oq.setup(plain, P=P, q=q, A=A, l=l, u=u, polish=False, **opts)
        oq.setup(polished, P=P, q=q, A=A, l=l, u=u, polish=True, **opts)
        r0, r1 = oq.solve(plain), oq.solve(polished)
        if r0.info.status_val != 1:
            assert r1.info.status_polish == 0
        else:
            solved += 1
            state = pol.oracle_state(plain, len(q), len(l), scaling)
            out = pol.polish(P, q, A, l, u, *state, r0.info.pri_res, r0.info.dua_res, delta=1e-6, refine=3, unscaled=unscaled)
            assert out["status"] == r1.info.status_polish, (family, variant, i, out["status"], r1.info.status_polish)
            if out["status"] == 1:
                accepted += 1
                ex = max(ex, float(np.max(np.abs(out["x"] - r1.x))) / max(1.0, float(np.max(np.abs(r1.x)))))
                ey = max(ey, float(np.max(np.abs(out["y"] - r1.y))) / max(1.0, float(np.max(np.abs(r1.y)))))
                assert out["pri_res"] < r0.info.pri_res or out["dua_res"] < r0.info.dua_res
                assert abs(out["obj_val"] - r1.info.obj_val) <= 1e-9 * max(1.0, abs(r1.info.obj_val))
            else:
                assert np.array_equal(out["xs"], state[3])
        oq.clean(plain); oq.clean(polished)
    print(f"{family}/{variant}: solved {solved} accepted {accepted} rel dx {ex:.2e} dy {ey:.2e}")
    assert accepted >= (20 if family == "mpc" else 5)
    assert ex <= TOL_X and ey <= TOL_Y, (ex, ey)


def test_the_two_polish_symbols_are_bound_and_exported(product_lib):
    for name, nargs in (("osqp_amd_batch_polish_status", 3), ("osqp_amd_batch_update_polish", 3)):
        assert name in T.EXT_SYMBOLS, name
        res, args = T.EXT_SYMBOLS[name]
        assert res is T.c_int and len(args) == nargs
        fn = getattr(product_lib, name)  # AttributeError: not exported
        assert fn.restype is T.c_int and list(fn.argtypes) == list(args)


def test_update_polish_checks_its_arguments_in_python():
    rb = batch.ResidentBatch.__new__(batch.ResidentBatch)  # the checks of a live handle, without a device
    rb.lib, rb.handle, rb.device = _NoLibrary(), None, 0
    rb.count, rb.n, rb.m, rb.nnzP, rb.nnzA = 3, 2, 3, 2, 4
    for bad in (2, -1, 0.5, None, "on"):
        with pytest.raises(ValueError, match="polish"):
            rb.update_polish(bad)
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="polish_refine_iter"):
            rb.update_polish(1, bad)
    with pytest.raises(ValueError, match="out"):
        rb.polish_status(out=np.zeros(3))
    rb.handle = None


def test_polish_entries_refuse_a_null_handle(product_lib):
    """Both calls go through the resident handle check: no handle, return 1 and a message."""
    buf = np.zeros(4)
    assert product_lib.osqp_amd_batch_polish_status(None, buf.ctypes.data, 0) == 1
    assert b"handle" in product_lib.osqp_amd_last_error()
    assert product_lib.osqp_amd_batch_update_polish(None, 1, 3) == 1
    assert b"handle" in product_lib.osqp_amd_last_error()
