"""The resident batch (osqp_amd_batch_setup ... _resolve) without a GPU: the Python signatures, the argument checks of
`batch.ResidentBatch`, the loud failure without a device, and the oracle-side reference driver the GPU tests compare with."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_jl_amd as oq
from osqp_jl_amd import batch
from osqp_jl_amd import types as T
import batch_resident_ref as ref

SYMBOLS = {
    "osqp_amd_batch_setup": 15,
    "osqp_amd_batch_update_lin_cost": 3,
    "osqp_amd_batch_update_bounds": 4,
    "osqp_amd_batch_update_matrices": 4,
    "osqp_amd_batch_warm_start": 4,
    "osqp_amd_batch_resolve": 5,
}


def test_the_six_symbols_are_bound_and_exported(product_lib):
    for name, nargs in SYMBOLS.items():
        assert name in T.EXT_SYMBOLS, name
        res, args = T.EXT_SYMBOLS[name]
        assert res is T.c_int and len(args) == nargs and args[-1] is T.c_int, name  # ..., where / device
        fn = getattr(product_lib, name)  # AttributeError: not exported
        assert fn.restype is T.c_int and list(fn.argtypes) == list(args)
    assert T.EXT_SYMBOLS["osqp_amd_batch_setup"][1][0] == C.POINTER(C.c_void_p)
    assert batch.ResidentBatch is not None


def _tiny(count=3):
    P = sp.identity(2, format="csc"); A = sp.csc_matrix(np.array([[1.0, 1.0], [1.0, 0.0], [0.0, 1.0]]))
    return P, A, np.ones((count, 2)), np.ones((count, 4)), np.ones((count, 2)), -np.ones((count, 3)), np.ones((count, 3))


class _NoLibrary:
    """Stands in for the library where the call must fail before it is reached."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


@pytest.mark.parametrize("arg,bad,word", [
    (2, np.ones((3, 3)), "Px_all"),          # wrong width
    (3, np.ones((3, 5)), "Ax_all"),
    (4, np.ones(2), "q_all"),                # not [count x n]
    (5, -np.ones((2, 3)), "l_all"),          # count mismatch
    (6, np.ones((3, 2)), "u_all"),
    (5, np.array([["a"] * 3] * 3), "l_all"),  # not numeric
])
def test_resident_batch_checks_setup_arguments_in_python(arg, bad, word):
    args = list(_tiny())
    args[arg] = bad
    with pytest.raises((ValueError, oq.OSQPError), match=word):
        batch.ResidentBatch(_NoLibrary(), *args, verbose=False)


def test_resident_batch_checks_update_arguments_in_python():
    rb = batch.ResidentBatch.__new__(batch.ResidentBatch)  # the checks of a live handle, without a device
    rb.lib, rb.handle, rb.device = _NoLibrary(), None, 0
    rb.count, rb.n, rb.m, rb.nnzP, rb.nnzA = 3, 2, 3, 2, 4
    for kwargs, word in ((dict(q=np.ones((3, 3))), "q"), (dict(l=np.ones((2, 3))), "l"), (dict(u=np.ones(3)), "u"),
                         (dict(Px=np.ones((3, 4))), "Px"), (dict(Ax=np.ones((3, 2))), "Ax"),
                         (dict(q=np.array([[1j, 0]] * 3)), "q")):
        with pytest.raises(ValueError, match=word):
            rb.update(**kwargs)
    with pytest.raises(oq.OSQPError, match="lower bound"):
        rb.update(l=np.ones((3, 3)), u=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="x"):
        rb.warm_start(x=np.ones((3, 3)))
    with pytest.raises(ValueError, match="y"):
        rb.warm_start(y=np.ones((3, 2)))

    class Dev:  # a device array of the wrong type / shape
        def __init__(self, shape, dtype="float64"):
            self.shape, self.dtype = shape, dtype

        def data_ptr(self):
            return 4096

    with pytest.raises(ValueError, match="q"):
        rb.update(q=Dev((3, 2), "float32"))
    with pytest.raises(ValueError, match="l"):
        rb.update(l=Dev((3, 4)))
    with pytest.raises(ValueError, match="both"):
        rb.update(l=Dev((3, 3)), u=np.ones((3, 3)))
    with pytest.raises(ValueError, match=r"out\[1\]"):
        rb.solve(out=(Dev((3, 2)), Dev((3, 2)), Dev((3, 6))))
    rb.handle = None  # nothing for __del__ to free


def test_resident_batch_without_a_device_fails_loudly(product_lib):
    """Without a HIP device the setup raises; it never computes anywhere else."""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    with pytest.raises(oq.OSQPError):
        batch.ResidentBatch(product_lib, *_tiny(), verbose=False)


def test_reference_driver_follows_updates_and_warm_starts(oracle_lib):
    """The oracle half of the GPU tests on four MPC instances: a repeated solve ends at its first check, an update of q
    before the first solve keeps the scaling of the setup data, a warm start at the solution ends at the first check."""
    probs = ref.mpc_instances(oracle_lib, 0, 4, 5)
    ob = ref.OracleBatch(oracle_lib, probs, **ref.OPTS)
    first = ob.solve()
    again = ob.solve()
    assert all(r.info.status_val == 1 and 75 <= r.info.iter <= 125 for r in first)
    assert all(r.info.status_val == 1 and r.info.iter == 25 for r in again)
    _, _, _, _, q, l, u = ref.stack(probs)
    ob.update(q=1.01 * q, l=l, u=u)
    moved = ob.solve()
    assert all(r.info.status_val == 1 for r in moved)
    cold = ref.cold_oracle(oracle_lib, ref.with_vectors(probs, q=1.01 * q), **ref.OPTS)
    assert all(np.max(np.abs(a.x - b.x)) <= 50 * 1e-5 * max(1.0, np.max(np.abs(b.x))) for a, b in zip(moved, cold))
    ob.warm_start(x=np.array([r.x for r in cold]), y=np.array([r.y for r in cold]))
    assert all(r.info.iter == 25 for r in ob.solve())
    ob.close()
    # scaling comes from the setup data: MPC instance 2 of seed 2, q <- 3 q + 1 before the first solve
    p2 = ref.mpc_instances(oracle_lib, 2, 1, 2)
    ob = ref.OracleBatch(oracle_lib, p2, **ref.OPTS)
    ob.update(q=np.array([3 * p2[0][1] + 1]))
    kept = ob.solve()[0]
    fresh = ref.cold_oracle(oracle_lib, ref.with_vectors(p2, q=np.array([3 * p2[0][1] + 1])), **ref.OPTS)[0]
    ob.close()
    assert (kept.info.iter, fresh.info.iter) == (150, 100)


def test_oracle_totals_of_the_closed_loop_family(oracle_lib):
    """The condition of the GPU test 'warm starting pays' on the reference alone: 16 MPC instances of seed 5, six solves,
    the totals of ADMM iterations per step of one updated model (warm) against a fresh setup + solve (cold).  The totals
    pinned here are the oracle's own for the draw order of `closed_loop_steps` (3 725 warm against 7 775 cold over steps
    1 .. 5; no instance-step has warm > cold)."""
    probs = ref.mpc_instances(oracle_lib, 0, 16, 5)
    _, _, _, _, q, l, u = ref.stack(probs)
    steps = ref.closed_loop_steps(q, l, u)
    warm, cold = ref.closed_loop_oracle(oracle_lib, probs, steps, **ref.OPTS)
    wt = [sum(r.info.iter for r in rs) for rs in warm]
    ct = [sum(r.info.iter for r in rs) for rs in cold]
    print("oracle warm", wt, "cold", ct)
    assert all(r.info.status_val == 1 for rs in warm + cold for r in rs)
    assert wt == [1550, 650, 900, 675, 825, 675] and ct == [1550, 1550, 1525, 1575, 1575, 1550]
    assert all(a.info.iter <= b.info.iter for ws, cs in zip(warm, cold) for a, b in zip(ws, cs))
    assert sum(wt[1:]) < sum(ct[1:])
