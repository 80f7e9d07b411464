"""Settings updates of the resident batch without a GPU: the null-handle refusal of osqp_amd_batch_update_setting, and what
`ResidentBatch.update_settings` does before and around the library call -- names, None values, the order of the calls,
`polish_refine_iter` kept current -- on a handle made with `__new__` and a stand-in library."""
import numpy as np
import pytest

from osqp_jl_amd import batch
from osqp_jl_amd.constants import UPDATABLE_SETTINGS
from osqp_jl_amd.interface import OSQPError
from test_batch_resident_host import _NoLibrary


def _handle(lib):
    rb = batch.ResidentBatch.__new__(batch.ResidentBatch)
    rb.lib, rb.handle, rb.device = lib, None, 0
    rb.count, rb.n, rb.m, rb.nnzP, rb.nnzA = 3, 2, 3, 2, 4
    rb.polish_refine_iter = 3
    return rb


class _Recorder:
    """Records the calls of osqp_amd_batch_update_setting; refuses the setting named in `refuse`."""

    def __init__(self, refuse=None):
        self.calls, self.refuse = [], refuse

    def osqp_amd_batch_update_setting(self, handle, name, value):
        self.calls.append((name.decode(), value))
        return 1 if name.decode() == self.refuse else 0

    def osqp_amd_last_error(self):
        return b"invalid value for the setting " + self.refuse.encode()


def test_update_setting_refuses_a_null_handle(product_lib):
    assert product_lib.osqp_amd_batch_update_setting(None, b"eps_abs", 1e-4) == 1
    assert b"handle" in product_lib.osqp_amd_last_error()


@pytest.mark.parametrize("name", ["sigma", "scaling", "adaptive_rho", "adaptive_rho_interval", "linsys_solver", "no_such_setting"])
def test_names_outside_the_list_raise_before_any_library_call(name):
    rb = _handle(_NoLibrary())
    with pytest.raises(OSQPError, match=f"{name} cannot be updated or is not recognized"):
        rb.update_settings(eps_abs=1e-4, **{name: 1})
    rb.handle = None


def test_none_values_are_skipped():
    rb = _handle(_NoLibrary())
    rb.update_settings(eps_abs=None, rho=None, polish=None)
    rb.update_settings()
    rb.handle = None


def test_calls_go_out_in_the_order_of_the_list_as_doubles():
    lib = _Recorder()
    rb = _handle(lib)
    given = dict(warm_start=False, scaled_termination=1, polish_refine_iter=5, polish=True, rho=0.5, eps_abs=1e-6, max_iter=np.int64(10),
                 eps_rel=None)
    rb.update_settings(**given)
    names = [c[0] for c in lib.calls]
    want = [k for k in list(UPDATABLE_SETTINGS) + ["scaled_termination"] if given.get(k) is not None]
    assert names == want, (names, want)
    assert all(isinstance(v, float) for _, v in lib.calls)
    assert dict(lib.calls) == dict(max_iter=10.0, eps_abs=1e-6, rho=0.5, polish=1.0, polish_refine_iter=5.0, warm_start=0.0, scaled_termination=1.0)
    assert rb.polish_refine_iter == 5
    rb.handle = None


def test_a_refused_setting_raises_and_stops_the_sequence():
    lib = _Recorder(refuse="alpha")
    rb = _handle(lib)
    with pytest.raises(OSQPError, match="alpha"):
        rb.update_settings(max_iter=10, alpha=2.0, polish_refine_iter=7)
    assert [c[0] for c in lib.calls] == ["max_iter", "alpha"]
    assert rb.polish_refine_iter == 3  # the call after the refused one was not made
    rb.handle = None
