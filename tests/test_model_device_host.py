"""The checks `interface.update` / `warm_start` / `adjoint` / `jvp` / `solution` make on device arrays before the library is
called (no device needed: stand-in objects with `data_ptr()` / `shape` / `dtype`, a model that was never set up or a stub
whose library refuses to be called), and the declarations of the device-pointer forms in include/osqp_amd.h."""
import numpy as np
import pytest

from osqp_jl_amd import interface
from osqp_jl_amd import types as T
from test_abi_exports import _declared_symbols

DEVICE_FORMS = (
    "osqp_amd_update_vectors_dev", "osqp_amd_update_values_dev", "osqp_amd_warm_start_dev", "osqp_amd_solution_dev",
    "osqp_amd_adjoint_dev", "osqp_amd_jvp_dev", "osqp_amd_device_form_calls",
)


class Dev:
    """What `interface` takes for a device array: an address, a shape, an element type."""

    def __init__(self, *shape, dtype="float64", contiguous=True):
        self.shape, self.dtype, self._contiguous = tuple(shape), dtype, contiguous

    def data_ptr(self):
        return 4096

    def is_contiguous(self):
        return self._contiguous


class _NoCall:
    """A library that must not be reached."""

    class _Fn:
        argtypes = ()

        def __call__(self, *a):
            raise AssertionError("the library was called")

    def __getattr__(self, name):
        return _NoCall._Fn()


def _never_set_up():
    mdl = interface.Model.__new__(interface.Model)
    mdl.lib = _NoCall()
    mdl.workspace = T.Workspace_p()
    mdl.isempty = True
    return mdl


def _stub(n, m):
    mdl = interface.Model.__new__(interface.Model)
    mdl.lib = _NoCall()
    data = T.Data(n, m, None, None, None, None, None)
    ws = T.Workspace()
    ws.data = T.C.pointer(data)
    mdl._keep = (data, ws)
    mdl.workspace = T.C.pointer(ws)
    mdl.isempty = False
    return mdl


def _done(mdl):
    mdl.workspace = T.Workspace_p()  # nothing for __del__ to clean


def test_mixing_the_forms_raises():
    mdl = _never_set_up()
    with pytest.raises(ValueError, match="one form per call"):
        interface.update(mdl, q=Dev(3), l=np.zeros(2))
    with pytest.raises(ValueError, match="one form per call"):
        interface.update(mdl, q=np.zeros(3), Ax=Dev(5))
    with pytest.raises(ValueError, match="one form per call"):
        interface.warm_start(mdl, x=Dev(3), y=[0.0, 0.0])
    with pytest.raises(ValueError, match="one form per call"):
        interface.adjoint(mdl, dx=Dev(3), dy=np.zeros(2))
    with pytest.raises(ValueError, match="one form per call"):
        interface.jvp(mdl, q=np.zeros(3), l=Dev(2))
    with pytest.raises(ValueError, match="device array"):
        interface.solution(mdl, x=np.zeros(3))
    with pytest.raises(ValueError, match="out="):
        interface.adjoint(mdl, dx=np.zeros(3), out=dict(q=Dev(3)))


def test_wrong_dtype_layout_or_shape_raises():
    mdl = _stub(3, 2)
    try:
        for call in (
            lambda a: interface.update(mdl, q=a),
            lambda a: interface.warm_start(mdl, x=a),
            lambda a: interface.adjoint(mdl, dx=a, want=("q",)),
            lambda a: interface.jvp(mdl, q=a),
            lambda a: interface.solution(mdl, x=a),
        ):
            with pytest.raises(ValueError, match="float64"):
                call(Dev(3, dtype="float32"))
            with pytest.raises(ValueError, match="contiguous"):
                call(Dev(3, contiguous=False))
            with pytest.raises(ValueError, match="shape"):
                call(Dev(4))
        with pytest.raises(ValueError, match="shape"):
            interface.update(mdl, q=Dev(3), l=Dev(3))
        with pytest.raises(ValueError, match="shape"):
            interface.update(mdl, q=Dev(2, 3))  # a vector: no leading axis
        with pytest.raises(ValueError, match="shape"):
            interface.warm_start(mdl, x=Dev(3), y=Dev(3))
        with pytest.raises(ValueError, match="leading"):
            interface.adjoint(mdl, dx=Dev(3), dy=Dev(1, 2), want=("q",))
        with pytest.raises(ValueError, match="leading"):
            interface.adjoint(mdl, dx=Dev(2, 3), dy=Dev(3, 2), want=("q",))
        with pytest.raises(ValueError, match="shape"):
            interface.adjoint(mdl, dx=Dev(0, 3), want=("q",))
        with pytest.raises(ValueError, match="shape"):
            interface.adjoint(mdl, dx=Dev(2, 3), want=("q",), out=dict(q=Dev(3)))
        with pytest.raises(ValueError, match="float64"):
            interface.adjoint(mdl, dx=Dev(3), want=("q",), out=dict(q=Dev(3, dtype="float16")))
        with pytest.raises(ValueError, match="device array"):
            interface.adjoint(mdl, dx=Dev(3), want=("q",), out=dict(q=np.zeros(3)))
        with pytest.raises(ValueError, match="shape"):
            interface.jvp(mdl, q=Dev(2, 3), out=dict(x=Dev(3)))
    finally:
        _done(mdl)


def test_indices_with_device_values_raise():
    mdl = _never_set_up()
    with pytest.raises(ValueError, match="Px_idx"):
        interface.update(mdl, Px=Dev(2), Px_idx=np.array([0, 1]))
    with pytest.raises(ValueError, match="Ax_idx"):
        interface.update(mdl, Px=Dev(2), Ax=Dev(2), Ax_idx=np.array([0, 1]))


def test_the_header_declares_the_device_forms():
    names = _declared_symbols()
    for sym in DEVICE_FORMS:
        assert sym in names, sym
        assert sym in T.EXT_SYMBOLS, sym
