"""osqp_amd_adjoint_retain without a GPU: the header, the symbols and their bindings, the NULL
workspace, the argument check of `interface.adjoint_retain`, a library without the symbols, and the new argument of
`qp_layer.QPLayer` (False by default: nothing is called)."""
import inspect
import os
import re

import numpy as np
import pytest

import osqp_jl_amd as oq
from osqp_jl_amd import interface
from osqp_jl_amd import types as T
import model_adjoint_ref as mar
from test_model_adjoint_host import _fake_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = (("osqp_amd_adjoint_retain", 2), ("osqp_amd_adjoint_retain_stats", 3))
FIELDS = ("mode", "checks", "reused", "refactorised", "rebuilt_active_set", "rebuilt_failed", "last_rows_changed", "stale")


def test_the_header_declares_and_the_library_exports_the_symbols(product_lib):
    text = open(os.path.join(ROOT, "include", "osqp_amd.h")).read()
    for name, nargs in SYMBOLS:
        assert re.search(r"c_int\s+" + name + r"\s*\(", text), name
        assert name in T.EXT_SYMBOLS, name
        res, args = T.EXT_SYMBOLS[name]
        assert res is T.c_int and len(args) == nargs
        fn = getattr(product_lib, name)  # AttributeError: not exported
        assert fn.restype is T.c_int and list(fn.argtypes or []) == list(args)
    assert re.search(r"#define\s+OSQP_AMD_ADJOINT_RETAIN_STATS_COUNT\s+8\b", text)
    assert interface.ADJOINT_RETAIN_STATS_FIELDS == FIELDS
    assert oq.adjoint_retain is interface.adjoint_retain and oq.adjoint_retain_stats is interface.adjoint_retain_stats


def test_a_null_workspace(product_lib):
    buf = np.full(8, np.nan)
    assert product_lib.osqp_amd_adjoint_retain(None, 1) == 7
    assert b"workspace" in product_lib.osqp_amd_last_error()
    assert product_lib.osqp_amd_adjoint_retain_stats(None, buf.ctypes.data_as(T.c_float_p), 8) == 0 and np.all(np.isnan(buf))


class _Recorder:
    """A library of the two symbols that records its calls and reports a retained state after a reuse."""

    def __init__(self):
        self.calls = []
        outer = self

        class _Fn:
            argtypes = ()

            def __init__(self, name):
                self.name = name

            def __call__(self, *a):
                outer.calls.append((self.name,) + a[1:])
                if self.name == "osqp_amd_adjoint_retain_stats":
                    out = np.ctypeslib.as_array(a[1], (8,))
                    out[:] = (1, 3, 2, 0, 1, 0, 5, 0)
                    return a[2]
                return 0

        self.osqp_amd_adjoint_retain = _Fn("osqp_amd_adjoint_retain")
        self.osqp_amd_adjoint_retain_stats = _Fn("osqp_amd_adjoint_retain_stats")


def test_the_python_face():
    mdl = _fake_model(3, 2)
    nocall = mdl.lib
    try:
        for bad in (1, 0, "on", None):
            with pytest.raises(ValueError, match="on"):
                interface.adjoint_retain(mdl, bad)
        mdl.lib = rec = _Recorder()
        interface.adjoint_retain(mdl)
        interface.adjoint_retain(mdl, False)
        assert rec.calls == [("osqp_amd_adjoint_retain", 1), ("osqp_amd_adjoint_retain", 0)]
        st = interface.adjoint_retain_stats(mdl)
        assert tuple(st) == FIELDS and all(isinstance(v, int) for v in st.values())
        assert st == dict(mode=1, checks=3, reused=2, refactorised=0, rebuilt_active_set=1, rebuilt_failed=0, last_rows_changed=5, stale=0)
    finally:
        mdl.lib = nocall
        mdl.workspace = T.Workspace_p()  # nothing for __del__ to clean


def test_a_library_without_the_symbols_raises(oracle_lib):
    p = mar.problems(oracle_lib, "spd7")[0]
    mdl = oq.Model(oracle_lib)
    oq.setup(mdl, **mar.setup_args(p), verbose=False)
    for call in (lambda: oq.adjoint_retain(mdl), lambda: oq.adjoint_retain(mdl, False), lambda: oq.adjoint_retain_stats(mdl)):
        with pytest.raises(oq.OSQPError, match="does not export"):
            call()
    oq.clean(mdl)


def test_the_layer_argument_defaults_to_off_and_calls_nothing():
    from osqp_jl_amd.qp_layer import QPLayer

    assert inspect.signature(QPLayer.__init__).parameters["retain_factor"].default is False
    mdl = _fake_model(3, 2)
    nocall = mdl.lib
    try:
        QPLayer(mdl)  # the fake library raises on any call
        QPLayer(mdl, retain_factor=False)
        mdl.lib = rec = _Recorder()
        QPLayer(mdl, retain_factor=True)
        assert rec.calls == [("osqp_amd_adjoint_retain", 1)]
    finally:
        mdl.lib = nocall
        mdl.workspace = T.Workspace_p()
