"""The boundary of the gap stopping rule of the resident batch, without a GPU: the three calls are declared, exported and
bound, they refuse a null handle with its message, and the Python and Julia layers name them.  (A handle that
osqp_amd_batch_setup did not create can only be made on a device: tests/test_batch_gap_rule_gpu.py holds that refusal.)"""
import ctypes as C
import os
import re

import osqp_jl_amd as oq
from osqp_jl_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("osqp_amd_batch_duality_gap_check", "osqp_amd_batch_gap_refusals", "osqp_amd_batch_gap_refusals_rows")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", _read("include", "osqp_amd.h"), flags=re.S)
    lib = oq.load_library()
    for sym in SYMBOLS:
        assert re.search(r"\bc_int\s+%s\s*\(" % sym, header), sym
        assert sym in T.EXT_SYMBOLS and hasattr(lib, sym), sym
        assert getattr(lib, sym).argtypes == T.EXT_SYMBOLS[sym][1]
    assert C.sizeof(T.Settings) == 176  # the rule is state of the handle, not a setting


def test_a_null_handle_is_refused():
    lib = oq.load_library()
    out = (C.c_double * 4)()
    rows = (T.c_int * 1)(0)
    for rc in (lib.osqp_amd_batch_duality_gap_check(None, 1), lib.osqp_amd_batch_duality_gap_check(None, 0),
               lib.osqp_amd_batch_gap_refusals(None, C.addressof(out), 0), lib.osqp_amd_batch_gap_refusals_rows(None, rows, 1, C.addressof(out), 0)):
        assert rc == 1
        assert lib.osqp_amd_last_error() == b"null batch handle"


def test_the_host_layers_name_the_symbols():
    py, layer, jl = _read("osqp.jl_amd", "batch.py"), _read("osqp.jl_amd", "qp_layer.py"), _read("osqp.jl_amd", "julia", "OSQPAMD.jl")
    for sym in SYMBOLS:
        assert sym in py and ":" + sym in jl, sym
    assert "def duality_gap_check(self, on=True)" in py and "def gap_refusals(self, out=None, rows=None)" in py
    assert "duality_gap_check=False" in layer
    assert "function batch_duality_gap_check!(" in jl and "function batch_gap_refusals(" in jl
