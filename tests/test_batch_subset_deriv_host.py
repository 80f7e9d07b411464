"""The host side of the reading calls of the resident batch for a selection (`rows=` of batch.ResidentBatch.adjoint / jvp /
certificates / polish_status, and of qp_layer.BatchQPLayer): the declarations of the four new entry points, what the Python
methods hand to the library -- on a handle without a device, with a recording stand-in for the library -- and the
per-instance stamps of the torch layer.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from osqp_jl_amd import batch
from osqp_jl_amd import types as T

ROWS_SYMBOLS = {
    "osqp_amd_batch_adjoint_rows": 13,
    "osqp_amd_batch_jvp_rows": 14,
    "osqp_amd_batch_polish_status_rows": 5,
    "osqp_amd_batch_certificates_rows": 6,
}
N, M, NNZP, NNZA, COUNT = 4, 3, 6, 5, 7


def test_the_four_entries_are_declared():
    """rows (an integer pointer) and k directly after the handle, then the whole-batch signature."""
    for name, nargs in ROWS_SYMBOLS.items():
        assert name in T.EXT_SYMBOLS, name
        restype, argtypes = T.EXT_SYMBOLS[name]
        assert restype is T.c_int and len(argtypes) == nargs, (name, argtypes)
        assert argtypes[1] is T.c_int_p and argtypes[2] is T.c_int and argtypes[-1] is T.c_int, (name, argtypes)
        whole = T.EXT_SYMBOLS[name[: -len("_rows")]][1]
        assert argtypes[:1] + argtypes[3:] == whole, (name, argtypes, whole)


def test_the_header_declares_them():
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "osqp_amd.h")).read()
    for name in ROWS_SYMBOLS:
        assert f"c_int {name}(osqp_amd_batch *batch, const c_int *rows, c_int k," in header, name


class _Recorder:
    """Stands in for the library: every entry returns 0 and is recorded as (name, args); the selection of a *_rows call is
    read from its pointer while the call runs."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            if name.endswith("_rows"):
                k = args[2]
                sel = np.ctypeslib.as_array(C.cast(args[1], C.POINTER(C.c_int64)), shape=(k,)).tolist()
                self.calls.append((name, k, sel, args[3:]))
            else:
                self.calls.append((name, None, None, args[1:]))
            return 0

        return entry


def _handle():
    rb = object.__new__(batch.ResidentBatch)
    rb.n, rb.m, rb.nnzP, rb.nnzA, rb.count = N, M, NNZP, NNZA, COUNT
    rb.lib, rb.handle = _Recorder(), None
    return rb


class _Dev:
    """A device array as far as the host side can tell: a shape and an address."""

    def __init__(self, *shape):
        self.shape, self.dtype = shape, "float64"

    def data_ptr(self):
        return 4096


def test_int64_is_the_librarys_integer():
    assert C.sizeof(T.c_int) == 8  # what _Recorder reads the selection as


def test_adjoint_hands_the_selection_and_compact_arrays():
    rb = _handle()
    sel = [6, 0, 2]
    g = rb.adjoint(dx=np.ones((3, N)), dy=np.ones((3, M)), rows=sel)
    (name, k, got, rest), = rb.lib.calls
    assert name == "osqp_amd_batch_adjoint_rows" and k == 3 and got == sel
    assert len(rest) == 10 and rest[-1] == 0 and all(p is not None for p in rest[:9])
    assert {key: g[key].shape for key in g} == dict(q=(3, N), l=(3, M), u=(3, M), Px=(3, NNZP), Ax=(3, NNZA), act=(3, M), status=(3,))
    rb.lib.calls.clear()
    g = rb.adjoint(dx=np.ones((1, N)), want=("q",), rows=[4])  # k = 1, a want subset, no dy
    (name, k, got, rest), = rb.lib.calls
    assert name == "osqp_amd_batch_adjoint_rows" and k == 1 and got == [4]
    assert rest[1] is None and rest[2] is not None and rest[3:7] == (None,) * 4 and sorted(g) == ["act", "q", "status"]


def test_adjoint_device_form():
    rb = _handle()
    out = dict(q=_Dev(2, N), Ax=_Dev(2, NNZA), status=_Dev(2, 1))
    assert rb.adjoint(dx=_Dev(2, N), want=("q", "Ax"), out=out, rows=[5, 1]) is out
    (name, k, got, rest), = rb.lib.calls
    assert name == "osqp_amd_batch_adjoint_rows" and got == [5, 1] and rest[-1] == 1
    with pytest.raises(ValueError, match=r"out\['q'\]"):
        rb.adjoint(dx=_Dev(2, N), want=("q",), out=dict(q=_Dev(COUNT, N)), rows=[5, 1])
    with pytest.raises(ValueError, match="both"):
        rb.adjoint(dx=_Dev(2, N), dy=np.ones((2, M)), out=out, rows=[5, 1])
    assert len(rb.lib.calls) == 1


def test_jvp_hands_the_selection_and_compact_arrays():
    rb = _handle()
    sel = [6, 0, 2]
    t = rb.jvp(q=np.ones((2, 3, N)), Ax=np.ones((2, 3, NNZA)), rows=sel)
    (name, k, got, rest), = rb.lib.calls
    assert name == "osqp_amd_batch_jvp_rows" and k == 3 and got == sel
    assert len(rest) == 11 and rest[0] == 2 and rest[-1] == 0
    assert rest[1] is not None and rest[2:5] == (None,) * 3 and rest[5] is not None  # tq, (tl, tu, tPx), tAx
    assert {key: t[key].shape for key in t} == dict(x=(2, 3, N), y=(2, 3, M), act=(3, M), status=(3,))
    rb.lib.calls.clear()
    t = rb.jvp(l=np.ones((3, M)), rows=np.array(sel))  # one direction
    (name, k, got, rest), = rb.lib.calls
    assert rest[0] == 1 and t["x"].shape == (3, N) and t["y"].shape == (3, M)


def test_jvp_device_form():
    rb = _handle()
    out = dict(x=_Dev(2, 2, N), y=_Dev(2, 2, M), act=_Dev(2, M))
    assert rb.jvp(q=_Dev(2, 2, N), out=out, rows=[3, 6]) is out
    (name, k, got, rest), = rb.lib.calls
    assert name == "osqp_amd_batch_jvp_rows" and got == [3, 6] and rest[0] == 2 and rest[-1] == 1
    with pytest.raises(ValueError, match=r"out\['x'\]"):
        rb.jvp(q=_Dev(2, 2, N), out=dict(x=_Dev(2, COUNT, N), y=_Dev(2, 2, M)), rows=[3, 6])
    with pytest.raises(ValueError, match="all be host arrays or all device arrays"):
        rb.jvp(q=_Dev(2, 2, N), l=np.ones((2, 2, M)), out=out, rows=[3, 6])
    assert len(rb.lib.calls) == 1


def test_certificates_and_polish_status_hand_the_selection():
    rb = _handle()
    p, d = rb.certificates(rows=[2, 5])
    st = rb.polish_status(rows=[2, 5])
    assert p.shape == (2, M) and d.shape == (2, N) and st.shape == (2,) and st.dtype == np.int64
    (n1, k1, s1, r1), (n2, k2, s2, r2) = rb.lib.calls
    assert (n1, k1, s1) == ("osqp_amd_batch_certificates_rows", 2, [2, 5]) and len(r1) == 3 and r1[-1] == 0
    assert (n2, k2, s2) == ("osqp_amd_batch_polish_status_rows", 2, [2, 5]) and len(r2) == 2 and r2[-1] == 0
    rb.lib.calls.clear()
    out = (None, _Dev(2, N))
    assert rb.certificates(out=out, rows=[2, 5])[1] is out[1]
    sd = _Dev(2, 1)
    assert rb.polish_status(out=sd, rows=[2, 5]) is sd
    assert [c[0] for c in rb.lib.calls] == ["osqp_amd_batch_certificates_rows", "osqp_amd_batch_polish_status_rows"]
    assert rb.lib.calls[0][3] == (None, 4096, 1) and rb.lib.calls[1][3] == (4096, 1)
    with pytest.raises(ValueError, match=r"out\[1\]"):
        rb.certificates(out=(None, _Dev(COUNT, N)), rows=[2, 5])
    with pytest.raises(ValueError, match="out"):
        rb.polish_status(out=_Dev(COUNT, 1), rows=[2, 5])
    assert len(rb.lib.calls) == 2


def test_without_constraints_the_primal_certificate_is_none():
    rb = _handle()
    rb.m = rb.nnzA = 0
    p, d = rb.certificates(rows=[3, 1])
    assert p is None and d.shape == (2, N)
    assert rb.lib.calls[0][3][0] is None
    assert sorted(rb.adjoint(dx=np.ones((2, N)), rows=[3, 1])) == ["Px", "q", "status"]
    assert sorted(rb.jvp(q=np.ones((2, N)), rows=[3, 1])) == ["status", "x"]


def test_a_mask_selects_ascending():
    rb = _handle()
    mask = np.zeros(COUNT, dtype=bool)
    mask[[5, 1, 3]] = True
    rb.adjoint(dx=np.ones((3, N)), rows=mask)
    rb.jvp(q=np.ones((3, N)), rows=mask)
    rb.certificates(rows=mask)
    rb.polish_status(rows=mask)
    assert [c[2] for c in rb.lib.calls] == [[1, 3, 5]] * 4 and [c[1] for c in rb.lib.calls] == [3] * 4


def test_whole_batch_arrays_are_refused_with_a_selection():
    rb = _handle()
    with pytest.raises(ValueError, match="dx"):
        rb.adjoint(dx=np.ones((COUNT, N)), rows=[6, 0, 2])
    with pytest.raises(ValueError, match="dy"):
        rb.adjoint(dx=np.ones((3, N)), dy=np.ones((COUNT, M)), rows=[6, 0, 2])
    with pytest.raises(ValueError, match="q"):
        rb.jvp(q=np.ones((COUNT, N)), rows=[6, 0, 2])
    with pytest.raises(ValueError, match="Ax"):
        rb.jvp(q=np.ones((2, 3, N)), Ax=np.ones((2, COUNT, NNZA)), rows=[6, 0, 2])
    assert rb.lib.calls == []


@pytest.mark.parametrize("bad, word", [([1, 3, 1], "repeated"), ([0, -1], "out of range"), ([COUNT], "out of range"), ([], "empty"),
                                       (np.zeros(COUNT, dtype=bool), "empty"), (np.ones(COUNT + 1, dtype=bool), "length"),
                                       (list(range(COUNT)) + [0], "entries"), ([0.5], "integers"), ([[0, 1]], "one-dimensional")])
def test_a_bad_selection_is_refused_before_the_library_is_called(bad, word):
    rb = _handle()
    k = max(len(bad), 1)
    for call in (lambda: rb.adjoint(dx=np.ones((k, N)), rows=bad), lambda: rb.jvp(q=np.ones((k, N)), rows=bad),
                 lambda: rb.certificates(rows=bad), lambda: rb.polish_status(rows=bad)):
        with pytest.raises(ValueError, match=word):
            call()
    assert rb.lib.calls == []


def test_without_rows_the_whole_batch_entries_are_called():
    rb = _handle()
    g = rb.adjoint(dx=np.ones((COUNT, N)))
    t = rb.jvp(q=np.ones((2, COUNT, N)))
    p, d = rb.certificates()
    st = rb.polish_status()
    assert [c[0] for c in rb.lib.calls] == ["osqp_amd_batch_adjoint", "osqp_amd_batch_jvp", "osqp_amd_batch_certificates",
                                            "osqp_amd_batch_polish_status"]
    assert [len(c[3]) for c in rb.lib.calls] == [10, 11, 3, 2]
    assert g["q"].shape == (COUNT, N) and t["x"].shape == (2, COUNT, N) and p.shape == (COUNT, M) and st.shape == (COUNT,)


def test_the_layers_stamps_are_per_instance():
    """A forward stamps the instances it served; a backward may run while all of ITS instances still carry its stamp."""
    from osqp_jl_amd.qp_layer import stamp_forward, stamp_holds

    class Handle:
        count = 6

    rb = Handle()
    assert not stamp_holds(rb, 1, None)  # no forward yet
    a_sel, b_sel = np.array([5, 0]), np.array([2, 3])
    a = stamp_forward(rb, a_sel)
    b = stamp_forward(rb, b_sel)
    assert a != b and stamp_holds(rb, a, a_sel) and stamp_holds(rb, b, b_sel)  # disjoint: both backwards may run
    c = stamp_forward(rb, np.array([3, 4]))  # overlaps b
    assert stamp_holds(rb, a, a_sel) and not stamp_holds(rb, b, b_sel) and stamp_holds(rb, c, np.array([3, 4]))
    w = stamp_forward(rb, None)  # a whole forward invalidates everything before it
    assert not stamp_holds(rb, a, a_sel) and not stamp_holds(rb, c, np.array([3, 4])) and stamp_holds(rb, w, None)
    d = stamp_forward(rb, a_sel)
    assert not stamp_holds(rb, w, None) and stamp_holds(rb, d, a_sel) and stamp_holds(rb, w, b_sel)
