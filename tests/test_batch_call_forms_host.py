"""Which library entry `batch.ResidentBatch` calls for every instance and for a selection (`rows=`), with which arguments
and in which order: update, warm_start, solve, polish_status, certificates, duality, gap_refusals.  No library is loaded:
the handle is made with `object.__new__` and its `lib` is a stub that records (symbol, args).  No GPU."""
import numpy as np
import pytest

from osqp_jl_amd import batch
from osqp_jl_amd.interface import OSQPError

COUNT, N, M, NNZP, NNZA = 4, 3, 2, 5, 4
ROWS = [2, 0]
HANDLE = "the handle"


class StubLib:
    """Every osqp_amd_batch_* symbol records its call and returns `rc`."""

    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def osqp_amd_last_error(self):
        return b"refused by the stub"

    def __getattr__(self, name):
        if not name.startswith("osqp_amd_batch_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return self.rc

        return call


class Dev:
    """What `_batch_array` takes for a device array: a shape and an address."""
    dtype = "float64"

    def __init__(self, *shape):
        self.shape = shape
        self.address = 4096 * (1 + sum(shape)) + len(shape)

    def data_ptr(self):
        return self.address


def _handle(rc=0):
    rb = object.__new__(batch.ResidentBatch)
    rb.lib, rb.handle, rb.device = StubLib(rc), HANDLE, 0
    rb.count, rb.n, rb.m, rb.nnzP, rb.nnzA = COUNT, N, M, NNZP, NNZA
    return rb


def _host(k):
    return dict(q=np.ones((k, N)), l=-np.ones((k, M)), u=np.ones((k, M)), Px=np.ones((k, NNZP)), Ax=np.ones((k, NNZA)),
                x=np.zeros((k, N)), y=np.zeros((k, M)))


def _split(call, rows):
    """(base symbol, arguments after the handle and the selection) of a recorded call; checks the handle and the selection."""
    name, args = call
    assert args[0] == HANDLE
    if rows is None:
        assert not name.endswith("_rows")
        return name, args[1:]
    assert name.endswith("_rows") and args[2] == len(rows)
    assert np.ctypeslib.as_array(args[1], shape=(len(rows),)).tolist() == list(rows)
    return name[:-len("_rows")], args[3:]


@pytest.mark.parametrize("rows", [None, ROWS])
def test_update_issues_lin_cost_bounds_matrices_in_that_order(rows):
    rb, k = _handle(), COUNT if rows is None else len(rows)
    a = _host(k)
    rb.update(q=a["q"], l=a["l"], u=a["u"], Px=a["Px"], Ax=a["Ax"], rows=rows)
    got = [_split(c, rows) for c in rb.lib.calls]
    assert got == [("osqp_amd_batch_update_lin_cost", (a["q"].ctypes.data, 0)),
                   ("osqp_amd_batch_update_bounds", (a["l"].ctypes.data, a["u"].ctypes.data, 0)),
                   ("osqp_amd_batch_update_matrices", (a["Px"].ctypes.data, a["Ax"].ctypes.data, 0))]


@pytest.mark.parametrize("rows", [None, ROWS])
def test_update_passes_a_missing_array_as_null_and_device_arrays_by_address(rows):
    rb, k = _handle(), COUNT if rows is None else len(rows)
    u, Ax = Dev(k, M), Dev(k, NNZA)
    rb.update(u=u, Ax=Ax, rows=rows)
    got = [_split(c, rows) for c in rb.lib.calls]
    assert got == [("osqp_amd_batch_update_bounds", (None, u.address, 1)), ("osqp_amd_batch_update_matrices", (None, Ax.address, 1))]


@pytest.mark.parametrize("rows", [None, ROWS])
def test_warm_start(rows):
    rb, k = _handle(), COUNT if rows is None else len(rows)
    a = _host(k)
    rb.warm_start(x=a["x"], y=a["y"], rows=rows)
    rb.warm_start(y=Dev(k, M), rows=rows)
    got = [_split(c, rows) for c in rb.lib.calls]
    assert got == [("osqp_amd_batch_warm_start", (a["x"].ctypes.data, a["y"].ctypes.data, 0)),
                   ("osqp_amd_batch_warm_start", (None, Dev(k, M).address, 1))]


@pytest.mark.parametrize("rows", [None, ROWS])
def test_a_call_with_nothing_to_do_calls_nothing(rows):
    rb = _handle()
    rb.update(rows=rows)
    rb.warm_start(rows=rows)
    assert rb.lib.calls == []


@pytest.mark.parametrize("rows", [None, ROWS])
def test_solve(rows):
    rb, k = _handle(), COUNT if rows is None else len(rows)
    x, y, info = rb.solve(rows=rows)
    assert x.shape == (k, N) and y.shape == (k, M) and info.shape == (k, 6)
    out = (Dev(k, N), Dev(k, M), Dev(k, 6))
    assert rb.solve(out=out, rows=rows) is out
    got = [_split(c, rows) for c in rb.lib.calls]
    assert got == [("osqp_amd_batch_resolve", (x.ctypes.data, y.ctypes.data, info.ctypes.data, 0)),
                   ("osqp_amd_batch_resolve", (out[0].address, out[1].address, out[2].address, 1))]


@pytest.mark.parametrize("rows", [None, ROWS])
def test_certificates(rows):
    rb, k = _handle(), COUNT if rows is None else len(rows)
    p, d = rb.certificates(rows=rows)
    assert p.shape == (k, M) and d.shape == (k, N)
    out = (None, Dev(k, N))
    assert rb.certificates(out=out, rows=rows) == out
    got = [_split(c, rows) for c in rb.lib.calls]
    assert got == [("osqp_amd_batch_certificates", (p.ctypes.data, d.ctypes.data, 0)),
                   ("osqp_amd_batch_certificates", (None, out[1].address, 1))]


@pytest.mark.parametrize("rows", [None, ROWS])
@pytest.mark.parametrize("method, symbol, host_shape, device_shape", [
    ("polish_status", "osqp_amd_batch_polish_status", (), (1,)),
    ("duality", "osqp_amd_batch_duality", (3,), (3,)),
    ("gap_refusals", "osqp_amd_batch_gap_refusals", (), ()),
])
def test_one_output_is_a_numpy_result_or_a_device_array_filled_in_place(rows, method, symbol, host_shape, device_shape):
    rb, k = _handle(), COUNT if rows is None else len(rows)
    res = getattr(rb, method)(rows=rows)
    assert isinstance(res, np.ndarray) and res.shape == (k,) + host_shape
    assert res.dtype == (np.int64 if method == "polish_status" else np.float64)
    out = Dev(*((k,) + device_shape))
    assert getattr(rb, method)(out=out, rows=rows) is out
    got = [_split(c, rows) for c in rb.lib.calls]
    assert [g[0] for g in got] == [symbol, symbol]
    assert isinstance(got[0][1][0], int) and got[0][1][1:] == (0,) and got[1][1] == (out.address, 1)
    with pytest.raises(ValueError, match="expected a device array"):
        getattr(rb, method)(out=np.zeros((k,) + device_shape), rows=rows)
    with pytest.raises(ValueError, match="expected shape"):
        getattr(rb, method)(out=Dev(k + 1, *device_shape), rows=rows)
    assert len(rb.lib.calls) == 2


@pytest.mark.parametrize("rows", [None, ROWS])
@pytest.mark.parametrize("method, word", [
    ("update", "update"), ("warm_start", "warm start"), ("solve", "solve"), ("polish_status", "polish status"),
    ("certificates", "certificates"), ("duality", "duality"), ("gap_refusals", "gap_refusals"),
])
def test_a_refusal_raises_with_the_word_of_the_method(rows, method, word):
    rb, k = _handle(rc=1), COUNT if rows is None else len(rows)
    a = _host(k)
    kw = dict(update=dict(q=a["q"]), warm_start=dict(x=a["x"])).get(method, {})
    with pytest.raises(OSQPError) as err:
        getattr(rb, method)(rows=rows, **kw)
    assert str(err.value) == f"Error in batched {word}: refused by the stub"
    assert len(rb.lib.calls) == 1  # nothing is issued after a refusal
