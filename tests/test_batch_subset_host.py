"""The host side of the subset calls of the resident batch (`rows=` of batch.ResidentBatch.update / warm_start / solve): the
selection helper that runs before the library is called, and the declarations of the five new entry points.  No GPU."""
import numpy as np
import pytest

from osqp_jl_amd import batch
from osqp_jl_amd import types as T

ROWS_SYMBOLS = {
    "osqp_amd_batch_update_lin_cost_rows": 5,
    "osqp_amd_batch_update_bounds_rows": 6,
    "osqp_amd_batch_update_matrices_rows": 6,
    "osqp_amd_batch_warm_start_rows": 6,
    "osqp_amd_batch_resolve_rows": 7,
}


def test_selection_keeps_the_order_and_converts():
    got = batch.selection([5, 0, 3], 8)
    assert got.dtype == np.int64 and got.flags["C_CONTIGUOUS"] and got.tolist() == [5, 0, 3]
    assert batch.selection(np.array([7, 2], dtype=np.int32), 8).tolist() == [7, 2]
    assert batch.selection(np.array([1, 6], dtype=np.uint8), 8).tolist() == [1, 6]
    assert batch.selection((4,), 8).tolist() == [4]
    assert batch.selection(np.arange(8)[::-1], 8).tolist() == list(range(7, -1, -1))  # a strided view, every instance
    assert batch.selection(range(3), 3).tolist() == [0, 1, 2]


def test_selection_takes_a_mask():
    mask = np.array([False, True, False, True, True])
    assert batch.selection(mask, 5).tolist() == [1, 3, 4]
    assert batch.selection([True, False], 2).tolist() == [0]
    assert batch.selection(np.ones(4, dtype=bool), 4).tolist() == [0, 1, 2, 3]
    status = np.array([1, -2, 1, -2])
    assert batch.selection(np.flatnonzero(status != 1), 4).tolist() == [1, 3]  # the selection of a retry


@pytest.mark.parametrize("rows, count, word", [
    ([1, 3, 1], 5, "repeated"),
    ([-1], 5, "out of range"),
    ([5], 5, "out of range"),
    ([0, 7, 2], 5, "out of range"),
    ([], 5, "empty"),
    (np.zeros(0, dtype=np.int64), 5, "empty"),
    (np.zeros(5, dtype=bool), 5, "empty"),
    (np.ones(4, dtype=bool), 5, "length 5"),
    (np.ones(6, dtype=bool), 5, "length 5"),
    ([0, 1, 2, 3, 4, 0], 5, "6 entries"),
    ([0.0, 1.0], 5, "integers"),
    (np.array([0.5]), 5, "integers"),
    (["a"], 5, "integers"),
    ([None], 5, "integers"),
    ([[0, 1]], 5, "one-dimensional"),
    (3, 5, "one-dimensional"),
    (np.array([2 ** 63], dtype=np.uint64), 5, "out of range"),
])
def test_selection_refuses(rows, count, word):
    with pytest.raises(ValueError, match=word):
        batch.selection(rows, count)


def test_selection_names_the_repeated_instance():
    with pytest.raises(ValueError, match="instance 4 is repeated"):
        batch.selection([0, 4, 2, 4], 6)
    with pytest.raises(ValueError, match="instance -3 is out of range"):
        batch.selection([1, -3], 6)


def test_the_five_entries_are_declared():
    """types.py declares them with rows (an integer pointer) and k after the handle; tests/test_abi_exports.py holds the
    library to whatever the header declares."""
    for name, nargs in ROWS_SYMBOLS.items():
        assert name in T.EXT_SYMBOLS, name
        restype, argtypes = T.EXT_SYMBOLS[name]
        assert restype is T.c_int and len(argtypes) == nargs, (name, argtypes)
        assert argtypes[1] is T.c_int_p and argtypes[2] is T.c_int and argtypes[-1] is T.c_int, (name, argtypes)
        whole = T.EXT_SYMBOLS[name[: -len("_rows")]][1]
        assert argtypes[:1] + argtypes[3:] == whole, (name, argtypes, whole)  # the whole-batch signature with rows, k inserted


def test_the_header_declares_them():
    import os

    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "osqp_amd.h")).read()
    for name in ROWS_SYMBOLS:
        assert f"c_int {name}(osqp_amd_batch *batch, const c_int *rows, c_int k," in header, name
