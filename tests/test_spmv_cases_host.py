"""Host checks of the sparse-product test material (spmv_cases.py, spmv_reference.py): the exact reference against rational
arithmetic, the check against deliberate mutations, and every case against the structure its name claims at the panel
widths the GPU test (test_spmv_shapes_gpu.py) runs it at.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import spmv_cases as sc
import spmv_reference as ref


def _all_cases():
    seen = set()
    for name, args, shift in sc.LDS_RUNS:
        for variant in sc.VARIANTS:
            key = (name, args, shift if name == "slice_edges" else None, variant)
            if key not in seen:
                seen.add(key)
                yield pytest.param(name, args, shift, variant, id=f"{name}{dict(args) or ''}-{shift if key[2] else 'any'}-{variant}")


ALL = list(_all_cases())


def test_reference_is_the_rational_row_sum_rounded_once():
    """On small instances (rows of wildly different scale, cancellation, stored zeros) exact_i is the Fraction row sum
    rounded once and S_i the Fraction sum of |a||x|, to a rounding."""
    case = sc.slice_edges("real", 6)
    for op, (M, v) in case.matrices().items():
        prod = ref.reference(M, v)
        sums, sabs = ref.reference_fraction(M, v)
        assert [float(s) for s in sums] == prod.exact.tolist()
        assert [float(s) for s in sabs] == prod.S.tolist()
        assert prod.L.tolist() == np.diff(sp.csr_matrix(M).indptr).tolist()
    # cancellation: the row sum is far below its terms, and the error terms of the products decide its value
    a = np.array([[1e16 + 2.0, -1e16, 3.0, 0.1]])
    x = np.array([1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, 1.0 / 3.0, 0.1])
    prod = ref.reference(sp.csr_matrix(a), x)
    want = sum(Fraction(float(a[0, j])) * Fraction(float(x[j])) for j in range(4))
    assert prod.exact[0] == float(want) and prod.exact_int is None
    # the integer path is the same number
    ci = sc.slice_edges("int", 6)
    for op, (M, v) in ci.matrices().items():
        prod = ref.reference(M, v)
        sums, _ = ref.reference_fraction(M, v)
        assert prod.exact_int is not None and [int(s) for s in sums] == prod.exact_int.tolist()


@pytest.mark.parametrize("name,args,shift,variant", ALL)
def test_plain_float64_product_passes(name, args, shift, variant):
    """scipy's float64 product is one order of summation among the admissible ones: it must pass, with no depth allowance."""
    case = sc.build(name, variant, shift, **dict(args))
    prods = case.products()
    for op, (M, v) in case.matrices().items():
        ref.assert_product(M @ v, prods[op], 0, (name, variant, op))
        assert (prods[op].exact_int is not None) == (variant == "int")


@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_check_catches_one_entry(variant):
    """The three mutations: one entry of the smallest-scale row left out, one entry counted twice, 1e-300 in an empty row."""
    case = sc.ragged(variant)
    M, v = case.matrices()[0]
    prod = case.products()[0]
    good = M @ v
    ref.assert_product(good, prod)
    scale = np.where(prod.L > 0, prod.S, np.inf)
    i = int(np.argmin(np.where(scale > 0, scale, np.inf)))  # the row a normwise tolerance would never see
    assert prod.S[i] <= 1e-3 * prod.S.max() or variant == "int"
    terms = M.data[M.indptr[i]:M.indptr[i + 1]] * v[M.indices[M.indptr[i]:M.indptr[i + 1]]]
    t = terms[np.argmax(np.abs(terms))]
    assert t != 0.0
    for mutated in (good[i] - t, good[i] + t):
        out = good.copy(); out[i] = mutated
        with pytest.raises(AssertionError):
            ref.assert_product(out, prod)
    e = case.notes["empty"][0]
    assert prod.L[e] == 0
    for junk in (1e-300, -0.0):
        out = good.copy(); out[e] = junk
        with pytest.raises(AssertionError):
            ref.assert_product(out, prod)
    if variant == "real":  # what the old normwise check (1e-12 of the largest row) lets through
        out = good.copy(); out[i] = good[i] - t
        assert np.max(np.abs(out - good)) <= 1e-12 * np.max(np.abs(good))


# ---------------------------------------------------------------------------------------------------------------------
# structure
# ---------------------------------------------------------------------------------------------------------------------
def _widths(name):
    return sc.LDS_SHIFTS + (sc.WIDE_SHIFTS if name in ("ragged", "many_short_rows") else ())


@pytest.mark.parametrize("variant", sc.VARIANTS)
@pytest.mark.parametrize("n", [1000, 5000])
def test_ragged_structure(variant, n):
    case = sc.ragged(variant, n=n)
    assert case.A.shape == (1500, n)
    A = sp.csr_matrix(case.A)
    L = np.diff(A.indptr)
    assert np.sum(L == 0) == 150 and np.sum(L == 1) > 300 and np.sum(L == 2) > 300 and np.sum(L > 64) >= 5
    assert L.max() == n - 256 == L[case.notes["dense"]]  # every column the matrix uses
    assert np.sum(case.A.data == 0) == 12 and case.A.nnz < 2e5 and case.Pfull.nnz < 2e5
    if variant == "real":
        rowmax = np.array([np.abs(A.data[A.indptr[i]:A.indptr[i + 1]]).max() for i in range(A.shape[0]) if L[i]])
        assert rowmax.max() / rowmax.min() > 1e10
    for shift in _widths("ragged") if n == 1000 else (6,):
        st = sc.structure(A, shift)
        W = 1 << shift
        assert st["empty_rows"] == 150 and st["empty_cells"] > st["B"] * 150
        lo, hi = sc.EMPTY_BLOCK
        want_empty = [b for b in range(st["B"]) if lo <= b * W and (b + 1) * W <= hi]
        assert st["empty_panels"] == want_empty and (want_empty or shift > 8)
        assert st["width"][-1] < W  # the last panel is partial
        cell = st["cell"]
        only_first = [i for i in case.notes["first_only"] if cell[i, 0] == L[i]]
        only_last = [i for i in case.notes["last_only"] if cell[i, -1] == L[i]]
        assert len(only_first) == 30 and len(only_last) == 30
        if shift in (6, 8):  # a row dense in exactly one panel: as many entries as the panel has columns, none elsewhere
            dense_one = [i for i in case.notes["dense_in_one"] if np.sum(cell[i] > 0) == 1 and cell[i].max() == st["width"][np.argmax(cell[i])]]
            assert dense_one, shift
    if n == 5000:
        assert sc.structure(A, 6)["B"] == 79  # more panels than a wavefront has lanes: the strided loop of k_panel_count
    # A' has empty rows too (the columns of the empty block) and P none
    assert sc.structure(case.A.T, 6)["empty_rows"] == 256 and sc.structure(case.Pfull, 6)["empty_rows"] == 0


@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_many_short_rows_structure(variant):
    case = sc.many_short_rows(variant)
    assert case.A.shape == (9000, 8200)
    L = np.diff(sp.csr_matrix(case.A).indptr)
    assert set(L.tolist()) == {0, 1, 2}
    # every (group, row) cell costs at least 1 of a budget that gives a tile at most TILE_ROWS_MAX rows: three tiles per group
    assert min(case.m, case.n) > 2 * sc.TILE_ROWS_MAX
    for shift in _widths("many_short_rows"):
        st = sc.structure(case.A, shift)
        assert st["empty_cells"] > 0.99 * st["cell"].size - case.A.nnz
    assert sc.structure(case.A, 6)["B"] == 129 and sc.structure(case.A, 8)["B"] == 33


@pytest.mark.parametrize("variant", sc.VARIANTS)
@pytest.mark.parametrize("shift", sc.LDS_SHIFTS)
def test_slice_edges_structure(variant, shift):
    case = sc.slice_edges(variant, shift)
    st = sc.structure(case.A, shift)
    assert st["B"] == 4 and tuple(st["rows_in_panel"].tolist()) == sc.SLICE_EDGE_COUNTS == (1, 63, 64, 65)


@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_long_rows_structure(variant):
    case = sc.long_rows(variant)
    A = sp.csr_matrix(case.A)
    assert int(case.env["OSQP_AMD_PANEL_TILE_NNZ"]) == sc.LONG_ROWS_TILE_NNZ
    aligned = 0
    for i, (c0, k) in case.notes["runs"].items():
        cols = A.indices[A.indptr[i]:A.indptr[i + 1]]
        assert k >= 200 and np.array_equal(cols, np.arange(c0, c0 + k))
        for shift in sc.LDS_SHIFTS:
            st = sc.structure(A, shift)
            for g in sc.GROUPS:  # more entries inside one group than the tile budget asked for
                B, W = st["B"], 1 << shift
                per_group = [st["cell"][i, b0:b0 + g].sum() for b0 in range(0, B, g)]
                assert max(per_group) > sc.LONG_ROWS_TILE_NNZ
            changes = [c - c0 for c in range(c0 + 1, c0 + k) if c % W == 0]  # entry numbers at which the panel changes
            aligned += any(p % 64 == 0 for p in changes)
    assert aligned >= 4  # at both widths some run changes panel exactly on a chunk boundary of the value refresh ...
    c0, k = sc.LONG_RUNS[3]
    assert all((c - c0) % 64 for c in range(c0 + 1, c0 + k) if c % 64 == 0)  # ... and one never does
    assert np.diff(A.indptr)[case.notes["dense"]] == case.n
    assert A.nnz > sc.TILE_ROWS_MAX  # one group holding every panel is cut into two tiles by the non-zero budget


@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_flat_structure(variant):
    case = sc.flat(variant)
    for shift in sc.LDS_SHIFTS:
        assert case.m == 40 <= (1 << shift) < case.n
        assert sc.expected_layout(case.n, 2, shift, 1)["kernel"] == 2 and sc.expected_layout(case.m, 2, shift, 1)["kernel"] == 0
    L = np.diff(sp.csr_matrix(case.A).indptr)
    assert L.min() == 0 and L.max() == case.n


@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_unroll_edges_structure(variant):
    case = sc.unroll_edges(variant)
    L = np.diff(sp.csr_matrix(case.A).indptr).tolist()
    assert L == case.notes["lengths"]
    for G in sc.CSR_LANES:
        for k in (0, 1, G - 1, G, G + 1, 4 * G - 1, 4 * G, 4 * G + 1, 8 * G + 3):
            assert L.count(k) >= 3, (G, k)


def test_runs_cover_the_layout_edges():
    """Across the LDS-panel runs: B not divisible by Gp (a short last group) for every Gp > 1, B > 64, and reduction depths
    NG = 1, 3, 4, 5, 8, 9, 13 (the 8-wide, 4-wide and tail loops of panel_reduce_rows, alone and combined)."""
    depths, short_last, big_B = set(), set(), False
    for name, args, shift in sc.LDS_RUNS:
        case = sc.build(name, "int", shift, **dict(args))
        for cols in (case.n, case.m):
            for g in sc.GROUPS:
                lay = sc.expected_layout(cols, 2, shift, g)
                if lay["kernel"] == 2:
                    depths.add(lay["NG"])
                    if lay["B"] % lay["Gp"]:
                        short_last.add(lay["Gp"])
                    big_B = big_B or lay["B"] > 64
    assert {1, 3, 4, 5, 8, 9, 13} <= depths, sorted(depths)
    assert short_last == {2, 3, 4} and big_B


def test_over_budget_row_structure():
    """At n = 4400 the row holding every column has 4096 entries inside the first group of 16 panels of 256 columns: more than
    a tile's budget max(48 * 16, 3968) under the case's OSQP_AMD_PANEL_TILE_NNZ."""
    case = sc.long_rows("int", n=sc.OVER_BUDGET_N)
    st = sc.structure(case.A, 8)
    lay = sc.expected_layout(case.n, 2, 8, sc.OVER_BUDGET_GROUP)
    assert (lay["B"], lay["Gp"], lay["NG"]) == (18, 16, 2)
    assert st["cell"][case.notes["dense"], :16].sum() == 4096 > max(sc.LONG_ROWS_TILE_NNZ * 16, sc.TILE_ROWS_MAX)
    assert case.A.nnz < 2e5
