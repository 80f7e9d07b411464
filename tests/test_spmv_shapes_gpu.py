"""The sparse products A x, A' y, P x (op 0, 1, 2 of osqp_amd_apply) on ragged matrices at small panel widths, against the
exact host reference (spmv_reference.py) on the cases of spmv_cases.py: the CSR kernel k_spmv<G> at every lane width, the
LDS-staged sliced-ELL panels at 64 and 256 columns with 1-4 panels per group, the wide panels, value updates through
k_sell_scatter and through the slot maps of a compact workspace, Ruiz scaling through the slice visitors, the paired launch.

Every product assertion stands next to a layout assertion (osqp_amd_spmv_layout): the matrix ran on the kernel the case
names, with the panels, groups and reduction depth worked out from its shape -- no case can pass on another kernel.
Integer-valued cases are compared bit for bit, real-valued ones row by row against (L + NG + 2) 2^-53 sum |a||x|; there is
no normwise tolerance in this file.

OSQP_AMD_SPMV_RECORD=<file> (optional): the largest |err| / bound seen per kernel path is written there as JSON when the
module is done -- a record (profiles/spmv_shapes.json), nothing asserts on it."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_jl_amd as oq
import spmv_cases as sc
import spmv_reference as ref

pytestmark = pytest.mark.gpu
f = oq.interface._fptr

# read per setup (csrc/panel.hip, kernels.hip, engine.hip); cleared before every setup so that a run sets exactly its own
ENV = ("OSQP_AMD_PANEL", "OSQP_AMD_PANEL_SHIFT", "OSQP_AMD_PANEL_GROUP", "OSQP_AMD_PANEL_TILE_NNZ", "OSQP_AMD_WIDE_SHIFT",
       "OSQP_AMD_SPMV_G", "OSQP_AMD_COMPACT_NNZ")
_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    path = os.environ.get("OSQP_AMD_SPMV_RECORD")
    if path and _RATIOS:
        with open(path, "w") as fh:
            json.dump({"max_err_over_bound": {k: round(v, 4) for k, v in sorted(_RATIOS.items())},
                       "bound": "(L_i + NG + 2) * 2^-53 * sum_j |a_ij||x_j| per row (NG = 0 on the CSR kernel)"}, fh, indent=1)
            fh.write("\n")


def _env(monkeypatch, case, **env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**env, **case.env}.items():
        monkeypatch.setenv(k, str(v))


def _setup(lib, case, **settings):
    opts = dict(scaling=0, linsys_solver="pcg", verbose=False)
    opts.update(settings)
    m = oq.Model(lib)
    oq.setup(m, **case.problem(), **opts)
    assert oq.dimensions(m) == (case.n, case.m)
    return m


def _apply(lib, m, case, op, vec=None):
    vec = (case.y if op == 1 else case.x) if vec is None else vec
    out = np.full(case.m if op == 0 else case.n, np.nan)
    assert lib.osqp_amd_apply(m.workspace, op, f(vec), f(out)) == 0
    return out


def _layouts(m, case, mode, shift, group, wide_shift=None, compact=0, lanes=None):
    """The layout of A, A', P as the library reports it, asserted against what the settings imply for these shapes."""
    got = {}
    mats = case.matrices()
    for op in (0, 1, 2):
        M = mats[op][0]
        lay = oq.spmv_layout(m, op)
        want = sc.expected_layout(M.shape[1], mode, shift, group, wide_shift)
        what = (case.name, case.variant, "op", op, lay, want)
        assert lay["kernel"] == want["kernel"], what
        assert lay["nnz"] == M.nnz, what
        if lanes is not None:
            assert lay["G"] == lanes, what
        if want["kernel"]:
            assert all(lay[k] == want[k] for k in ("shift", "B", "Gp", "NG")), what
            assert lay["compact"] == compact, what
            st = sc.structure(M, lay["shift"])
            least = int(np.sum((st["rows_in_panel"] + 63) // 64))  # a slice is up to 64 non-empty rows of one tile inside one panel
            assert lay["tiles"] >= lay["NG"] and lay["slices"] >= least, what
            if lay["tiles"] == lay["NG"]:
                assert lay["slices"] == least, what
            assert lay["padded"] >= M.nnz and lay["padded"] % 64 == 0 and lay["padded"] <= 64 * int(st["cell"].max(initial=0)) * lay["slices"], what
        else:
            assert lay["tiles"] == lay["slices"] == lay["padded"] == lay["B"] == 0 and lay["compact"] == 0, what
        got[op] = lay
    return got


def _check(lib, m, case, prods, lays, path):
    for op in (0, 1, 2):
        out = _apply(lib, m, case, op)
        depth = lays[op]["NG"]
        if prods[op].exact_int is None:
            key = path if lays[op]["kernel"] else path + " (this matrix on CSR)"
            _RATIOS[key] = max(_RATIOS.get(key, 0.0), ref.error_ratio(out, prods[op], depth))
        ref.assert_product(out, prods[op], depth, (case.name, case.variant, path, "op", op, lays[op]))


_PRODUCTS = {}


def _products(case):
    key = (case.name, case.variant, case.n, case.notes.get("shift"))
    if key not in _PRODUCTS:
        _PRODUCTS[key] = case.products()
    return _PRODUCTS[key]


def _feature_asserts(case, lays):
    """The layout has the feature the case is there for."""
    if case.name == "many_short_rows":  # rows > 2 * 3968 and every row costs at least 1: the row cap cuts every group at least twice
        for op in (0, 1, 2):
            assert lays[op]["tiles"] >= 3 * lays[op]["NG"], lays[op]
    if case.name == "long_rows" and lays[0]["NG"] == 1:  # one group of every panel: more stored entries than one tile's budget
        assert lays[0]["tiles"] > lays[0]["NG"], lays[0]
    if case.name == "ragged" and case.n == 5000:
        assert lays[0]["B"] == 79 and lays[2]["B"] == 79
    if case.name == "flat":
        assert lays[0]["kernel"] == 2 and lays[1]["kernel"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# the three kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sc.VARIANTS)
@pytest.mark.parametrize("name,args,lanes", sc.CSR_RUNS, ids=[f"{n}-G{g}" for n, _, g in sc.CSR_RUNS])
def test_csr_kernel_at_every_lane_width(product_lib, monkeypatch, name, args, lanes, variant):
    """k_spmv<G> forced to G lanes per row on rows of length 0, 1, G-1, G, G+1, 4G-1, 4G, 4G+1, 8G+3 (the 4G unroll test, the
    tail loop, rows shorter than G) and on the ragged matrix."""
    case = sc.build(name, variant, **dict(args))
    _env(monkeypatch, case, OSQP_AMD_PANEL=0, OSQP_AMD_SPMV_G=lanes)
    m = _setup(product_lib, case)
    lays = _layouts(m, case, 0, 14, 1, lanes=lanes)
    _check(product_lib, m, case, _products(case), lays, "csr")
    oq.clean(m)


@pytest.mark.parametrize("variant", sc.VARIANTS)
@pytest.mark.parametrize("name,args,shift", sc.LDS_RUNS, ids=[f"{n}{dict(a).get('n', '')}-shift{s}" for n, a, s in sc.LDS_RUNS])
def test_lds_panels(product_lib, monkeypatch, name, args, shift, variant):
    """Sliced-ELL panels of 2^shift columns staged in LDS, 1-4 panels per group: every builder."""
    case = sc.build(name, variant, shift, **dict(args))
    prods = _products(case)
    for group in sc.GROUPS:
        _env(monkeypatch, case, OSQP_AMD_PANEL=2, OSQP_AMD_PANEL_SHIFT=shift, OSQP_AMD_PANEL_GROUP=group)
        m = _setup(product_lib, case)
        lays = _layouts(m, case, 2, shift, group)
        _feature_asserts(case, lays)
        _check(product_lib, m, case, prods, lays, "lds-panels")
        oq.clean(m)


@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_row_longer_than_a_whole_tile_budget(product_lib, monkeypatch, variant):
    """long_rows at n = 4400, 256-column panels, 16 panels per group: the row that holds every column has 4096 entries inside
    the first group, more than the 3968 a tile's budget can ever be under OSQP_AMD_PANEL_TILE_NNZ = 48 -- its cost spans two
    windows of the tile cut."""
    case = sc.long_rows(variant, n=sc.OVER_BUDGET_N)
    group = sc.OVER_BUDGET_GROUP
    st = sc.structure(case.A, 8)
    assert st["cell"][case.notes["dense"], :group].sum() > max(sc.LONG_ROWS_TILE_NNZ * group, sc.TILE_ROWS_MAX)
    _env(monkeypatch, case, OSQP_AMD_PANEL=2, OSQP_AMD_PANEL_SHIFT=8, OSQP_AMD_PANEL_GROUP=group)
    m = _setup(product_lib, case)
    lays = _layouts(m, case, 2, 8, group)
    assert (lays[0]["B"], lays[0]["Gp"], lays[0]["NG"]) == (18, 16, 2) and lays[0]["tiles"] > lays[0]["NG"], lays[0]
    _check(product_lib, m, case, _products(case), lays, "lds-panels")
    P2, A2 = _new_values(case, 9)
    oq.update(m, Px=P2.data, Ax=A2.data)
    _check(product_lib, m, case, case.products(P2, A2), _layouts(m, case, 2, 8, group), "lds-panels after a full update")
    oq.clean(m)


@pytest.mark.parametrize("variant", sc.VARIANTS)
@pytest.mark.parametrize("name,args,wshift", sc.WIDE_RUNS, ids=[f"{n}-wide{s}" for n, _, s in sc.WIDE_RUNS])
def test_wide_panels(product_lib, monkeypatch, name, args, wshift, variant):
    """The same tiles over wide panels gathered through L2 (32-bit local column ids), at 128 and 512 columns."""
    case = sc.build(name, variant, **dict(args))
    prods = _products(case)
    for group in (1, 3):
        _env(monkeypatch, case, OSQP_AMD_PANEL=3, OSQP_AMD_PANEL_SHIFT=sc.WIDE_PANEL_SHIFT, OSQP_AMD_WIDE_SHIFT=wshift,
             OSQP_AMD_PANEL_GROUP=group)
        m = _setup(product_lib, case)
        lays = _layouts(m, case, 3, sc.WIDE_PANEL_SHIFT, group, wide_shift=wshift)
        assert all(lays[op]["kernel"] == 3 for op in (0, 1, 2))
        _feature_asserts(case, lays)
        _check(product_lib, m, case, prods, lays, "wide-panels")
        oq.clean(m)


# ---------------------------------------------------------------------------------------------------------------------
# value updates
# ---------------------------------------------------------------------------------------------------------------------
def _new_values(case, seed):
    """New values for every stored entry of triu P and A: each entry times its own factor from {2, -3} (diagonal of P: 3, so
    it still dominates its row); integers stay integers."""
    rng = np.random.default_rng(seed)
    P = case.P.copy(); A = case.A.copy()
    fp = rng.choice(np.array([2.0, -3.0]), size=P.nnz)
    col = np.repeat(np.arange(P.shape[1]), np.diff(P.indptr))
    fp[P.indices == col] = 3.0
    P.data = P.data * fp
    A.data = A.data * rng.choice(np.array([2.0, -3.0]), size=A.nnz)
    return P, A


def _stratified(M_csc, rng, fraction=0.2):
    """nnz indices of a CSC matrix: a random fifth, plus one entry of every non-empty (64-row block, 64-column block) -- every
    panel of the matrix and of its transpose, at either width -- plus the first and last entry of every row longer than 64."""
    M = sp.csc_matrix(M_csc)
    col = np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))
    key = (M.indices >> 6).astype(np.int64) * (1 << 20) + (col >> 6)
    _, first = np.unique(key, return_index=True)
    pick = set(first.tolist()) | set(rng.choice(M.nnz, size=max(1, int(fraction * M.nnz)), replace=False).tolist())
    L = np.bincount(M.indices, minlength=M.shape[0])
    for i in np.nonzero(L > 64)[0]:
        at = np.nonzero(M.indices == i)[0]
        pick.update((int(at[0]), int(at[-1])))
    return np.array(sorted(pick), dtype=np.int64)


@pytest.mark.parametrize("variant", sc.VARIANTS)
@pytest.mark.parametrize("name", ["ragged", "long_rows"])
@pytest.mark.parametrize("shift", sc.LDS_SHIFTS)
def test_full_update_refreshes_the_slices(product_lib, monkeypatch, name, shift, variant):
    """A workspace that keeps its CSR arrays: osqp_update_P_A with every value rewrites the slices through k_sell_scatter
    (rows of 200+ consecutive columns: panel changes on and off the 64-entry chunk boundaries)."""
    case = sc.build(name, variant, shift)
    _env(monkeypatch, case, OSQP_AMD_PANEL=2, OSQP_AMD_PANEL_SHIFT=shift, OSQP_AMD_PANEL_GROUP=2)
    m = _setup(product_lib, case)
    lays = _layouts(m, case, 2, shift, 2)
    _check(product_lib, m, case, _products(case), lays, "lds-panels")
    for seed in (1, 2):
        P2, A2 = _new_values(case, seed)
        oq.update(m, Px=P2.data, Ax=A2.data)
        lays = _layouts(m, case, 2, shift, 2)
        _check(product_lib, m, case, case.products(P2, A2), lays, "lds-panels after a full update")
    oq.clean(m)


@pytest.mark.parametrize("variant", sc.VARIANTS)
@pytest.mark.parametrize("shift", sc.LDS_SHIFTS)
def test_compact_updates_in_full_and_by_index(product_lib, monkeypatch, shift, variant):
    """A compact workspace (m, n > W: all three matrices give up their CSR arrays): the products, then updates through the
    slot maps, in full and by index with every row class and every panel of A, A' and P hit."""
    case = sc.ragged(variant)
    _env(monkeypatch, case, OSQP_AMD_PANEL=2, OSQP_AMD_PANEL_SHIFT=shift, OSQP_AMD_PANEL_GROUP=3, OSQP_AMD_COMPACT_NNZ=0)
    m = _setup(product_lib, case)
    assert oq.stats(m)[18] == 1.0
    lays = _layouts(m, case, 2, shift, 3, compact=1)
    _check(product_lib, m, case, _products(case), lays, "lds-panels compact")
    P2, A2 = _new_values(case, 3)
    oq.update(m, Px=P2.data, Ax=A2.data)
    _check(product_lib, m, case, case.products(P2, A2), _layouts(m, case, 2, shift, 3, compact=1), "lds-panels compact after a full update")
    rng = np.random.default_rng(4)
    idxP, idxA = _stratified(case.P, rng), _stratified(case.A, rng)
    P3, A3 = _new_values(case, 5)
    P4, A4 = P2.copy(), A2.copy()
    P4.data[idxP] = P3.data[idxP]; A4.data[idxA] = A3.data[idxA]
    oq.update(m, Px=P4.data[idxP], Px_idx=idxP, Ax=A4.data[idxA], Ax_idx=idxA)
    _check(product_lib, m, case, case.products(P4, A4), _layouts(m, case, 2, shift, 3, compact=1), "lds-panels compact after an update by index")
    oq.update(m, Ax=A3.data[idxA[::2]], Ax_idx=idxA[::2])  # A alone, then P alone
    A4.data[idxA[::2]] = A3.data[idxA[::2]]
    oq.update(m, Px=P2.data[idxP[::3]], Px_idx=idxP[::3])
    P4.data[idxP[::3]] = P2.data[idxP[::3]]
    _check(product_lib, m, case, case.products(P4, A4), _layouts(m, case, 2, shift, 3, compact=1), "lds-panels compact after an update by index")
    oq.clean(m)


@pytest.mark.parametrize("shift", sc.LDS_SHIFTS)
def test_scaling_through_the_slice_visitors_is_the_csr_scaling(product_lib, monkeypatch, shift):
    """Ruiz scaling on a compact workspace walks the slices (k_sell_scale_norm, k_sell_visit), on one that keeps its CSR
    arrays the CSR kernels, and the slices are filled from the result: the same operations in the same order on every value
    (Engine::scale_data), the same layout -- the three products are bit-identical, after setup, after an update
    that passes the unchanged values (unscale, rescale), after one that changes some by index and after one that changes all."""
    case = sc.ragged("real")
    ms = {}
    for mode, limit in (("compact", 0), ("csr", -1)):
        _env(monkeypatch, case, OSQP_AMD_PANEL=2, OSQP_AMD_PANEL_SHIFT=shift, OSQP_AMD_PANEL_GROUP=2, OSQP_AMD_COMPACT_NNZ=limit)
        ms[mode] = _setup(product_lib, case, scaling=10)
        assert oq.stats(ms[mode])[18] == float(mode == "compact")
    lays = {mode: _layouts(ms[mode], case, 2, shift, 2, compact=int(mode == "compact")) for mode in ms}
    for op in (0, 1, 2):
        a, b = lays["compact"][op], lays["csr"][op]
        assert {k: v for k, v in a.items() if k != "compact"} == {k: v for k, v in b.items() if k != "compact"}

    def same(stage):
        for op in (0, 1, 2):
            a, b = (_apply(product_lib, ms[mode], case, op) for mode in ("compact", "csr"))
            bad = np.nonzero(a != b)[0]
            assert np.array_equal(a, b), (stage, "op", op, "rows", bad[:8], a[bad[:8]], b[bad[:8]])

    same("after setup")
    for m in ms.values():
        oq.update(m, Px=case.P.data, Ax=case.A.data)
    same("after an update with the unchanged values")
    P2, A2 = _new_values(case, 6)
    rng = np.random.default_rng(7)
    idxP, idxA = _stratified(case.P, rng), _stratified(case.A, rng)
    for m in ms.values():
        oq.update(m, Px=P2.data[idxP], Px_idx=idxP, Ax=A2.data[idxA], Ax_idx=idxA)
    same("after an update by index")
    for m in ms.values():
        oq.update(m, Px=P2.data, Ax=A2.data)
    same("after a full update")
    for m in ms.values():
        oq.clean(m)


# ---------------------------------------------------------------------------------------------------------------------
# the paired launch, and the sort key of the per-tile ordering
# ---------------------------------------------------------------------------------------------------------------------
def _iterate(lib, m, iters):
    assert lib.osqp_amd_iterate(m.workspace, iters) == 0
    n, mm = oq.dimensions(m)
    x, y = np.full(n, np.nan), np.full(mm, np.nan)
    assert lib.osqp_amd_get_iterate(m.workspace, f(x), f(y)) == 0
    return x, y


def test_pair_launch_small_panels_then_default_width(product_lib, monkeypatch):
    """A p and P p of a CG iteration go out as one launch when both matrices run on LDS panels of one width (spmv_pair).
    Five ADMM iterations on 256-column panels against the same on the CSR kernel; then, in the same process, the generated
    n = 40000 problem at the default width of 16384 columns -- the launch needs 159 KB of dynamic LDS there, after a first
    pair launch that needed 33 KB."""
    case = sc.many_short_rows("int")
    its = {}
    for mode in (2, 0):
        _env(monkeypatch, case, OSQP_AMD_PANEL=mode, OSQP_AMD_PANEL_SHIFT=8, OSQP_AMD_PANEL_GROUP=1)
        m = _setup(product_lib, case, scaling=10)
        lays = _layouts(m, case, mode, 8, 1)
        assert lays[0]["kernel"] == lays[2]["kernel"] == mode and lays[0]["tiles"] + lays[2]["tiles"] <= 2048  # the pair's conditions
        its[mode] = _iterate(product_lib, m, 5)
        oq.clean(m)
    for a, b in zip(its[2], its[0]):
        assert np.all(np.isfinite(a)) and np.max(np.abs(a - b)) <= 1e-9
    big = {}
    for mode in (2, 0):
        for k in ENV:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("OSQP_AMD_PANEL", str(mode))
        m = oq.Model(product_lib)
        oq.setup_generated(m, 0, 40000, 96, 21, verbose=False, linsys_solver="pcg")
        for op in (0, 1, 2):
            lay = oq.spmv_layout(m, op)
            assert lay["kernel"] == mode and (mode == 0 or (lay["shift"], lay["B"]) == (14, 3)), lay
        big[mode] = _iterate(product_lib, m, 5)
        oq.clean(m)
    for a, b in zip(big[2], big[0]):
        assert np.all(np.isfinite(a)) and np.max(np.abs(a - b)) <= 1e-9


def test_budget_row_over_a_wide_panel_stays_on_csr(product_lib, monkeypatch):
    """A = [ones(1, n); I_n], n = 600000, one wide panel of 2^20 columns: the budget row has more entries inside the panel
    than the 32-bit sort key of the per-tile ordering holds (2^19 - 1), so the layout is declined before anything is sized
    from the key and A stays on the CSR kernel; A' (two entries per row) and P run on the wide panels.  All exact."""
    n = 600000
    rng = np.random.default_rng(8)
    vals = lambda k: rng.choice(np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0]), size=k)
    A = sp.vstack([sp.csr_matrix(vals(n).reshape(1, n)), sp.diags(vals(n))]).tocsc()
    A.sort_indices()
    P = sp.diags(rng.integers(1, 4, size=n).astype(np.float64)).tocsc()
    x = rng.integers(-4, 5, size=n).astype(np.float64); y = rng.integers(-4, 5, size=n + 1).astype(np.float64)
    case = sc.Case("budget_row", "int", P, np.zeros(n), A, -np.ones(n + 1), np.ones(n + 1), x, y)
    _env(monkeypatch, case, OSQP_AMD_PANEL=3, OSQP_AMD_WIDE_SHIFT=20)
    m = _setup(product_lib, case)
    lays = {op: oq.spmv_layout(m, op) for op in (0, 1, 2)}
    assert lays[0]["kernel"] == 0 and lays[0]["nnz"] == 2 * n, lays[0]
    for op in (1, 2):
        assert (lays[op]["kernel"], lays[op]["shift"], lays[op]["B"], lays[op]["NG"]) == (3, 20, 1, 1), lays[op]
        assert lays[op]["tiles"] >= n // sc.TILE_ROWS_MAX
    prods = case.products()
    assert all(p.exact_int is not None for p in prods.values())
    _check(product_lib, m, case, prods, lays, "wide-panels")
    oq.clean(m)
