"""The 2-byte per-lane slice table of the panel product and its non-temporal matrix loads (csrc/panel.hip), on the cases of
spmv_stream_cases.py against the exact host reference (spmv_reference.py): rows 0 .. 39 entries short of their slice, slices
ending on, past and short of a full batch, a slice of a single lane, local row 3967 (the largest table entry) next to empty
lanes, the wide mode, a value refresh, and OSQP_AMD_SELL_NT off against on, bit for bit.

Integer-valued variants are compared with array_equal, real-valued ones row by row against (L + NG + 2) 2^-53 sum |a||x|
(spmv_reference.assert_product); the on / off comparison is array_equal on real-valued data.  Every product assertion
stands next to a layout assertion: the matrix ran on the kernel and with the slices the case is there for."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # run as the child of the on / off test: no conftest has put the package on the path
    sys.path.insert(0, ROOT)

import osqp_jl_amd as oq
import spmv_cases as sc
import spmv_reference as ref
import spmv_stream_cases as ssc

pytestmark = pytest.mark.gpu
f = oq.interface._fptr
HERE = os.path.dirname(os.path.abspath(__file__))

ENV = ("OSQP_AMD_PANEL", "OSQP_AMD_PANEL_SHIFT", "OSQP_AMD_PANEL_GROUP", "OSQP_AMD_PANEL_TILE_NNZ", "OSQP_AMD_WIDE_SHIFT",
       "OSQP_AMD_SPMV_G", "OSQP_AMD_COMPACT_NNZ")
# read once per process by panel.hip (default on): the switches of the streaming path that this build has
SWITCHES = ("OSQP_AMD_SELL_NT",)


def _env(monkeypatch, case, **env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**env, **case.env}.items():
        monkeypatch.setenv(k, str(v))


def _setup(lib, case):
    m = oq.Model(lib)
    oq.setup(m, **case.problem(), scaling=0, linsys_solver="pcg", verbose=False)
    assert oq.dimensions(m) == (case.n, case.m)
    return m


def _apply(lib, m, case, op):
    vec = case.y if op == 1 else case.x
    out = np.full(case.m if op == 0 else case.n, np.nan)
    assert lib.osqp_amd_apply(m.workspace, op, f(vec), f(out)) == 0
    return out


def _layouts(m, case, mode, shift, group, wide_shift=None):
    lays = {}
    for op, (M, _) in case.matrices().items():
        lay = oq.spmv_layout(m, op)
        want = sc.expected_layout(M.shape[1], mode, shift, group, wide_shift)
        assert lay["kernel"] == want["kernel"] == mode and lay["nnz"] == M.nnz, (case.name, op, lay, want)
        assert all(lay[k] == want[k] for k in ("shift", "B", "Gp", "NG")), (case.name, op, lay, want)
        lays[op] = lay
    return lays


def _check(lib, m, case, prods, lays, what):
    for op in (0, 1, 2):
        ref.assert_product(_apply(lib, m, case, op), prods[op], lays[op]["NG"], (case.name, case.variant, what, "op", op, lays[op]))


def _one_tile_per_group(lay, M, shift):
    """The matrix is one tile per group, so its slices are those spmv_stream_cases.slices_of works out."""
    s = ssc.slices_of(M, shift)
    assert lay["tiles"] == lay["NG"] and lay["slices"] == sum(len(v) for v in s.values()) and lay["padded"] == ssc.padded_of(s), lay


_PRODUCTS = {}


def _products(case):
    key = (case.name, case.variant)
    if key not in _PRODUCTS:
        _PRODUCTS[key] = case.products()
    return _PRODUCTS[key]


@pytest.mark.parametrize("group", ssc.GROUPS)
@pytest.mark.parametrize("variant", sc.VARIANTS)
@pytest.mark.parametrize("name", ["ladder", "lone_row"])
def test_short_rows_and_a_lone_row_on_lds_panels(product_lib, monkeypatch, name, variant, group):
    """ladder: rows 0 .. 39 short of a slice of length 40, a slice of 17s, a slice of 16, ..., 15; lone_row: a slice of one
    lane and 63 empty ones, length 33.  256-column panels, one and two panels per group, A x, A' y and P x."""
    case = getattr(ssc, name)(variant)
    _env(monkeypatch, case, OSQP_AMD_PANEL=2, OSQP_AMD_PANEL_SHIFT=ssc.SHIFT, OSQP_AMD_PANEL_GROUP=group)
    m = _setup(product_lib, case)
    lays = _layouts(m, case, 2, ssc.SHIFT, group)
    _one_tile_per_group(lays[0], case.A, ssc.SHIFT)
    _check(product_lib, m, case, _products(case), lays, "lds-panels")
    oq.clean(m)


@pytest.mark.parametrize("group", ssc.GROUPS)
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_last_local_row_of_a_full_tile(product_lib, monkeypatch, variant, group):
    """Tiles of exactly 3968 rows at 64-column panels; local row 3967 sits in a slice of length 17 with one entry, in front of
    52 empty lanes.  Taken for an empty lane, its row sum would be 0 instead of 3 a."""
    case = ssc.last_local_row(variant)
    _env(monkeypatch, case, OSQP_AMD_PANEL=2, OSQP_AMD_PANEL_SHIFT=6, OSQP_AMD_PANEL_GROUP=group)
    m = _setup(product_lib, case)
    lays = _layouts(m, case, 2, 6, group)
    assert lays[0]["tiles"] == 2 * lays[0]["NG"], lays[0]  # 7936 rows, never more than 3968 per tile: two tiles of exactly 3968
    prods = _products(case)
    assert prods[0].exact[case.notes["row"]] == 3.0 * case.A[case.notes["row"], case.notes["col"]] != 0.0
    _check(product_lib, m, case, prods, lays, "lds-panels")
    oq.clean(m)


@pytest.mark.parametrize("group", ssc.GROUPS)
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_ladder_on_wide_panels(product_lib, monkeypatch, variant, group):
    """The ladder over wide panels of 128 columns gathered through L2 (32-bit column ids, no staging)."""
    case = ssc.ladder(variant)
    _env(monkeypatch, case, OSQP_AMD_PANEL=3, OSQP_AMD_PANEL_SHIFT=6, OSQP_AMD_WIDE_SHIFT=7, OSQP_AMD_PANEL_GROUP=group)
    m = _setup(product_lib, case)
    lays = _layouts(m, case, 3, 6, group, wide_shift=7)
    _one_tile_per_group(lays[0], case.A, 7)
    _check(product_lib, m, case, _products(case), lays, "wide-panels")
    oq.clean(m)


def _new_values(case, seed):
    """Every stored entry of triu P and A times its own factor from {2, -3} (the diagonal of P: 3, it still dominates)."""
    rng = np.random.default_rng(seed)
    P = case.P.copy(); A = case.A.copy()
    fp = rng.choice(np.array([2.0, -3.0]), size=P.nnz)
    fp[P.indices == np.repeat(np.arange(P.shape[1]), np.diff(P.indptr))] = 3.0
    P.data = P.data * fp
    A.data = A.data * rng.choice(np.array([2.0, -3.0]), size=A.nnz)
    return P, A


@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_ladder_after_a_value_refresh(product_lib, monkeypatch, variant):
    """A full update of A and P rewrites the slice values through cellbase; the table stays."""
    case = ssc.ladder(variant)
    _env(monkeypatch, case, OSQP_AMD_PANEL=2, OSQP_AMD_PANEL_SHIFT=ssc.SHIFT, OSQP_AMD_PANEL_GROUP=2)
    m = _setup(product_lib, case)
    P2, A2 = _new_values(case, 41)
    oq.update(m, Px=P2.data, Ax=A2.data)
    lays = _layouts(m, case, 2, ssc.SHIFT, 2)
    _one_tile_per_group(lays[0], case.A, ssc.SHIFT)
    _check(product_lib, m, case, case.products(P2, A2), lays, "lds-panels after a full update")
    oq.clean(m)


# ---------------------------------------------------------------------------------------------------------------------
# every switch off against on: the same bits
# ---------------------------------------------------------------------------------------------------------------------
def device_products(lib, setenv):
    """The three products of the real-valued ladder and of spmv_cases.ragged on 256-column panels, two panels per group."""
    out = {}
    for case in (ssc.ladder("real"), sc.ragged("real")):
        for k, v in (("OSQP_AMD_PANEL", 2), ("OSQP_AMD_PANEL_SHIFT", ssc.SHIFT), ("OSQP_AMD_PANEL_GROUP", 2)):
            setenv(k, str(v))
        m = _setup(lib, case)
        for op in (0, 1, 2):
            assert oq.spmv_layout(m, op)["kernel"] == 2
            out["%s_%d" % (case.name, op)] = _apply(lib, m, case, op)
        oq.clean(m)
    return out


_ON = {}


@pytest.mark.parametrize("switch", SWITCHES)
def test_a_switch_off_gives_the_bits_of_on(product_lib, monkeypatch, tmp_path, switch):
    """A switch is read once per process: this process runs with it on (the default), a child with it off."""
    assert all(os.environ.get(k, "1") != "0" for k in SWITCHES), "this process must run the default path"
    if not _ON:
        for k in ENV:
            monkeypatch.delenv(k, raising=False)
        _ON.update(device_products(product_lib, monkeypatch.setenv))
    path = str(tmp_path / "off.npz")
    env = {k: v for k, v in os.environ.items() if k not in ENV}
    env[switch] = "0"
    subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=HERE, check=True, timeout=300)
    off = np.load(path)
    assert sorted(off.files) == sorted(_ON)
    for k, a in _ON.items():
        bad = np.nonzero(a != off[k])[0]
        assert np.array_equal(a, off[k]), (switch, k, "rows", bad[:8], a[bad[:8]], off[k][bad[:8]])
        assert np.all(np.isfinite(a))


if __name__ == "__main__":  # the child of the test above: products with the environment it was given
    np.savez(sys.argv[1], **device_products(oq.load_library(), os.environ.__setitem__))
