"""The single panel product with its group sums added up inside the product launch (csrc/panel.hip k_spmv_sell_fused,
OSQP_AMD_PANEL_FUSED_REDUCE) against the two-kernel form (k_spmv_sell + k_panel_reduce): the same bits, and both inside the
exact-reference bound of spmv_reference.py.

Products.  The seeded families of spmv_cases.py (ragged at three widths, many_short_rows, slice_edges, long_rows, and flat for a
matrix of fewer rows than a reduce block) through op 0, 1, 2 of osqp_amd_apply under OSQP_AMD_PANEL=2, panel shifts 6 and 8,
1-4 panels per group and reduce blocks of 64 rows (OSQP_AMD_PANEL_RBLOCK=64; one run at the default of 2048).  Every case
builds two workspaces from the same data, one with the switch on and one with it off: array_equal outputs, both inside
(L + NG + 2) 2^-53 sum |a||x| per row, rows without entries +0.0, twenty launches in a row equal to the first (the arrival
counters are back at zero after every launch).  The layout the device reports is held against the layout arithmetic of
spmv_cases.py (kernel, B, Gp, NG) and against tile_cuts below, the tile cuts of panel.hip restated on the host -- from which
the shape facts the cases are there for are worked out, not assumed (test_the_cases_hold_the_shapes_they_are_there_for).

Solver.  The generated QP of kind 0, n = 20 000, 20 per row, on 256-column panels, 40 iterations of osqp_amd_iterate, switch on
against off: identical iterates, CG totals and residuals -- in this process with the paired A p / P p launch (the right-hand
side, A' t and the residual products run fused, with every sum over rows in its separate pass), and in a child process with
OSQP_AMD_SPMV_PAIR=0 (read once per process), where A p with its second output and P p + sigma p run fused too: the path of
the headline workload, whose layouts are too large for the pair.

One evaluation per iteration.  osqp_amd_iterate(50) at check_termination = 25 evaluates iteration 50 once: the iterate,
residuals and objective of 49 iterations plus 1 (which evaluate at 25, 49 and 1), with three whole-matrix products fewer in
stats[26] (6 against 9).  On the direct back-end: its iterations do not depend on how the calls are cut (the indirect one
restarts its CG start vector at every call)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # run as the child of the unpaired solver test: no conftest has put the package on the path
    sys.path.insert(0, ROOT)

import osqp_jl_amd as oq
import spmv_cases as sc
import spmv_reference as ref

pytestmark = pytest.mark.gpu
f = oq.interface._fptr
HERE = os.path.dirname(os.path.abspath(__file__))

ENV = ("OSQP_AMD_PANEL", "OSQP_AMD_PANEL_SHIFT", "OSQP_AMD_PANEL_GROUP", "OSQP_AMD_PANEL_TILE_NNZ", "OSQP_AMD_WIDE_SHIFT",
       "OSQP_AMD_SPMV_G", "OSQP_AMD_COMPACT_NNZ", "OSQP_AMD_PANEL_FUSED_REDUCE", "OSQP_AMD_PANEL_RBLOCK")
RBLOCK = 64
NG_WANTED = {1, 3, 4, 5, 8, 9, 13}  # every piece of the 8-wide / 4-wide / scalar group sum, alone and combined
CUS = 256                           # compute units of the device (the tile budget of a small single-panel group depends on it)

# (builder, builder arguments, panel shift, panels per group, reduce block or None for the default)
RUNS = [("ragged", (("n", n),), shift, g, RBLOCK) for n in (800, 1000, 1100) for shift in sc.LDS_SHIFTS for g in sc.GROUPS]
RUNS += [(name, (), shift, g, RBLOCK) for name in ("many_short_rows", "slice_edges", "long_rows") for shift in sc.LDS_SHIFTS for g in sc.GROUPS]
RUNS += [("flat", (), shift, g, RBLOCK) for shift in sc.LDS_SHIFTS for g in (1, 3)]
RUNS += [("ragged", (), 8, 2, None)]


def _id(run):
    name, kw, shift, g, rb = run
    return "%s%s-s%d-g%d-r%s" % (name, "".join("-%s%s" % kv for kv in kw), shift, g, rb if rb else "dflt")


def _case(run, variant="real"):
    name, kw, shift, _, _ = run
    return sc.build(name, variant, shift, **dict(kw))


# ---------------------------------------------------------------------------------------------------------------------
# the tile cuts of panel.hip (panel_build: k_tile_cost, k_tile_starts), restated
# ---------------------------------------------------------------------------------------------------------------------
def tile_cuts(M, shift, group, tile_nnz_env=None):
    """[(group, r0, r1)] for a matrix on LDS panels of 2^shift columns, `group` panels per group.  Every (group, row) cell
    costs max(entries, cmin), cmin = ceil(budget / 3968); the cells of a group whose exclusive cost offset falls into the same
    window of `budget` share a tile.  budget = max(tile_nnz Gp, 3968); tile_nnz = OSQP_AMD_PANEL_TILE_NNZ, else 65536 -- cut
    to max(32768, min(65536, nnz / (0.85 CUs))) for a layout of single-panel groups with fewer than one tile per compute unit."""
    M = sp.csr_matrix(M)
    rows, cols = M.shape
    cell = sc.structure(M, shift)["cell"]
    B = cell.shape[1]
    Gp = min(group, B)
    NG = (B + Gp - 1) // Gp
    tile_nnz = 65536 if tile_nnz_env is None else int(tile_nnz_env)
    if tile_nnz_env is None and Gp == 1 and M.nnz / tile_nnz < CUS:
        tile_nnz = max(32768, min(tile_nnz, int(M.nnz / (0.85 * CUS))))
    budget = max(tile_nnz * Gp, sc.TILE_ROWS_MAX)
    cmin = -(-budget // sc.TILE_ROWS_MAX)
    tiles = []
    for g in range(NG):
        cost = np.maximum(cell[:, g * Gp:(g + 1) * Gp].sum(axis=1), cmin)
        win = (np.cumsum(cost) - cost) // budget
        starts = np.nonzero(np.concatenate(([True], win[1:] != win[:-1])))[0]
        ends = np.concatenate((starts[1:], [rows]))
        tiles += [(g, int(a), int(b)) for a, b in zip(starts, ends)]
    return tiles


def shape_facts(M, shift, group, R, tile_nnz_env=None):
    """What the fused reduce meets on this matrix at reduce blocks of R rows."""
    rows = M.shape[0]
    tiles = tile_cuts(M, shift, group, tile_nnz_env)
    met = {}
    for g, r0, r1 in tiles:
        for k in range(r0 // R, (r1 - 1) // R + 1):
            met[(g, k)] = met.get((g, k), 0) + 1
    return dict(tiles=len(tiles), rows_not_a_multiple=rows % R != 0, fewer_rows_than_a_block=rows < R,
                tile_meets_three_blocks=any((r1 - 1) // R - r0 // R + 1 >= 3 for _, r0, r1 in tiles),
                block_met_by_tiles_of_one_group=max(met.values()) >= 2,
                empty_rows=bool(np.any(np.diff(sp.csr_matrix(M).indptr) == 0)))


def _panel_ops(case, shift):
    """The ops of the case whose matrix gets panels at this width (flat: A' has too few columns and stays on the CSR kernel)."""
    return [op for op, (M, _) in case.matrices().items() if M.shape[1] > (1 << shift)]


def test_the_cases_hold_the_shapes_they_are_there_for():
    """Host arithmetic only: over RUNS, every NG of NG_WANTED occurs and every shape fact occurs at reduce blocks of 64 rows."""
    ngs, facts = set(), {}
    for run in RUNS:
        name, _, shift, g, rb = run
        if rb is None:
            continue
        case = _case(run)
        for op in _panel_ops(case, shift):
            M = case.matrices()[op][0]
            ngs.add(sc.expected_layout(M.shape[1], 2, shift, g)["NG"])
            for k, v in shape_facts(M, shift, g, rb, case.env.get("OSQP_AMD_PANEL_TILE_NNZ")).items():
                if k != "tiles":
                    facts[k] = facts.get(k, False) or v
    assert NG_WANTED <= ngs, sorted(NG_WANTED - ngs)
    assert all(facts.values()), facts


# ---------------------------------------------------------------------------------------------------------------------
# products: on against off
# ---------------------------------------------------------------------------------------------------------------------
def _env(monkeypatch, case, **env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**env, **case.env}.items():
        if v is not None:
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


_PRODUCTS = {}


def _products(run, case):
    key = run[:3]
    if key not in _PRODUCTS:
        _PRODUCTS[key] = case.products()
    return _PRODUCTS[key]


@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_fused_reduce_gives_the_bits_of_the_two_kernel_form(product_lib, monkeypatch, run):
    name, _, shift, group, rb = run
    case = _case(run)
    prods = _products(run, case)
    ops = _panel_ops(case, shift)
    assert 0 in ops and 2 in ops and (1 in ops or case.m <= (1 << shift))  # A' stays on the CSR kernel when m fits one panel
    ms = {}
    for on in (1, 0):
        _env(monkeypatch, case, OSQP_AMD_PANEL=2, OSQP_AMD_PANEL_SHIFT=shift, OSQP_AMD_PANEL_GROUP=group, OSQP_AMD_PANEL_RBLOCK=rb,
             OSQP_AMD_PANEL_FUSED_REDUCE=on)
        ms[on] = _setup(product_lib, case)
    for op in ops:
        M = case.matrices()[op][0]
        want = sc.expected_layout(M.shape[1], 2, shift, group)
        tiles = len(tile_cuts(M, shift, group, case.env.get("OSQP_AMD_PANEL_TILE_NNZ")))
        for on in (1, 0):
            lay = oq.spmv_layout(ms[on], op)
            assert lay["kernel"] == want["kernel"] == 2 and lay["nnz"] == M.nnz, (_id(run), op, on, lay, want)
            assert all(lay[k] == want[k] for k in ("shift", "B", "Gp", "NG")) and lay["tiles"] == tiles, (_id(run), op, on, lay, want, tiles)
            # the switch and the block size arrived: the two workspaces are the two forms, not one form twice
            assert lay["fused"] == on and (1 << lay["rshift"]) == (rb or 2048), (_id(run), op, on, lay)
        before = {on: oq.spmv_layout(ms[on], op)["fused_launches"] for on in (1, 0)}
        what = (_id(run), "op", op)
        first = _apply(product_lib, ms[1], case, op)
        off = _apply(product_lib, ms[0], case, op)
        bad = np.nonzero(first != off)[0]
        assert np.array_equal(first, off), (what, "fused differs from two kernels in rows", bad[:8], first[bad[:8]], off[bad[:8]])
        ref.assert_product(first, prods[op], want["NG"], what + ("fused",))
        ref.assert_product(off, prods[op], want["NG"], what + ("two kernels",))
        for rep in range(20):  # the counters are back at zero: every launch is the first
            again = _apply(product_lib, ms[1], case, op)
            assert np.array_equal(again, first), (what, "launch", rep + 2, np.nonzero(again != first)[0][:8])
        ran = {on: oq.spmv_layout(ms[on], op)["fused_launches"] - before[on] for on in (1, 0)}
        assert ran == {1: 21, 0: 0}, (what, "products on k_spmv_sell_fused", ran)  # every launch of the one, none of the other
    for m in ms.values():
        oq.clean(m)


def test_integer_products_are_exact_under_the_fused_reduce(product_lib, monkeypatch):
    """The integer variants (any order of summation is exact): a dropped, doubled or misplaced row cannot hide."""
    for run in (("ragged", (("n", 800),), 6, 1, RBLOCK), ("many_short_rows", (), 8, 2, RBLOCK), ("long_rows", (), 6, 3, RBLOCK)):
        name, _, shift, group, rb = run
        case = _case(run, "int")
        _env(monkeypatch, case, OSQP_AMD_PANEL=2, OSQP_AMD_PANEL_SHIFT=shift, OSQP_AMD_PANEL_GROUP=group, OSQP_AMD_PANEL_RBLOCK=rb,
             OSQP_AMD_PANEL_FUSED_REDUCE=1)
        m = _setup(product_lib, case)
        prods = case.products()
        for op in (0, 1, 2):
            lay = oq.spmv_layout(m, op)
            assert lay["kernel"] == 2 and lay["fused"] == 1 and lay["rshift"] == 6, lay
            ref.assert_product(_apply(product_lib, m, case, op), prods[op], lay["NG"], (_id(run), "int", "op", op))
            assert oq.spmv_layout(m, op)["fused_launches"] == lay["fused_launches"] + 1
        oq.clean(m)


# ---------------------------------------------------------------------------------------------------------------------
# solver level
# ---------------------------------------------------------------------------------------------------------------------
def solver_run(lib, setenv, fused, n=20000, per_row=20, iters=40):
    for k, v in (("OSQP_AMD_PANEL", 2), ("OSQP_AMD_PANEL_SHIFT", 8), ("OSQP_AMD_PANEL_GROUP", 4), ("OSQP_AMD_PANEL_FUSED_REDUCE", fused)):
        setenv(k, str(v))
    m = oq.Model(lib)
    oq.setup_generated(m, 0, n, per_row, 3, linsys_solver="pcg", verbose=False, check_termination=25, adaptive_rho_interval=50, polish=False)
    lays = [oq.spmv_layout(m, op) for op in (0, 1, 2)]
    assert all(lay["kernel"] == 2 and lay["shift"] == 8 and lay["fused"] == fused for lay in lays), lays
    st0 = oq.stats(m)
    assert lib.osqp_amd_iterate(m.workspace, iters) == 0
    nn, mm = oq.dimensions(m)
    x, y = np.full(nn, np.nan), np.full(mm, np.nan)
    assert lib.osqp_amd_get_iterate(m.workspace, f(x), f(y)) == 0
    info = m.workspace.contents.info.contents
    st = oq.stats(m)
    out = dict(x=x, y=y, cg=np.array([st[6] - st0[6]]), res=np.array([float(info.pri_res), float(info.dua_res), float(info.obj_val)]),
               backend=np.array([st[0]]),
               launches=np.array([oq.spmv_layout(m, op)["fused_launches"] - lays[op]["fused_launches"] for op in (0, 1, 2)]))
    oq.clean(m)
    return out


def _same_solver_runs(a, b, what):
    assert a["backend"][0] == b["backend"][0] == 2.0
    for k in ("x", "y", "cg", "res"):
        assert np.all(np.isfinite(a[k])), (what, k)
        assert np.array_equal(a[k], b[k]), (what, k, a[k][:4], b[k][:4])
    assert a["cg"][0] >= 40, (what, a["cg"])
    # `a` ran products of A, A' and P on k_spmv_sell_fused during the iterations (at the least those of the residual
    # evaluation at iteration 25), `b` none
    assert np.all(a["launches"] >= 1) and np.all(b["launches"] == 0), (what, a["launches"], b["launches"])


def test_forty_iterations_fused_against_two_kernels(product_lib, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    on = solver_run(product_lib, monkeypatch.setenv, 1)
    off = solver_run(product_lib, monkeypatch.setenv, 0)
    _same_solver_runs(on, off, "paired A p / P p")


def test_forty_iterations_fused_against_two_kernels_without_the_pair_launch(tmp_path):
    """OSQP_AMD_SPMV_PAIR is read once per process: a child runs both forms with the pair launch off."""
    path = str(tmp_path / "unpaired.npz")
    env = {k: v for k, v in os.environ.items() if k not in ENV}
    env["OSQP_AMD_SPMV_PAIR"] = "0"
    subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=HERE, check=True, timeout=300)
    got = np.load(path)
    on = {k[3:]: got[k] for k in got.files if k.startswith("on_")}
    off = {k[4:]: got[k] for k in got.files if k.startswith("off_")}
    _same_solver_runs(on, off, "single A p and P p")


# ---------------------------------------------------------------------------------------------------------------------
# the last iteration of a call is evaluated once
# ---------------------------------------------------------------------------------------------------------------------
def test_fifty_iterations_evaluate_the_fiftieth_once(product_lib, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    runs = {}
    for cuts in ((50,), (49, 1)):
        m = oq.Model(product_lib)
        oq.setup_generated(m, 1, 3000, 0, 5, linsys_solver="direct", verbose=False, check_termination=25, adaptive_rho_interval=50, polish=False)
        st0 = oq.stats(m)
        assert st0[0] == 0.0 and len(st0) == 27
        for k in cuts:
            assert product_lib.osqp_amd_iterate(m.workspace, k) == 0
        nn, mm = oq.dimensions(m)
        x, y = np.full(nn, np.nan), np.full(mm, np.nan)
        assert product_lib.osqp_amd_get_iterate(m.workspace, f(x), f(y)) == 0
        info = m.workspace.contents.info.contents
        st = oq.stats(m)
        runs[cuts] = dict(x=x, y=y, res=(float(info.pri_res), float(info.dua_res), float(info.obj_val)), products=st[26] - st0[26],
                          iters=st[7] - st0[7])
        oq.clean(m)
    a, b = runs[(50,)], runs[(49, 1)]
    assert a["iters"] == b["iters"] == 50
    assert np.all(np.isfinite(a["x"])) and np.all(np.isfinite(a["y"])) and all(np.isfinite(v) for v in a["res"])
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["y"], b["y"])
    assert a["res"] == b["res"], (a["res"], b["res"])
    assert a["products"] == 6 and b["products"] == 9, (a["products"], b["products"])  # evaluations at 25, 50 against 25, 49, 1


if __name__ == "__main__":  # the child of the unpaired solver test
    lib = oq.load_library()
    out = {}
    for tag, fused in (("on", 1), ("off", 0)):
        out.update({"%s_%s" % (tag, k): v for k, v in solver_run(lib, os.environ.__setitem__, fused).items()})
    np.savez(sys.argv[1], **out)
