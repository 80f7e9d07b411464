"""GPU parity tests proper: the HIP engine, called through its C ABI, against
(a) the reference's known answers (same cases as test_oracle_golden.py) and
(b) the CPU oracle on the same seeded inputs.  Floating-point tolerance: the
solutions must agree to the solver's own eps (BASELINE.json north_star); kernel
level checks (SpMV, KKT solve) use 1e-12 relative."""
import numpy as np
import pytest
import scipy.sparse as sp

import osqp_jl_amd as oq
import qp_cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("linsys", ["qdldl", "pcg"])
@pytest.mark.parametrize("case", qp_cases.ALL_CASES, ids=lambda f: f.__name__)
def test_product_case(product_lib, case, linsys):
    case(oq, product_lib, linsys)


def _data_to_scipy(d):
    n, m = int(d.n), int(d.m)
    def mat(c):
        nn = int(c.n)
        p = np.ctypeslib.as_array(c.p, shape=(nn + 1,)).copy()
        nz = int(p[-1])
        i = np.ctypeslib.as_array(c.i, shape=(max(nz, 1),))[:nz].copy()
        x = np.ctypeslib.as_array(c.x, shape=(max(nz, 1),))[:nz].copy()
        return sp.csc_matrix((x, i, p), shape=(int(c.m), nn))
    P = mat(d.P.contents); A = mat(d.A.contents)
    q = np.ctypeslib.as_array(d.q, shape=(n,)).copy()
    l = np.ctypeslib.as_array(d.l, shape=(max(m, 1),))[:m].copy()
    u = np.ctypeslib.as_array(d.u, shape=(max(m, 1),))[:m].copy()
    return P, q, A, l, u


@pytest.mark.parametrize("kind,n,k", [(0, 3000, 12), (0, 700, 64), (1, 5000, 0)])
def test_device_generator_matches_host_generator(product_lib, oracle_lib, kind, n, k):
    """The device generator and oracle/gen.c produce the same problem: a solve of
    the device-generated problem equals a solve of the host-generated one fed
    through osqp_setup, and SpMV through the ABI hook equals scipy on the host data."""
    d = oracle_lib.oracle_generate(kind, n, k, 7)
    P, q, A, l, u = _data_to_scipy(d.contents)
    oracle_lib.oracle_data_free(d)
    opts = dict(verbose=False, eps_abs=1e-6, eps_rel=1e-6, adaptive_rho_interval=25, linsys_solver="pcg")
    mg = oq.Model(product_lib)
    oq.setup_generated(mg, kind, n, k, 7, **opts)
    rng = np.random.default_rng(0)
    nn, mm = oq.dimensions(mg)
    assert (nn, mm) == (P.shape[0], A.shape[0])
    # bit-level: unscaled data are not reachable after setup, so compare through scaling-free setup
    mg0 = oq.Model(product_lib)
    oq.setup_generated(mg0, kind, n, k, 7, scaling=0, **opts)
    xv = rng.standard_normal(nn); yv = rng.standard_normal(mm)
    out = np.zeros(mm); product_lib.osqp_amd_apply(mg0.workspace, 0, oq.interface._fptr(xv), oq.interface._fptr(out))
    ref = A @ xv
    assert np.max(np.abs(out - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))
    out = np.zeros(nn); product_lib.osqp_amd_apply(mg0.workspace, 1, oq.interface._fptr(yv), oq.interface._fptr(out))
    ref = A.T @ yv
    assert np.max(np.abs(out - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))
    out = np.zeros(nn); product_lib.osqp_amd_apply(mg0.workspace, 2, oq.interface._fptr(xv), oq.interface._fptr(out))
    Pfull = P + sp.triu(P, 1).T
    ref = Pfull @ xv
    assert np.max(np.abs(out - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))
    # solution-level
    rg = oq.solve(mg)
    mh = oq.Model(product_lib)
    oq.setup(mh, P=P, q=q, A=A, l=l, u=u, **opts)
    rh = oq.solve(mh)
    assert rg.info.status == rh.info.status == "Solved"
    assert rg.info.iter == rh.info.iter
    assert np.allclose(rg.x, rh.x, atol=1e-9) and np.allclose(rg.y, rh.y, atol=1e-9)


@pytest.mark.parametrize("linsys", ["pcg", "direct"])  # "direct" = forced LDL' (auto would pick PCG for the fill-heavy random QP)
@pytest.mark.parametrize("kind,n,k", [(0, 2000, 20), (1, 4000, 0)])
def test_solution_parity_with_oracle(product_lib, oracle_lib, kind, n, k, linsys):
    """Same seeded problem, same settings: HIP engine vs CPU oracle agree to the
    solver's own eps (here 1e-5 requested, compared at 2e-4 on x and y) and
    reach the same status in a comparable number of iterations."""
    opts = dict(verbose=False, eps_abs=1e-5, eps_rel=1e-5, adaptive_rho_interval=25, linsys_solver=linsys)
    mo = oq.Model(oracle_lib); oq.setup_generated(mo, kind, n, k, 3, **opts); ro = oq.solve(mo)
    mp = oq.Model(product_lib); oq.setup_generated(mp, kind, n, k, 3, **opts); rp = oq.solve(mp)
    assert ro.info.status == rp.info.status == "Solved"
    assert abs(ro.info.iter - rp.info.iter) <= 25
    scale = max(1.0, np.max(np.abs(ro.x)))
    assert np.max(np.abs(ro.x - rp.x)) <= 2e-4 * scale
    assert np.max(np.abs(ro.y - rp.y)) <= 2e-4 * max(1.0, np.max(np.abs(ro.y)))
    assert abs(ro.info.obj_val - rp.info.obj_val) <= 1e-4 * max(1.0, abs(ro.info.obj_val))


def test_iterates_match_oracle_early(product_lib, oracle_lib):
    """Fixed number of ADMM iterations from a cold start (no termination test):
    the device iterates track the CPU iterates to rounding (1e-9)."""
    fx, prob = qp_cases.load_polish_fixture()
    opts = dict(verbose=False, eps_abs=1e-12, eps_rel=1e-12, adaptive_rho=False, max_iter=40, check_termination=0,
                linsys_solver="qdldl")
    res = []
    for lib in (oracle_lib, product_lib):
        m = oq.Model(lib); oq.setup(m, **prob, **opts); r = oq.solve(m)
        assert r.info.status == "Max_iter_reached" and r.info.iter == 40
        res.append(r)
    assert np.max(np.abs(res[0].x - res[1].x)) <= 1e-9
    assert np.max(np.abs(res[0].y - res[1].y)) <= 1e-9
    assert abs(res[0].info.pri_res - res[1].info.pri_res) <= 1e-9
    assert abs(res[0].info.dua_res - res[1].info.dua_res) <= 1e-9


def test_alpha_update_after_a_solve_is_honoured(product_lib, oracle_lib):
    """The `check_termination` iterations of the direct back-end are replayed from a captured hipGraph whose nodes
    hold alpha as a launch argument: `update_settings!(model, alpha=...)` [REF src/interface.jl:552-563] after a first
    solve must reach the replayed iterations (the graph is dropped and captured again).  Direct back-end on both
    sides: identical iteration counts, before and after the update."""
    opts = dict(verbose=False, eps_abs=1e-5, eps_rel=1e-5, adaptive_rho_interval=50, check_termination=25, linsys_solver="qdldl")
    ms = []
    for lib in (product_lib, oracle_lib):
        m = oq.Model(lib); oq.setup_generated(m, 1, 4000, 0, 3, **opts); ms.append(m)
    r1 = [oq.solve(m) for m in ms]
    assert r1[0].info.status == r1[1].info.status == "Solved" and r1[0].info.iter == r1[1].info.iter
    for m in ms:
        oq.update_settings(m, alpha=1.0, warm_start=False)
    r2 = [oq.solve(m) for m in ms]
    assert r2[0].info.status == r2[1].info.status == "Solved"
    assert r2[0].info.iter == r2[1].info.iter and r2[0].info.iter != r1[0].info.iter
    assert np.max(np.abs(r2[0].x - r2[1].x)) <= 1e-7 and np.max(np.abs(r2[0].y - r2[1].y)) <= 1e-7
    for m in ms:  # rho and the matrices change what the replayed kernels read as well
        oq.update_settings(m, rho=0.3, alpha=1.6)
    r3 = [oq.solve(m) for m in ms]
    assert r3[0].info.iter == r3[1].info.iter and np.max(np.abs(r3[0].x - r3[1].x)) <= 1e-7


def test_large_property_checks(product_lib):
    """BASELINE-size-independent properties on a larger generated problem: the returned
    point satisfies OSQP's own stopping criteria when re-evaluated on the host from
    unscaled data, and a warm-started re-solve converges at the first check."""
    n, k = 50000, 40
    m = oq.Model(product_lib)
    oq.setup_generated(m, 0, n, k, 11, verbose=False, eps_abs=1e-4, eps_rel=1e-4, adaptive_rho_interval=25, linsys_solver="pcg")
    r = oq.solve(m)
    assert r.info.status == "Solved"
    # independent re-evaluation needs the data on the host: regenerate with the host generator
    lib_o = oq.load_library(oq.ORACLE_LIB_PATH)
    d = lib_o.oracle_generate(0, n, k, 11)
    P, q, A, l, u = _data_to_scipy(d.contents)
    lib_o.oracle_data_free(d)
    Pfull = P + sp.triu(P, 1).T
    Ax = A @ r.x
    z = np.clip(Ax, l, u)
    pri = np.max(np.abs(Ax - z))
    dua = np.max(np.abs(Pfull @ r.x + q + A.T @ r.y))
    eps_pri = 1e-4 + 1e-4 * max(np.max(np.abs(Ax)), np.max(np.abs(z)))
    eps_dua = 1e-4 + 1e-4 * max(np.max(np.abs(Pfull @ r.x)), np.max(np.abs(A.T @ r.y)), np.max(np.abs(q)))
    assert pri <= 2 * eps_pri and dua <= 2 * eps_dua
    oq.warm_start(m, x=r.x, y=r.y)
    r2 = oq.solve(m)
    assert r2.info.status == "Solved" and r2.info.iter <= 25


@pytest.mark.parametrize("mode,group", [("2", "1"), ("2", "2"), ("2", "4"), ("3", "1")])
def test_panel_spmv_matches_scipy(product_lib, oracle_lib, monkeypatch, mode, group):
    """The column-panel SpMV (csrc/panel.hip, used when x does not fit the caches) against scipy on the host-generated
    matrix, forced on at a size the test can hold: LDS-staged panels (3 panels of 16384 columns; 1, 2 or 4 panels per
    workgroup tile -- 1 below nnz = 2.7e8, 4 above) and the wide panels gathered through L2 (mode 3)."""
    monkeypatch.setenv("OSQP_AMD_PANEL", mode)
    monkeypatch.setenv("OSQP_AMD_PANEL_GROUP", group)
    n, k = 40000, 96
    d = oracle_lib.oracle_generate(0, n, k, 21)
    P, q, A, l, u = _data_to_scipy(d.contents)
    oracle_lib.oracle_data_free(d)
    m = oq.Model(product_lib)
    oq.setup_generated(m, 0, n, k, 21, scaling=0, verbose=False, linsys_solver="pcg")
    for which in (0, 1, 2):  # A, A' and P really run the kernel the test names, with the panels per group it asks for
        lay = oq.spmv_layout(m, which)
        assert lay["kernel"] == int(mode) and lay["Gp"] == min(int(group), lay["B"]), (which, lay)
        assert lay["B"] == (3 if mode == "2" else 1) and lay["compact"] == 0, (which, lay)
    rng = np.random.default_rng(5)
    xv, yv = rng.standard_normal(n), rng.standard_normal(n)
    Pfull = P + sp.triu(P, 1).T
    for op, mat, vec in ((0, A, xv), (1, A.T, yv), (2, Pfull, xv)):
        out = np.zeros(n)
        assert product_lib.osqp_amd_apply(m.workspace, op, oq.interface._fptr(vec), oq.interface._fptr(out)) == 0
        ref = mat @ vec
        assert np.max(np.abs(out - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))
    # value updates reach the panel copies: scale every entry of A and of triu(P) through osqp_update_P_A
    A2 = A.copy(); A2.data = A2.data * 1.5
    Pu = sp.triu(P, format="csc"); Pu2 = Pu.copy(); Pu2.data = Pu2.data * 0.5
    oq.update(m, Px=Pu2.data, Ax=A2.data)
    P2full = Pu2 + sp.triu(Pu2, 1).T
    for op, mat, vec in ((0, A2, xv), (1, A2.T, yv), (2, P2full, xv)):
        out = np.zeros(n)
        assert product_lib.osqp_amd_apply(m.workspace, op, oq.interface._fptr(vec), oq.interface._fptr(out)) == 0
        ref = mat @ vec
        assert np.max(np.abs(out - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))
    # and a whole solve through the panel kernels equals the CSR-kernel solve to rounding
    opts = dict(verbose=False, eps_abs=1e-6, eps_rel=1e-6, adaptive_rho_interval=25, linsys_solver="pcg")
    mp_ = oq.Model(product_lib); oq.setup_generated(mp_, 0, n, k, 21, **opts); rp = oq.solve(mp_)
    monkeypatch.setenv("OSQP_AMD_PANEL", "0")
    mc = oq.Model(product_lib); oq.setup_generated(mc, 0, n, k, 21, **opts); rc = oq.solve(mc)
    for which in (0, 1, 2):
        assert oq.spmv_layout(mp_, which)["kernel"] == int(mode) and oq.spmv_layout(mc, which)["kernel"] == 0
    assert rp.info.status == rc.info.status == "Solved" and rp.info.iter == rc.info.iter
    assert np.max(np.abs(rp.x - rc.x)) <= 1e-9 and np.max(np.abs(rp.y - rc.y)) <= 1e-9


def test_compact_mode(product_lib, oracle_lib, monkeypatch):
    """Compact workspaces (the CSR column / value arrays released once the sliced-ELL copies exist; automatic above 5e7
    stored entries, forced here at a size the test can hold): the products, osqp_update_P_A through the slot maps, Ruiz
    scaling and the Jacobi diagonal on the slices -- against scipy and against the same solve on a non-compact workspace."""
    monkeypatch.setenv("OSQP_AMD_PANEL", "2")
    n, k = 40000, 96
    d = oracle_lib.oracle_generate(0, n, k, 21)
    P, q, A, l, u = _data_to_scipy(d.contents)
    oracle_lib.oracle_data_free(d)
    Pu = sp.triu(P, format="csc")
    rng = np.random.default_rng(5)
    xv, yv = rng.standard_normal(n), rng.standard_normal(n)
    f = oq.interface._fptr

    def products(model, Pu_, A_):
        Pfull = Pu_ + sp.triu(Pu_, 1).T
        for op, mat, vec in ((0, A_, xv), (1, A_.T, yv), (2, Pfull, xv)):
            out = np.zeros(n)
            assert product_lib.osqp_amd_apply(model.workspace, op, f(vec), f(out)) == 0
            ref = mat @ vec
            assert np.max(np.abs(out - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))

    monkeypatch.setenv("OSQP_AMD_COMPACT_NNZ", "0")
    m0 = oq.Model(product_lib)
    oq.setup_generated(m0, 0, n, k, 21, scaling=0, verbose=False, linsys_solver="pcg")
    assert oq.stats(m0)[18] == 1.0
    for which in (0, 1, 2):  # all three on the LDS-staged panels, their CSR arrays released
        lay = oq.spmv_layout(m0, which)
        assert (lay["kernel"], lay["B"], lay["compact"]) == (2, 3, 1), (which, lay)
    bytes_compact = oq.stats(m0)[9]
    products(m0, Pu, A)
    # partial updates by index, then everything
    idxA = np.sort(rng.choice(A.nnz, 5000, replace=False)); idxP = np.sort(rng.choice(Pu.nnz, 3000, replace=False))
    A2 = A.copy(); A2.data[idxA] *= -2.0
    Pu2 = Pu.copy(); offdiag = Pu2.tocoo().row[idxP] != Pu2.tocoo().col[idxP]
    Pu2.data[idxP[offdiag]] *= 0.25
    oq.update(m0, Px=Pu2.data[idxP], Px_idx=idxP, Ax=A2.data[idxA], Ax_idx=idxA)  # 0-based positions in the Python mirror
    products(m0, Pu2, A2)
    oq.update(m0, Px=Pu.data * 0.5, Ax=A.data * 1.5)
    Pu3 = Pu.copy(); Pu3.data = Pu.data * 0.5
    A3 = A.copy(); A3.data = A.data * 1.5
    products(m0, Pu3, A3)
    oq.clean(m0)
    # whole solves with scaling, before and after a value update, against a workspace that kept its CSR arrays
    opts = dict(verbose=False, eps_abs=1e-6, eps_rel=1e-6, adaptive_rho_interval=25, linsys_solver="pcg")
    res = {}
    for mode, limit in (("compact", "0"), ("csr", "-1")):
        monkeypatch.setenv("OSQP_AMD_COMPACT_NNZ", limit)
        m = oq.Model(product_lib); oq.setup_generated(m, 0, n, k, 21, **opts)
        assert oq.stats(m)[18] == (1.0 if mode == "compact" else 0.0)
        for which in (0, 1, 2):
            lay = oq.spmv_layout(m, which)
            assert (lay["kernel"], lay["compact"]) == (2, int(mode == "compact")), (which, lay)
        if mode == "csr":
            assert oq.stats(m)[9] > bytes_compact + 12 * 2 * A.nnz  # what the three CSR copies weigh (roughly)
        r1 = oq.solve(m)
        oq.update(m, Px=Pu.data * 1.25, Ax=A.data * 0.8)
        oq.update_settings(m, warm_start=False)
        r2 = oq.solve(m)
        res[mode] = (r1, r2)
        oq.clean(m)
    for a, b in zip(res["compact"], res["csr"]):
        assert a.info.status == b.info.status == "Solved" and abs(a.info.iter - b.info.iter) <= 25
        assert np.max(np.abs(a.x - b.x)) <= 1e-5 * max(1.0, np.max(np.abs(b.x)))
        assert np.max(np.abs(a.y - b.y)) <= 1e-5 * max(1.0, np.max(np.abs(b.y)))


@pytest.mark.parametrize("kind,n,k", [(0, 20000, 40), (0, 3000, 12)])
def test_pcg_forms_are_one_arithmetic(product_lib, monkeypatch, kind, n, k):
    """The CG back-end has three forms of one iteration (pcg.hip): the host loop over the unfused kernels, the same loop over
    the fused kernels (start-up 6 launches, 8 per CG iteration; sums recombined from the same block partials in the same
    order), and the asynchronous form (convergence test on the device, predicated kernels, one hipGraph per ADMM iteration,
    stalled steps finished by the host loop).  Same iteration counts, same CG totals, bit-identical solutions.
    n = 20000 runs on the panel kernels (forced), where the fused kernels apply; n = 3000 on the CSR kernel."""
    monkeypatch.setenv("OSQP_AMD_PANEL", "2")
    opts = dict(verbose=False, eps_abs=1e-6, eps_rel=1e-6, adaptive_rho_interval=25, linsys_solver="pcg")
    out = {}
    for fused, asyn in (("0", "0"), ("1", "0"), ("0", "1"), ("1", "1")):
        monkeypatch.setenv("OSQP_AMD_PCG_FUSED", fused)
        monkeypatch.setenv("OSQP_AMD_PCG_ASYNC", asyn)
        m = oq.Model(product_lib); oq.setup_generated(m, kind, n, k, 5, **opts)
        r1 = oq.solve(m)
        oq.update_q(m, np.random.default_rng(1).standard_normal(n))
        r2 = oq.solve(m)
        out[fused + asyn] = (r1, r2, oq.stats(m)[6])
        oq.clean(m)
    ref = out["00"]
    assert ref[0].info.status == ref[1].info.status == "Solved"
    for key in ("10", "01", "11"):
        for a, b in zip(ref[:2], out[key][:2]):
            assert a.info.status == b.info.status and a.info.iter == b.info.iter, key
            assert np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y), key
            assert a.info.pri_res == b.info.pri_res and a.info.dua_res == b.info.dua_res, key
        assert ref[2] == out[key][2], key  # the same number of CG iterations in total


def test_single_reduction_cg_follows_the_oracles_statement(product_lib, oracle_lib, monkeypatch):
    """Round 5, opt-in (OSQP_AMD_PCG_SR=1): the single-reduction CG recurrence on the device (csrc/pcg.hip k_pcg_sr: every vector
    of a CG iteration updated in one kernel, the last workgroup adds up the partials) against its CPU statement (oracle/pcg.c
    with OSQP_ORACLE_PCG_SINGLE_REDUCTION=1): the same ADMM iteration count, the same number of CG iterations in total, the
    solution to 1e-9, through a second solve with a new q on the same workspace -- and the classic recurrence's solution to
    the solve's own tolerance (a different rounding path to the same point)."""
    monkeypatch.setenv("OSQP_AMD_PANEL", "2")  # the fused kernels (which the recurrence is built on) need the panel products
    n, k = 20000, 40
    opts = dict(verbose=False, eps_abs=1e-6, eps_rel=1e-6, adaptive_rho_interval=25, linsys_solver="pcg")
    q2 = np.random.default_rng(1).standard_normal(n)
    res = {}
    for name, lib, sr in (("oracle", oracle_lib, "1"), ("engine", product_lib, "1"), ("classic", product_lib, "0")):
        monkeypatch.setenv("OSQP_ORACLE_PCG_SINGLE_REDUCTION", sr)
        monkeypatch.setenv("OSQP_AMD_PCG_SR", sr)
        m = oq.Model(lib); oq.setup_generated(m, 0, n, k, 5, **opts)
        r1 = oq.solve(m)
        oq.update_q(m, q2)
        r2 = oq.solve(m)
        res[name] = (r1, r2, oq.stats(m)[6])
        oq.clean(m)
    for a, b in zip(res["oracle"][:2], res["engine"][:2]):
        assert a.info.status == b.info.status == "Solved" and a.info.iter == b.info.iter
        assert np.max(np.abs(a.x - b.x)) <= 1e-9 * max(1.0, np.max(np.abs(a.x)))
        assert np.max(np.abs(a.y - b.y)) <= 1e-9 * max(1.0, np.max(np.abs(a.y)))
    assert res["oracle"][2] == res["engine"][2]
    for a, b in zip(res["classic"][:2], res["engine"][:2]):
        assert b.info.status == "Solved" and abs(a.info.iter - b.info.iter) <= 25
        assert np.max(np.abs(a.x - b.x)) <= 1e-4 * max(1.0, np.max(np.abs(a.x)))


def test_dense_row_and_arrow_P(product_lib, oracle_lib):
    """Rows longer than the LDS sort tile (4096): a dense budget row sum(x) = 1 in A and an arrow-shaped P (dense
    first row / column) go through the global-memory row sort of the CSR build; products against scipy, 30 ADMM iterations
    against the oracle."""
    n = 9000
    rng = np.random.default_rng(3)
    S = sp.random(300, n, density=0.01, random_state=5, format="csc")
    A = sp.vstack([sp.csc_matrix(np.ones((1, n))), S, sp.eye(n, format="csc")], format="csc")
    mrows = A.shape[0]
    l = np.concatenate([[1.0], -np.ones(300), np.zeros(n)])
    u = np.concatenate([[1.0], np.ones(300), np.ones(n)])
    v = 0.01 * rng.standard_normal(n - 1)
    d = 1.0 + rng.random(n)
    P = sp.diags(d).tolil()
    P[0, 0] = 5.0
    P[0, 1:] = v
    P = sp.triu(sp.csc_matrix(P), format="csc")
    q = rng.standard_normal(n)
    opts = dict(verbose=False, eps_abs=1e-6, eps_rel=1e-6, adaptive_rho_interval=25, linsys_solver="pcg")
    m0 = oq.Model(product_lib)
    oq.setup(m0, P=P, q=q, A=A, l=l, u=u, scaling=0, **opts)
    xv = rng.standard_normal(n); yv = rng.standard_normal(mrows)
    Pfull = P + sp.triu(P, 1).T
    for op, mat, vec, nout in ((0, A, xv, mrows), (1, A.T, yv, n), (2, Pfull, xv, n)):
        out = np.zeros(nout)
        assert product_lib.osqp_amd_apply(m0.workspace, op, oq.interface._fptr(vec), oq.interface._fptr(out)) == 0
        ref = mat @ vec
        assert np.max(np.abs(out - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))
    # the problem itself converges slowly (thousands of iterations), so compare a fixed number of iterations; with
    # the direct back-end on both sides (exact KKT solves) the iterates agree to rounding
    fixed = dict(opts, max_iter=30, check_termination=0, adaptive_rho=False)
    res = []
    for lib, ls in ((oracle_lib, "qdldl"), (product_lib, "direct")):
        m = oq.Model(lib); oq.setup(m, P=P, q=q, A=A, l=l, u=u, **dict(fixed, linsys_solver=ls)); res.append(oq.solve(m))
    assert res[0].info.status == res[1].info.status == "Max_iter_reached"
    assert np.max(np.abs(res[0].x - res[1].x)) <= 1e-10 and np.max(np.abs(res[0].y - res[1].y)) <= 1e-10


def test_auto_backend_selection(product_lib):
    """linsys_solver = "qdldl" (0) is "auto" in this library: direct LDL' when the factor is cheap and its level
    schedule shallow (Lasso: 3 levels), PCG when the KKT factor fills (random sparsity) -- SURVEY.md section 0.3."""
    m = oq.Model(product_lib)
    oq.setup_generated(m, 1, 20000, 0, 1, verbose=False)
    assert int(oq.stats(m)[0]) == 0 and oq.stats(m)[5] <= 4
    m = oq.Model(product_lib)
    oq.setup_generated(m, 0, 3000, 30, 1, verbose=False)
    assert int(oq.stats(m)[0]) == 2
    m = oq.Model(product_lib)
    oq.setup_generated(m, 0, 600, 8, 1, verbose=False, linsys_solver="direct")
    assert int(oq.stats(m)[0]) == 0


def test_auto_rule_sends_a_dense_P_to_the_direct_back_end(product_lib, oracle_lib):
    """Round-4 review, item 7b: under the DEFAULT linsys_solver ("qdldl" = auto) a dense P goes to the direct back-end --
    the dense top block is priced by what inverting it on the matrix cores costs (csrc/direct.hip, make_direct) -- the
    block-sweep path runs (>= 512 pivots: k_gj_*), and the solve is the oracle's: same iteration count, x to 1e-7."""
    import qp_zoo

    prob = qp_zoo.equality_qp(n=3000)
    opts = dict(verbose=False, eps_abs=1e-5, eps_rel=1e-5, max_iter=4000, adaptive_rho_interval=25)
    mo = oq.Model(oracle_lib)
    oq.setup(mo, linsys_solver="qdldl", **prob, **opts)
    ro = oq.solve(mo)
    m = oq.Model(product_lib)
    oq.setup(m, linsys_solver="qdldl", **prob, **opts)
    st = oq.stats(m)
    assert int(st[0]) == 0, "the auto rule did not choose the direct back-end"
    assert st[25] >= 512 and st[25] >= 0.9 * prob["P"].shape[0], st[25]  # the dense P is the block; the blocked sweeps took it
    rp = oq.solve(m)
    assert ro.info.status == rp.info.status == "Solved" and ro.info.iter == rp.info.iter
    assert np.max(np.abs(ro.x - rp.x)) <= 1e-7 * max(1.0, np.max(np.abs(ro.x)))
    oq.clean(m); oq.clean(mo)


@pytest.mark.parametrize("n", [1100, 1984])
def test_dense_block_product_from_the_lower_triangle(product_lib, monkeypatch, n):
    """Round 5: the product with the inverted dense top block reads the lower triangle of the symmetric array alone
    (csrc/direct.hip k_dense_apply_sym + k_dense_sym_reduce: a workgroup per 64 x 64 tile, the mirrored half from the same tile
    through LDS, shares added up in a fixed order) -- half the bytes of the iteration of a dense-P problem.  Against the product
    over the full array (OSQP_AMD_DENSE_SYM=0): the same KKT solves, before and after a refactorisation, on a block whose size
    is not a multiple of the tile (padded) and on one that is."""
    import ctypes as C

    import qp_zoo

    prob = qp_zoo.equality_qp(n=n)
    rhs = np.random.default_rng(21).standard_normal(n + n // 2)
    sols = {}
    for sym in ("0", "1"):
        monkeypatch.setenv("OSQP_AMD_DENSE_SYM", sym)
        m = oq.Model(product_lib)
        oq.setup(m, linsys_solver="direct", verbose=False, adaptive_rho=False, **prob)
        assert oq.stats(m)[25] >= 512
        out = []
        for rho in (None, 0.37):
            if rho is not None:
                oq.update_settings(m, rho=rho)
            o = np.empty_like(rhs)
            assert m.lib.osqp_amd_apply(m.workspace, 3, rhs.ctypes.data_as(C.POINTER(C.c_double)), o.ctypes.data_as(C.POINTER(C.c_double))) == 0
            out.append(o)
        r = oq.solve(m)
        assert r.info.status == "Solved"
        sols[sym] = out + [r.x.copy()]
        oq.clean(m)
    for k in range(3):
        a, b = sols["0"][k], sols["1"][k]
        assert np.all(np.isfinite(b))
        assert np.max(np.abs(a - b)) <= 1e-9 * max(1.0, np.max(np.abs(a))), (n, k, np.max(np.abs(a - b)))


def test_auto_rule_still_sends_random_sparsity_to_pcg(product_lib):
    """Item 7c: the same rule on a fill-heavy problem of the same size (random sparsity, n = m = 3000, 30 per row: the factor
    fills to a dense block with nothing cheap about the columns below it) still falls through to the indirect back-end."""
    m = oq.Model(product_lib)
    oq.setup_generated(m, 0, 3000, 30, 1, verbose=False)
    st = oq.stats(m)
    assert int(st[0]) == 2 and st[25] == 0
    r = oq.solve(m)
    assert r.info.status == "Solved" and st[6] == 0 and oq.stats(m)[6] > 0  # CG iterations were what solved it
    oq.clean(m)


def test_full_size_properties(product_lib):
    """BASELINE.json's full-size workload (n = m = 1e6, nnz(A) = 1e9) cannot be rebuilt on the host inside a test,
    so it is checked through size-independent properties of the operators the solve is made of -- the CSR /
    sliced-ELL copies of A, A' and P are built by independent code paths, so these identities tie them together:
      adjointness  y'(A x) = x'(A' y),   symmetry  x'(P y) = y'(P x),   linearity  A(a x + y) = a A x + A y,
    plus the solver-level ones: a solve reaches eps = 1e-4, and a warm-started re-solve stops at its first check."""
    n = 1_000_000
    m = oq.Model(product_lib)
    oq.setup_generated(m, 0, n, 1000, 1, verbose=False, eps_abs=1e-4, eps_rel=1e-4, adaptive_rho_interval=50,
                       linsys_solver="pcg", scaling=10)
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    f = oq.interface._fptr

    def apply(op, v):
        out = np.zeros(n)
        assert product_lib.osqp_amd_apply(m.workspace, op, f(v), f(out)) == 0
        return out

    Ax, Aty, Px, Py = apply(0, x), apply(1, y), apply(2, x), apply(2, y)
    scale = np.linalg.norm(Ax) * np.linalg.norm(y)
    assert abs(y @ Ax - x @ Aty) <= 1e-12 * scale
    assert abs(x @ Py - y @ Px) <= 1e-12 * np.linalg.norm(Px) * np.linalg.norm(y)
    Axy = apply(0, 0.5 * x + y)
    assert np.max(np.abs(Axy - (0.5 * Ax + apply(0, y)))) <= 1e-11 * np.max(np.abs(Axy))
    r = oq.solve(m)
    assert r.info.status == "Solved" and r.info.iter <= 400
    assert np.all(np.isfinite(r.x)) and np.all(np.isfinite(r.y))
    oq.warm_start(m, x=r.x, y=r.y)
    r2 = oq.solve(m)
    assert r2.info.status == "Solved" and r2.info.iter <= 25
    assert abs(r2.info.obj_val - r.info.obj_val) <= 1e-3 * abs(r.info.obj_val)


def test_cleanup_releases_device_memory(product_lib):
    """osqp_cleanup frees everything the workspace owns in HBM (the Julia finalizer relies on it
    [REF src/interface.jl:24-25, 223-233]); repeated setup / cleanup does not accumulate."""
    base = None
    for rep in range(4):
        m = oq.Model(product_lib)
        oq.setup_generated(m, 0, 30000, 40, 1 + rep, verbose=False, linsys_solver="pcg")
        used = oq.stats(m)[9]
        assert used > 30000 * 40 * 12
        oq.solve(m)
        oq.clean(m)
        m2 = oq.Model(product_lib)
        oq.setup_generated(m2, 1, 1000, 0, 1, verbose=False)
        after = oq.stats(m2)[9]          # bytes held now = only the small model
        oq.clean(m2)
        if base is None:
            base = after
        assert after == base


def test_host_arrays_of_an_indirect_setup_are_narrowed_and_checked_on_the_device(product_lib, oracle_lib):
    """A setup that is certain to run the indirect back-end sends the caller's 64-bit index arrays to the device as they
    are and narrows them there (engine.hip, setup_host): the same solution as through the host-side conversion (the
    direct back-end's path, here forced by linsys_solver), and a row index outside the matrix is refused with error 1 as
    libosqp's validate_data does [REF src/interface.jl:147-153: a non-zero exit flag is an error]."""
    d = oracle_lib.oracle_generate(0, 3000, 30, 3)
    P, q, A, l, u = _data_to_scipy(d.contents)
    oracle_lib.oracle_data_free(d)
    opts = dict(verbose=False, eps_abs=1e-6, eps_rel=1e-6, adaptive_rho_interval=25)
    xs = {}
    for solver in ("pcg", "qdldl"):
        m = oq.Model(product_lib)
        oq.setup(m, P=P, q=q, A=A, l=l, u=u, linsys_solver=solver, **opts)
        r = oq.solve(m)
        assert r.info.status == "Solved"
        xs[solver] = r.x.copy()
        oq.clean(m)
    assert np.max(np.abs(xs["pcg"] - xs["qdldl"])) <= 1e-4 * max(1.0, np.max(np.abs(xs["qdldl"])))
    A2 = A.copy()
    A2.indices = A2.indices.copy()
    A2.indices[5] = A.shape[0] + 7
    m = oq.Model(product_lib)
    with pytest.raises(oq.OSQPError):
        oq.setup(m, P=P, q=q, A=A2, l=l, u=u, linsys_solver="pcg", **opts)


def test_polish_on_a_compact_workspace(product_lib, oracle_lib, monkeypatch):
    """Polish [REF test/polishing.jl:16-93] where no reduced KKT matrix can be assembled (a compact workspace has released
    its CSR arrays; round 3 reported status_polish = -1 there): the iterative form on the operator of the indirect back-end
    (csrc/pcg.hip polish_run_pcg) must succeed and improve both residuals as the acceptance rule demands.
    (a) a banded problem the CPU oracle can factorise: the polished solution is the oracle's (a factorisation of the same
    reduced system); (b) the random family of the headline workload, where no factorisation exists on either side: the
    polished point meets the optimality conditions orders of magnitude below the tolerance ADMM stopped at."""
    import qp_zoo

    monkeypatch.setenv("OSQP_AMD_PANEL", "2")
    monkeypatch.setenv("OSQP_AMD_COMPACT_NNZ", "0")
    monkeypatch.setenv("OSQP_AMD_POLISH_ITERATIVE", "1")  # (a) is too small for the panels: the iterative form is asked for by name
    opts = dict(verbose=False, eps_abs=1e-4, eps_rel=1e-4, adaptive_rho_interval=25, polish=True)
    prob = qp_zoo.control(nx=8, nu=4, T=120)
    mg = oq.Model(product_lib)
    oq.setup(mg, linsys_solver="pcg", **prob, **opts)
    rg = oq.solve(mg)
    mo = oq.Model(oracle_lib)
    oq.setup(mo, linsys_solver="qdldl", **prob, **opts)
    ro = oq.solve(mo)
    assert rg.info.status == ro.info.status == "Solved"
    assert ro.info.status_polish == 1
    assert rg.info.status_polish == 1, product_lib.osqp_amd_last_error()
    assert np.max(np.abs(rg.x - ro.x)) <= 1e-5 * max(1.0, np.max(np.abs(ro.x)))
    assert abs(rg.info.obj_val - ro.info.obj_val) <= 1e-6 * max(1.0, abs(ro.info.obj_val))
    assert rg.info.pri_res <= max(100.0 * ro.info.pri_res, 1e-7) and rg.info.dua_res <= max(100.0 * ro.info.dua_res, 1e-6)
    oq.clean(mg); oq.clean(mo)
    # (b)
    n, k = 20000, 48
    mg = oq.Model(product_lib)
    oq.setup_generated(mg, 0, n, k, 3, linsys_solver="pcg", **opts)
    assert oq.stats(mg)[18] == 1.0
    m0 = oq.Model(product_lib)
    oq.setup_generated(m0, 0, n, k, 3, linsys_solver="pcg", **dict(opts, polish=False))
    r0 = oq.solve(m0)
    rg = oq.solve(mg)
    assert rg.info.status == "Solved" and rg.info.status_polish == 1, product_lib.osqp_amd_last_error()
    assert rg.info.pri_res < 1e-3 * r0.info.pri_res + 1e-9 and rg.info.dua_res < 1e-3 * r0.info.dua_res + 1e-8
    assert rg.info.obj_val <= r0.info.obj_val + 1e-3 * abs(r0.info.obj_val)
    oq.clean(mg); oq.clean(m0)


@pytest.mark.parametrize("linsys", ["qdldl", "pcg"])
def test_unsorted_columns_of_A_are_accepted_as_libosqp_accepts_them(product_lib, linsys):
    """Boundary [REF src/interface.jl:132-155 hands csc arrays over verbatim]: libosqp takes the rows of a column of A in any
    order; until round 3 this library answered exit flag 1.  Now the setup is repeated on a sorted host copy and
    osqp_update_A translates the caller's nnz indices: the workspace built from shuffled columns gives bit for bit the
    results of the one built from sorted columns, before and after updates by index and in full."""
    rng = np.random.default_rng(11)
    n, m = 60, 90
    A = sp.random(m, n, density=0.15, random_state=rng, data_rvs=rng.standard_normal, format="csc")
    A.sort_indices()
    M = sp.random(n, n, density=0.1, random_state=rng, data_rvs=rng.standard_normal)
    P = sp.triu(M @ M.T + 0.1 * sp.eye(n), format="csc")
    q = rng.standard_normal(n)
    l, u = -rng.random(m), rng.random(m)
    # the same matrix with the entries of every column in a random order, and where each sorted entry went
    perm = np.concatenate([A.indptr[j] + rng.permutation(A.indptr[j + 1] - A.indptr[j]) for j in range(n)])
    Ash = sp.csc_matrix((A.data[perm], A.indices[perm], A.indptr.copy()), shape=A.shape)
    assert not Ash.has_sorted_indices
    pos_of_sorted = np.empty_like(perm)
    pos_of_sorted[perm] = np.arange(len(perm))  # shuffled position of sorted entry k
    opts = dict(verbose=False, eps_abs=1e-7, eps_rel=1e-7, adaptive_rho_interval=25, max_iter=8000, linsys_solver=linsys)
    ms, mu = oq.Model(product_lib), oq.Model(product_lib)
    oq.setup(ms, P=P, q=q, A=A, l=l, u=u, **opts)
    oq.setup(mu, P=P, q=q, A=Ash, l=l, u=u, keep_A_order=True, **opts)
    rs, ru = oq.solve(ms), oq.solve(mu)
    assert rs.info.status == ru.info.status == "Solved" and rs.info.iter == ru.info.iter
    assert np.array_equal(rs.x, ru.x) and np.array_equal(rs.y, ru.y)
    # by index: sorted entries k get new values; the same entries in the caller's (shuffled) numbering
    k = rng.choice(A.nnz, size=40, replace=False).astype(np.int64)
    newv = rng.standard_normal(40)
    oq.update_A(ms, newv, k)
    oq.update_A(mu, newv, pos_of_sorted[k].astype(np.int64))
    rs, ru = oq.solve(ms), oq.solve(mu)
    assert rs.info.status == ru.info.status and rs.info.iter == ru.info.iter and np.array_equal(rs.x, ru.x)
    # in full: values in each model's own entry order
    full = A.data * 1.3
    oq.update_A(ms, full, None)
    oq.update_A(mu, full[perm], None)
    rs, ru = oq.solve(ms), oq.solve(mu)
    assert rs.info.status == ru.info.status and rs.info.iter == ru.info.iter and np.array_equal(rs.x, ru.x)
    # a column that holds a row twice stays refused
    dup = sp.csc_matrix((np.array([1.0, 2.0, 3.0]), np.array([1, 0, 1]), np.array([0, 3] + [3] * (n - 1))), shape=(m, n))
    md = oq.Model(product_lib)
    with pytest.raises(oq.OSQPError):
        oq.setup(md, P=P, q=q, A=dup, l=l, u=u, keep_A_order=True, **opts)
    oq.clean(ms); oq.clean(mu)
