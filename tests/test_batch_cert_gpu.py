"""Infeasibility certificates of the resident batch (`ResidentBatch.certificates`, osqp_amd_batch_certificates) on the GPU.
The families and the criteria checker are those of tests/batch_cert_cases.py (held to the oracle, without a GPU, by
tests/test_batch_cert_host.py); the reference of every instance is one oracle model given the same data and settings.

Three kinds of check.  (a) Statuses, NaN rows and the criteria a certificate has to meet by definition, from the raw data
in numpy with derived rounding slacks: these hold whatever iterate the kernel stopped at.  (b) Agreement with the oracle's
certificate, on the instances whose iteration count equals the oracle's (one check apart the two sides stopped at different
iterates and are not comparable); at least three quarters of the infeasible instances of every case must be compared.
(c) That nothing else moved: records, one-shot entries, launch counts.

Tolerance of (b), max|v - v_ref| with both normalised to max|v| = 1: ten times the largest difference measured on the
MI355X over all cases and variants, rounded up to a power of ten.
FIGURES (MI355X, the first test prints them; profiles/batch_cert_device_figures.md): every infeasible instance of every case stopped
at the oracle's iteration and was compared (5 of 5 on mpc / mpc512, 4 of 4 on the chains).  Largest difference per case
over the variants {}, {scaling: 0}, {scaled_termination: 1}:
    mpc       5.4e-13  1.8e-13  5.7e-13        chain12   1.3e-14  9.0e-15  1.6e-14
    mpc512    9.4e-13  1.2e-13  1.0e-12        chain33   1.6e-14  2.1e-14  2.4e-14
                                               chain40d  3.1e-14  2.7e-14  3.5e-14
The largest is 9.996e-13 (mpc512, scaled_termination = 1); ten times that, rounded up to a power of ten: TOL = 1e-11."""
import numpy as np
import pytest

from osqp_jl_amd import batch
import batch_cert_cases as cases
import batch_resident_ref as ref

pytestmark = pytest.mark.gpu

TOL = 1e-11

# name -> (problems, OSQP_AMD_BATCH_QUAD, kernel osqp_amd_batch_last_kernel must report: 1 stands for "a table entry >= 1")
CASES = {
    "mpc": (lambda lib: cases.mpc(lib, 8), None, 0),
    "mpc512": (lambda lib: cases.mpc(lib, 8), "0", -1),
    "chain12": (lambda lib: cases.chain(12, 6), None, 1),
    "chain33": (lambda lib: cases.chain(33, 17), None, 1),
    "chain40d": (lambda lib: cases.chain(40, 20, True), None, -1),  # its 40-entry row exceeds every table entry's bound
}
_refs = {}


def _case(oracle_lib, monkeypatch, name, opts):
    """(problems, oracle results -- computed once per (case, settings) and shared --, wanted kernel)"""
    make, quad, kernel = CASES[name]
    if quad is not None:
        monkeypatch.setenv("OSQP_AMD_BATCH_QUAD", quad)
    key = (name.replace("512", ""), tuple(sorted(opts.items())))
    if key not in _refs:
        probs = make(oracle_lib)
        _refs[key] = (probs, ref.cold_oracle(oracle_lib, probs, **opts))
    return _refs[key] + (kernel,)


def _check_kernel(lib, kernel):
    got = lib.osqp_amd_batch_last_kernel()
    assert (got >= 1) if kernel == 1 else (got == kernel), (got, kernel)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _check_rows(info, x, y, p, d, tag):
    """Finite certificate rows where the status names them, NaN everywhere else -- x and y of infeasible instances included."""
    for i in range(len(info)):
        st = int(info[i, 1])
        assert np.all(np.isfinite(p[i])) == (st in cases.PRIM) and (st in cases.PRIM or np.all(np.isnan(p[i]))), (tag, i, st)
        assert np.all(np.isfinite(d[i])) == (st in cases.DUAL) and (st in cases.DUAL or np.all(np.isnan(d[i]))), (tag, i, st)
        if st in cases.PRIM + cases.DUAL:
            assert np.all(np.isnan(x[i])) and np.all(np.isnan(y[i])), (tag, i)


@pytest.mark.parametrize("variant", range(len(cases.VARIANTS)))
@pytest.mark.parametrize("name", list(CASES))
def test_certificates_follow_the_oracle(product_lib, oracle_lib, monkeypatch, name, variant):
    opts = dict(cases.OPTS, **cases.VARIANTS[variant])
    probs, refs, kernel = _case(oracle_lib, monkeypatch, name, opts)
    rb = batch.ResidentBatch(product_lib, *cases.stack(probs), **opts)
    x, y, info = rb.solve()
    _check_kernel(product_lib, kernel)
    p, d = rb.certificates()
    # the device form: the same values
    dp, dd = batch.DeviceArray(product_lib, rb.count, rb.m), batch.DeviceArray(product_lib, rb.count, rb.n)
    got = rb.certificates(out=(dp, dd))
    assert got[0] is dp and got[1] is dd and _same(dp.numpy(), p) and _same(dd.numpy(), d)
    dd.upload(np.zeros((rb.count, rb.n)))
    rb.certificates(out=(None, dd))  # one alone
    assert _same(dd.numpy(), d)
    dp.free(); dd.free()
    rb.close()
    tag = f"{name}/{variant}"
    ref.compare(x, y, info, refs, opts, tag=tag)
    assert [int(s) for s in info[:, 1]] == [{0: 1, 1: -3, 2: -4}[cases.kind(i)] for i in range(len(probs))]
    _check_rows(info, x, y, p, d, tag)
    infeasible = [i for i in range(len(probs)) if cases.kind(i)]
    for i in infeasible:
        v = p[i] if cases.kind(i) == 1 else d[i]
        assert float(np.max(np.abs(v))) == 1.0, (tag, i)
        if not opts.get("scaled_termination", 0):
            cases.check_certificate(int(info[i, 1]), p[i], d[i], probs[i], opts, tag=f"{tag}/{i}")
    compared, worst = 0, 0.0
    for i in infeasible:
        if int(info[i, 0]) != refs[i].info.iter:
            print(f"{tag} inst {i}: iter {int(info[i, 0])} / oracle {refs[i].info.iter}: not compared")
            continue
        compared += 1
        v, w = (p[i], refs[i].prim_inf_cert) if cases.kind(i) == 1 else (d[i], refs[i].dual_inf_cert)
        err = float(np.max(np.abs(v - w)))
        worst = max(worst, err)
        print(f"{tag} inst {i}: status {int(info[i, 1])} iter {int(info[i, 0])} max|v - v_ref| {err:.3e}")
    print(f"{tag}: compared {compared} of {len(infeasible)} infeasible instances, FIGURE max|v - v_ref| = {worst:.3e}")
    assert 4 * compared >= 3 * len(infeasible), (tag, compared, len(infeasible))
    assert worst <= TOL, (tag, worst)


def _mpc_two_data_sets(oracle_lib):
    """The plain MPC family (every instance solvable), and its bounds with instance 1 made primal infeasible."""
    probs = ref.mpc_instances(oracle_lib, 0, 8, 2)
    args = ref.stack(probs)
    l2, u2 = args[5].copy(), args[6].copy()
    l2[1, 60] = u2[1, 60] = 1000.0
    return args, l2, u2


def test_nothing_else_moved(product_lib, oracle_lib):
    """Handle A: solve, certificates, update (instance 1 becomes infeasible), solve, certificates, solve.  Handle B: the same
    without ever calling certificates().  Every solve of A is bit-identical to B's in x, y, info -- the third, which follows
    the infeasible one and starts instance 1 from its record, in particular: k_batch_cert put the record back.  The
    one-shot entry agrees in status and iteration count wherever both start from the same state: with A's first solve on
    the first data set, and, on the second data set, with the first solve of a handle set up on it (A's own second solve
    starts warm, with adapted rho, which the one-shot entry cannot).  k_batch_cert is launched once per resolve and by
    nothing else."""
    args, l2, u2 = _mpc_two_data_sets(oracle_lib)
    opts = cases.OPTS
    count = product_lib.osqp_amd_batch_cert_launches
    A, B = batch.ResidentBatch(product_lib, *args, **opts), batch.ResidentBatch(product_lib, *args, **opts)
    n0 = count()
    a1 = A.solve()
    assert count() == n0 + 1
    p1, d1 = A.certificates()
    assert count() == n0 + 1
    assert np.all(a1[2][:, 1] == 1) and np.all(np.isnan(p1)) and np.all(np.isnan(d1))
    A.update(l=l2, u=u2)
    a2 = A.solve()
    p2, d2 = A.certificates()
    assert count() == n0 + 2
    assert a2[2][1, 1] == -3 and np.all(np.isfinite(p2[1])) and np.all(np.isnan(np.delete(p2, 1, axis=0))) and np.all(np.isnan(d2))
    cases.check_primal(p2[1], (None, None, sp_A(args, 1), l2[1], u2[1]), 1e-4, tag="A/second")
    a3 = A.solve()
    A.certificates()
    b1 = B.solve()
    B.update(l=l2, u=u2)
    b2, b3 = B.solve(), B.solve()
    assert count() == n0 + 6
    for k, (a, b) in enumerate(((a1, b1), (a2, b2), (a3, b3))):
        assert all(_same(s, t) for s, t in zip(a, b)), k
    A.close(); B.close()
    n1 = count()
    x, y, info = batch.solve_batch(product_lib, *args, **opts)
    assert np.array_equal(info[:, :2], a1[2][:, :2])
    args2 = args[:5] + (l2, u2)
    x, y, info = batch.solve_batch(product_lib, *args2, **opts)
    assert count() == n1  # the one-shot entries launch no certificate kernel
    D = batch.ResidentBatch(product_lib, *args2, **opts)
    xd, yd, infod = D.solve()
    pd, _ = D.certificates()
    D.close()
    assert np.array_equal(info[:, :2], infod[:, :2]) and info[1, 1] == -3 and np.all(np.isfinite(pd[1]))
    assert np.array_equal(info[:, 1], a2[2][:, 1])


def sp_A(args, i):
    """A of instance i of a stacked family as a scipy matrix."""
    A = args[1].copy()
    A.data = np.array(args[3][i], dtype=float)
    return A


def test_the_inaccurate_case(product_lib, oracle_lib, monkeypatch):
    """chain(33, 17) with max_iter = 50: the instance of seed 104 stops at the limit with status 3
    (Primal_infeasible_inaccurate); its certificate passes the checker with 10 eps."""
    opts = dict(cases.OPTS, max_iter=50)
    probs, refs, kernel = _case(oracle_lib, monkeypatch, "chain33", opts)
    rb = batch.ResidentBatch(product_lib, *cases.stack(probs), **opts)
    x, y, info = rb.solve()
    _check_kernel(product_lib, kernel)
    p, d = rb.certificates()
    rb.close()
    ref.compare(x, y, info, refs, opts, tag="chain33/max_iter50")
    assert refs[4].info.status_val == 3 and info[4, 1] == 3 and info[4, 0] == 50
    _check_rows(info, x, y, p, d, "chain33/max_iter50")
    assert float(np.max(np.abs(p[4]))) == 1.0
    cases.check_certificate(3, p[4], d[4], probs[4], opts, tag="chain33/max_iter50/4")


@pytest.mark.parametrize("name", ["mpc", "mpc512"])
def test_the_inaccurate_case_of_the_mpc_family(product_lib, oracle_lib, monkeypatch, name):
    """mpc with max_iter = 25: the primal infeasible members 1 and 4 stop at the limit with status 3.  The 512-thread kernel
    takes the status of its certificate store from LDS, not from a register: this is its run with an inaccurate one."""
    opts = dict(cases.OPTS, max_iter=25)
    probs, refs, kernel = _case(oracle_lib, monkeypatch, name, opts)
    rb = batch.ResidentBatch(product_lib, *cases.stack(probs), **opts)
    x, y, info = rb.solve()
    _check_kernel(product_lib, kernel)
    p, d = rb.certificates()
    rb.close()
    tag = f"{name}/max_iter25"
    ref.compare(x, y, info, refs, opts, tag=tag)
    _check_rows(info, x, y, p, d, tag)
    for i in (1, 4):
        assert refs[i].info.status_val == 3 and info[i, 1] == 3 and info[i, 0] == 25, (tag, i)
        assert float(np.max(np.abs(p[i]))) == 1.0
        cases.check_certificate(3, p[i], d[i], probs[i], opts, tag=f"{tag}/{i}")


def test_certificates_are_results_of_the_last_resolve(product_lib, oracle_lib):
    """All rows NaN before any resolve; after update(q = ...) without a resolve the previous certificates are still returned,
    in both forms; the next resolve replaces them."""
    probs = cases.chain(12, 6)
    args = cases.stack(probs)
    rb = batch.ResidentBatch(product_lib, *args, **cases.OPTS)
    p0, d0 = rb.certificates()
    assert p0.shape == (6, 18) and d0.shape == (6, 12) and np.all(np.isnan(p0)) and np.all(np.isnan(d0))
    dp = batch.DeviceArray(product_lib, 6, 18).upload(np.zeros((6, 18)))
    rb.certificates(out=(dp, None))
    assert np.all(np.isnan(dp.numpy()))
    rb.solve()
    p1, d1 = rb.certificates()
    assert np.all(np.isfinite(p1[[1, 4]])) and np.all(np.isfinite(d1[[2, 5]]))
    rb.update(q=args[4] * 1.5)
    rb.warm_start(x=np.zeros((6, 12)))
    p2, d2 = rb.certificates()
    rb.certificates(out=(dp, None))
    assert _same(p1, p2) and _same(d1, d2) and _same(dp.numpy(), p1)
    # every instance made solvable: the next resolve leaves no certificate
    l, u = -np.ones((6, 18)), np.ones((6, 18))
    Px = np.array([probs[0][0].data] * 6)
    rb.update(l=l, u=u, Px=Px, q=args[4])
    x, y, info = rb.solve()
    p3, d3 = rb.certificates()
    assert np.all(info[:, 1] == 1) and np.all(np.isnan(p3)) and np.all(np.isnan(d3))
    # the library's own refusals: nothing asked for, and the other family's handle
    assert product_lib.osqp_amd_batch_certificates(rb.handle, None, None, 0) == 1
    mpc_handle = batch.MpcBatch(product_lib, 4, seed=2, **cases.OPTS)
    buf = np.zeros((4, 200))
    assert product_lib.osqp_amd_batch_certificates(mpc_handle.handle, buf.ctypes.data, None, 0) == 1
    assert b"osqp_amd_batch_setup" in product_lib.osqp_amd_last_error()
    mpc_handle.close()
    dp.free()
    rb.close()
