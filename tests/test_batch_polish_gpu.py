"""Solution polishing on the resident batch (settings.polish = 1: k_batch_polish after the ADMM launch;
`ResidentBatch.polish_status` / `update_polish`) on the GPU.  The reference of every instance is ONE oracle model with
polish = True driven through the same calls (batch_resident_ref.OracleBatch).

Tolerance on polished x / y (instances accepted on both sides), relative to max(1, max|ref|): ten times the largest
difference measured on the MI355X over all families, rounded up to a power of ten, and never above 1e-6 (polished and
unpolished solutions differ by ~1e-4, so anything looser would no longer show that polish ran).
FIGURES: NOT YET MEASURED ON THE MI355X -- this file was written without access to a device; TOL stands at the cap, 1e-6.
What is known: the kernel's source executed on the CPU (one thread per work-item, barriers for the workgroup's) against the
oracle, largest value over the three variants -- mpc x 1.4e-15 y 1.5e-15, quad64 x 4.8e-13 y 3.3e-11, rows300 x 2.1e-16
y 1.7e-8; ten times the largest rounds up to 1e-6.  The first test prints the figures of a run; whoever runs it on a device
replaces this paragraph with them and lowers TOL if they allow.  rows300 is a shape / path case (its polished and
unpolished x differ by ~1e-9); its multipliers are fixed only through the delta-regularisation (more active rows than
variables), which is where the largest y figure comes from -- the numpy model of the same algebra shows the same 1.9e-8
against the oracle (tests/test_batch_polish_host.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

import osqp_jl_amd as oq
from osqp_jl_amd import batch
import batch_resident_ref as ref
from batch_resident_ref import OPTS
from test_batch_gpu import _family

pytestmark = pytest.mark.gpu

TOL = 1e-6
VARIANTS = [dict(), dict(scaling=0), dict(scaled_termination=1)]
EPS = float(np.finfo(float).eps)


def _problem(oracle_lib, family, monkeypatch):
    """(probs, kernel the launcher must report, status mismatches with the oracle the family may show)."""
    if family in ("mpc", "mpc512"):
        if family == "mpc512":
            monkeypatch.setenv("OSQP_AMD_BATCH_QUAD", "0")
        return ref.mpc_instances(oracle_lib, 0, 64, 2), (0 if family == "mpc" else -1), 1
    if family == "quad64":
        return _family(64, 100, 6, 640100)[1], 1, 0
    return _family(40, 300, 5, 40300)[1], -1, 0


def _check_kernel(lib, kernel):
    got = lib.osqp_amd_batch_last_kernel()
    assert (got >= 1) if kernel == 1 else (got == kernel), (got, kernel)


def _rel(a, b):
    return float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(b)))) if len(b) else 0.0


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _oracle_polished(oracle_lib, probs, opts):
    ob = ref.OracleBatch(oracle_lib, probs, **dict(opts, polish=True))
    refs = ob.solve()
    ob.close()
    return refs


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("family", ["mpc", "mpc512", "quad64", "rows300"])
def test_polished_batch_follows_the_oracle(product_lib, oracle_lib, monkeypatch, family, variant):
    """status_polish equals the oracle's (on all but at most one of the 64 MPC instances; on every instance of the small
    families), at least 20 MPC instances are accepted on both sides, accepted instances agree in x / y within TOL, and what
    the oracle refuses (or does not polish) comes back bit-identical to a polish = 0 solve of the same handle state."""
    opts = dict(OPTS, **VARIANTS[variant])
    probs, kernel, allowed = _problem(oracle_lib, family, monkeypatch)
    args = ref.stack(probs)
    rb = batch.ResidentBatch(product_lib, *args, **dict(opts, polish=True))
    assert np.all(rb.polish_status() == 0)  # before any solve
    x, y, info = rb.solve()
    _check_kernel(product_lib, kernel)
    st = rb.polish_status()
    rb.close()
    plain = batch.ResidentBatch(product_lib, *args, **opts)
    x0, y0, info0 = plain.solve()
    assert np.all(plain.polish_status() == 0)
    plain.close()
    refs = _oracle_polished(oracle_lib, probs, opts)
    rst = np.array([r.info.status_polish for r in refs])
    both = [i for i in range(len(refs)) if st[i] == 1 and rst[i] == 1]
    ex = max([_rel(x[i], refs[i].x) for i in both], default=0.0)
    ey = max([_rel(y[i], refs[i].y) for i in both], default=0.0)
    moved = max([_rel(x[i], x0[i]) for i in both], default=0.0)
    differ = np.flatnonzero(st != rst)
    print(f"{family}/{variant}: Solved {int(np.sum(info[:, 1] == 1))} of {len(refs)}, accepted gpu {int(np.sum(st == 1))} oracle "
          f"{int(np.sum(rst == 1))} both {len(both)}, statuses differ at {differ.tolist()}, polished vs oracle rel dx {ex:.2e} dy {ey:.2e}, "
          f"polished vs unpolished rel dx {moved:.2e}, max polished residuals {max([max(info[i, 2], info[i, 3]) for i in both], default=0):.2e}")
    assert np.array_equal(info[:, 1], [r.info.status_val for r in refs])
    assert np.array_equal(info[:, [0, 1, 5]], info0[:, [0, 1, 5]])  # iter, status, rho_updates: the solve's
    assert len(differ) <= allowed, (differ, st[differ], rst[differ])
    assert len(both) >= (20 if family in ("mpc", "mpc512") else 5)
    assert ex <= TOL and ey <= TOL, (ex, ey)
    for i in range(len(refs)):
        if rst[i] != 1 and st[i] == rst[i]:
            assert _same(x[i], x0[i]) and _same(y[i], y0[i]) and _same(info[i], info0[i]), (family, i)
        if st[i] == 1:
            assert info[i, 2] < info0[i, 2] or info[i, 3] < info0[i, 3]


@pytest.mark.parametrize("family", ["mpc", "quad64"])
def test_accepted_polish_is_a_better_solution_of_the_raw_problem(product_lib, oracle_lib, monkeypatch, family):
    """For every accepted instance, from the RAW data in numpy (scaled_termination = 0: the unscaled definitions):
    |Ax - clamp(Ax, l, u)|_inf and |Px + q + A'y|_inf agree with info columns 2 and 3, the objective with column 4, and both
    residuals are smaller than what the polish = 0 solve of the instance returns.
    Agreement: the kernel evaluates the same sums on the scaled data (another order of rounding), and its primal residual
    is against z = clamp(Ax + y), which is clamp(Ax) up to rounding at a polished point.  Each entry of a residual is a
    sum of k <= (longest row of [P A'] or A) + 2 products of magnitude <= S = max|entry| max(1, |x|, |y|), evaluated twice,
    undone by factors D, E, c within [1e-4, 1e4] that cancel up to a rounding each: |difference| <= 16 (k + 8) eps S."""
    probs, kernel, _ = _problem(oracle_lib, family, monkeypatch)
    args = ref.stack(probs)
    rb = batch.ResidentBatch(product_lib, *args, **dict(OPTS, polish=True))
    x, y, info = rb.solve()
    st = rb.polish_status()
    rb.close()
    plain = batch.ResidentBatch(product_lib, *args, **OPTS)
    _, _, info0 = plain.solve()
    plain.close()
    accepted = np.flatnonzero(st == 1)
    assert len(accepted) >= (20 if family == "mpc" else 5)
    worst = [0.0, 0.0, 0.0]
    for i in accepted:
        P, q, A, l, u = probs[i]
        U = sp.triu(sp.csc_matrix(P), format="csc")  # the families hand P over as its upper triangle
        P, A = (U + sp.triu(U, 1).T).tocsr(), A.tocsr()
        ax = A @ x[i]
        pri = float(np.max(np.abs(ax - np.clip(ax, l, u))))
        dua = float(np.max(np.abs(P @ x[i] + q + A.T @ y[i])))
        obj = float(0.5 * x[i] @ (P @ x[i]) + q @ x[i])
        k = int(max(np.max(np.diff(A.indptr)), np.max(np.diff(P.indptr)) + np.max(np.diff(A.tocsc().indptr)))) + 2
        S = max(float(np.max(np.abs(A.data))), float(np.max(np.abs(P.data))), float(np.max(np.abs(q)))) * max(1.0, float(np.max(np.abs(x[i]))), float(np.max(np.abs(y[i]))))
        bound = 16 * (k + 8) * EPS * S
        worst = [max(worst[0], abs(pri - info[i, 2]) / bound), max(worst[1], abs(dua - info[i, 3]) / bound),
                 max(worst[2], abs(obj - info[i, 4]) / (bound * len(q) * max(1.0, float(np.max(np.abs(x[i]))))))]
        print(f"{family} inst {i}: pri {pri:.2e}/{info[i, 2]:.2e} (unpolished {info0[i, 2]:.2e}) dua {dua:.2e}/{info[i, 3]:.2e} "
              f"(unpolished {info0[i, 3]:.2e}) obj {obj:.12e}/{info[i, 4]:.12e} bound {bound:.1e}")
        assert abs(pri - info[i, 2]) <= bound and abs(dua - info[i, 3]) <= bound, (i, pri, dua, info[i])
        assert abs(obj - info[i, 4]) <= bound * len(q) * max(1.0, float(np.max(np.abs(x[i]))))  # n terms x_j (.)_j
        assert pri < info0[i, 2] and dua < info0[i, 3] and info[i, 2] < info0[i, 2] and info[i, 3] < info0[i, 3]
    print(f"{family}: largest |difference| / bound: pri {worst[0]:.2e} dua {worst[1]:.2e} obj {worst[2]:.2e}")


def test_instances_without_a_solution_are_left_alone(product_lib, oracle_lib):
    """16 MPC instances, max_iter = 100; instances 1, 5, 9 made primal infeasible by an update of the bounds (the first
    state of the horizon pinned at 1000 against the dynamics).  Some of the rest run into max_iter, the others are Solved:
    the not-Solved rows have status_polish 0 and x (NaN for the infeasible ones), y, info bit-identical to the polish = 0
    run; the Solved instances of the same launch are polished as the oracle polishes them."""
    opts = dict(OPTS, max_iter=100)
    probs = ref.mpc_instances(oracle_lib, 0, 16, 2)
    args = ref.stack(probs)
    l2, u2 = args[5].copy(), args[6].copy()
    for i in (1, 5, 9):
        l2[i, 60] = u2[i, 60] = 1000.0
    out = []
    for polish in (True, False):
        rb = batch.ResidentBatch(product_lib, *args, **dict(opts, polish=polish))
        rb.update(l=l2, u=u2)
        out.append(rb.solve() + (rb.polish_status(),))
        rb.close()
    (x, y, info, st), (x0, y0, info0, st0) = out
    ob = ref.OracleBatch(oracle_lib, probs, **dict(opts, polish=True))
    ob.update(l=l2, u=u2)
    refs = ob.solve()
    ob.close()
    rst = np.array([r.info.status_polish for r in refs])
    print("status", info[:, 1], "status_polish gpu", st, "oracle", rst)
    assert np.array_equal(info[:, 1], [r.info.status_val for r in refs])
    assert np.all(info[[1, 5, 9], 1] == -3) and np.sum(info[:, 1] == -2) >= 1 and np.sum(info[:, 1] == 1) >= 4
    assert np.all(st0 == 0)
    assert np.array_equal(st, rst) and np.sum(st == 1) >= 2
    for i in np.flatnonzero(info[:, 1] != 1):
        assert st[i] == 0 and _same(x[i], x0[i]) and _same(y[i], y0[i]) and _same(info[i], info0[i]), i
    assert np.all(np.isnan(x[[1, 5, 9]]))
    for i in np.flatnonzero(st == 1):
        assert _rel(x[i], refs[i].x) <= TOL and _rel(y[i], refs[i].y) <= TOL, i


def test_life_cycle_of_a_polishing_handle(product_lib, oracle_lib):
    """(a) A warm re-solve after an accepted polish starts from the polished iterate, as the oracle's does: on MPC instance
    0 (seed 2) the second solve stops at iteration 25, is accepted again and returns the same x.  (b) update_polish(0):
    bit-identical to a handle set up without polish, all statuses 0; update_polish(1, 5) polishes again, with five
    refinement steps, as the oracle after update_settings.  (c) solve(out = device arrays) and polish_status into a device
    array give the numbers of the host form."""
    probs = ref.mpc_instances(oracle_lib, 0, 8, 2)
    args = ref.stack(probs)
    rb = batch.ResidentBatch(product_lib, *args, **dict(OPTS, polish=True))
    ob = ref.OracleBatch(oracle_lib, probs, **dict(OPTS, polish=True))
    first, rfirst = rb.solve() + (rb.polish_status(),), ob.solve()
    second, rsecond = rb.solve() + (rb.polish_status(),), ob.solve()
    ob.close()
    for tag, (x, y, info, st), refs in (("first", first, rfirst), ("second", second, rsecond)):
        rst = np.array([r.info.status_polish for r in refs])
        print(tag, "iter", info[:, 0], [r.info.iter for r in refs], "status_polish", st, rst)
        ref.compare(x, y, info, refs, OPTS, tag=tag)
        assert np.array_equal(st, rst)
        for i in np.flatnonzero(st == 1):
            assert _rel(x[i], refs[i].x) <= TOL and _rel(y[i], refs[i].y) <= TOL, (tag, i)
    assert rfirst[0].info.status_polish == 1 and rsecond[0].info.status_polish == 1 and rsecond[0].info.iter == 25
    assert second[2][0, 0] == 25 and second[3][0] == 1
    assert _rel(second[0][0], first[0][0]) <= TOL and _rel(rsecond[0].x, rfirst[0].x) <= TOL
    # (c) on the same state: a twin handle taken through the same two solves, results left on the device
    twin = batch.ResidentBatch(product_lib, *args, **dict(OPTS, polish=True))
    dev = twin.alloc()
    dst = batch.DeviceArray(product_lib, twin.count, 1)
    twin.solve(out=dev)
    twin.solve(out=dev)
    twin.polish_status(out=dst)
    assert _same(dev[0].numpy(), second[0]) and _same(dev[1].numpy(), second[1]) and _same(dev[2].numpy(), second[2])
    assert np.array_equal(dst.numpy().ravel(), second[3])
    twin.close()
    for d in dev + (dst,):
        d.free()
    rb.close()
    # (b)
    a = batch.ResidentBatch(product_lib, *args, **dict(OPTS, polish=True))
    b = batch.ResidentBatch(product_lib, *args, **OPTS)
    a.update_polish(0)
    for _ in range(2):
        ra, rb0 = a.solve(), b.solve()
        assert all(_same(p, q) for p, q in zip(ra, rb0))
        assert np.all(a.polish_status() == 0)
    # the library's own refusals (past the Python checks): return 1, a message, the handle unchanged -- still not polishing
    assert product_lib.osqp_amd_batch_update_polish(a.handle, 2, 3) == 1 and b"polish" in product_lib.osqp_amd_last_error()
    assert product_lib.osqp_amd_batch_update_polish(a.handle, 1, -1) == 1 and b"polish_refine_iter" in product_lib.osqp_amd_last_error()
    assert all(_same(p, q) for p, q in zip(a.solve(), b.solve())) and np.all(a.polish_status() == 0)
    mpc_handle = batch.MpcBatch(product_lib, 4, seed=2, **OPTS)  # the other family's handle is refused by both calls
    buf = np.zeros(4)
    assert product_lib.osqp_amd_batch_polish_status(mpc_handle.handle, buf.ctypes.data, 0) == 1
    assert product_lib.osqp_amd_batch_update_polish(mpc_handle.handle, 1, 3) == 1
    mpc_handle.close()
    a.update_polish(1, 5)
    xa, ya, ia = a.solve()
    sa = a.polish_status()
    ob = ref.OracleBatch(oracle_lib, probs, **OPTS)
    ob.solve(); ob.solve()
    for m in ob.models:
        oq.update_settings(m, polish=True, polish_refine_iter=5)
    refs = ob.solve()
    ob.close()
    rst = np.array([r.info.status_polish for r in refs])
    print("after update_polish(1, 5): status_polish", sa, rst, "iter", ia[:, 0])
    assert np.array_equal(sa, rst) and np.sum(sa == 1) >= 1
    for i in np.flatnonzero(sa == 1):
        assert _rel(xa[i], refs[i].x) <= TOL and _rel(ya[i], refs[i].y) <= TOL, i
    xb, yb, ib = b.solve()
    for i in np.flatnonzero(sa != 1):
        assert _same(xa[i], xb[i]) and _same(ya[i], yb[i]) and _same(ia[i], ib[i]), i
    a.close(); b.close()


def test_polish_off_is_the_parents_launch_sequence(product_lib, oracle_lib):
    """With polish = 0 a resolve launches what it launched before polish existed: the solve kernel (whose device code is
    the parent's, instruction for instruction: DESIGN.md 12.1) and nothing else.  The library counts its polish launches
    (osqp_amd_batch_polish_launches): none for a handle without polish and for one switched off by update_polish(0), one
    per resolve with polish = 1 -- and the handle that never polished and the one switched off agree bit for bit in x, y,
    info over two consecutive solves (the second starts from the records the first left)."""
    probs = ref.mpc_instances(oracle_lib, 0, 8, 2)
    args = ref.stack(probs)
    off = batch.ResidentBatch(product_lib, *args, **OPTS)
    on = batch.ResidentBatch(product_lib, *args, **dict(OPTS, polish=True))
    n0 = product_lib.osqp_amd_batch_polish_launches()
    first, second = off.solve(), off.solve()
    assert product_lib.osqp_amd_batch_polish_launches() == n0 and np.all(off.polish_status() == 0)
    on.solve()
    assert product_lib.osqp_amd_batch_polish_launches() == n0 + 1
    on.close()
    switched = batch.ResidentBatch(product_lib, *args, **dict(OPTS, polish=True))
    switched.update_polish(0)
    for want in (first, second):
        got = switched.solve()
        assert all(_same(a, b) for a, b in zip(got, want))
    assert product_lib.osqp_amd_batch_polish_launches() == n0 + 1
    off.close(); switched.close()
