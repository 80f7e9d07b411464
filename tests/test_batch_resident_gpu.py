"""The resident batch (osqp_amd_batch_setup / _update_* / _warm_start / _resolve; batch.ResidentBatch) on the GPU.  The
reference of every instance is ONE oracle model driven through the same sequence of calls (batch_resident_ref.OracleBatch),
under the tolerances tests/test_batch_gpu.py uses between the batched kernels and the oracle (batch_resident_ref.compare)."""
import numpy as np
import pytest

import osqp_jl_amd as oq
from osqp_jl_amd import batch
import batch_resident_ref as ref
from batch_resident_ref import OPTS
from test_batch_gpu import _family

pytestmark = pytest.mark.gpu


def _problem(oracle_lib, family, monkeypatch=None):
    """(probs, kernel the launcher must report, rows that are boxes and stay feasible as equalities at their midpoint)."""
    if family in ("mpc", "mpc512"):
        probs = ref.mpc_instances(oracle_lib, 0, 8, 2)  # instance 2 of seed 2: the one whose scaling shows (see below)
        if family == "mpc512":
            monkeypatch.setenv("OSQP_AMD_BATCH_QUAD", "0")
        return probs, (0 if family == "mpc" else -1), [66, 67, 68, 69]  # the inputs of the first stage
    if family == "quad64":
        _, probs = _family(64, 100, 6, 640100)
        kernel = 1
    else:  # more than 256 rows: the schedule of the four-wavefront kernel refuses, the 512-thread kernel takes it
        _, probs = _family(40, 300, 5, 40300)
        kernel = -1
    boxes = [i for i in range(len(probs[0][3])) if all(p[4][i] - p[3][i] > 1e-2 for p in probs)][:4]
    return probs, kernel, boxes


def _check_kernel(lib, kernel):
    got = lib.osqp_amd_batch_last_kernel()
    assert (got >= 1) if kernel == 1 else (got == kernel), (got, kernel)


FAMILIES = ["mpc", "quad64", "rows300", "mpc512"]


def test_first_solve_is_the_one_shot_path(product_lib, oracle_lib):
    """A handle's first solve against batch.solve_batch on the same data.  The handle applies the factors its setup stored
    in one pass (P <- c D P D, ...) where the one-shot path scales pass by pass, so the data differ in the last bits:
    status equal, iterations within one check, x / y within the tolerance of the file -- not bit-equality."""
    for probs, kernel in ((ref.mpc_instances(oracle_lib, 0, 12, 5), 0), (_family(64, 100, 6, 640100)[1], 1)):
        args = ref.stack(probs)
        rb = batch.ResidentBatch(product_lib, *args, **OPTS)
        x, y, info = rb.solve()
        _check_kernel(product_lib, kernel)
        rb.close()
        xo, yo, io = batch.solve_batch(product_lib, *args, **OPTS)
        tol = 50 * 1e-5
        print("first solve: iters", info[:, 0], io[:, 0], "dx", np.max(np.abs(x - xo)), "dy", np.max(np.abs(y - yo)))
        assert np.array_equal(info[:, 1], io[:, 1]) and np.all(info[:, 1] == 1)
        assert np.max(np.abs(info[:, 0] - io[:, 0])) <= 25
        assert np.max(np.abs(x - xo)) <= tol * max(1.0, np.max(np.abs(xo)))
        assert np.max(np.abs(y - yo)) <= tol * max(1.0, np.max(np.abs(yo)))


VARIANTS = [dict(), dict(scaling=0), dict(adaptive_rho=0), dict(warm_start=False)]


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("family", FAMILIES)
def test_update_and_resolve_rounds_follow_the_oracle(product_lib, oracle_lib, monkeypatch, family, variant):
    """Setup, then rounds of {update; solve} on every instance, each round against the oracle model of the instance that
    went through the same rounds: no update at all (the oracle ends at its first check wherever it warm-starts, so must the
    engine), q, both bounds, boxes turned into equalities and back (the constraint classes follow the bounds), l alone, u
    alone with q.  Under the default settings, without scaling, without rho adaptation, and with warm_start = 0 (every
    round from zero; the reference is still the one updated model)."""
    opts = dict(OPTS, **VARIANTS[variant])
    probs, kernel, boxes = _problem(oracle_lib, family, monkeypatch)
    args = ref.stack(probs)
    q, l, u = args[4], args[5], args[6]
    rng = np.random.default_rng(11)
    rb = batch.ResidentBatch(product_lib, *args, **opts)
    ob = ref.OracleBatch(oracle_lib, probs, **opts)
    leq, ueq = l.copy(), u.copy()
    leq[:, boxes] = ueq[:, boxes] = 0.5 * (l[:, boxes] + u[:, boxes])
    width = np.where(np.isfinite(u - l), u - l, 0.0)
    q2 = q * (1 + 0.05 * rng.standard_normal(q.shape))
    rounds = [
        ("first", dict()),
        ("repeat", dict()),
        ("q", dict(q=q2)),
        ("bounds", dict(l=l - 0.02 * width, u=u + 0.02 * width)),
        ("equalities", dict(l=leq, u=ueq)),
        ("boxes again", dict(l=l, u=u)),
        ("l alone", dict(l=l - 0.01 * width)),
        ("u and q", dict(u=u + 0.01 * width, q=q)),
    ]
    for name, upd in rounds:
        if upd:
            rb.update(**upd)
            ob.update(**upd)
        x, y, info = rb.solve()
        _check_kernel(product_lib, kernel)
        refs = ob.solve()
        ref.compare(x, y, info, refs, opts, tag=f"{family}/{variant}/{name}")
        if name == "repeat" and opts.get("warm_start", True):
            at_first_check = [i for i, r in enumerate(refs) if r.info.iter == 25]  # (not: an instance that ran into max_iter)
            assert len(at_first_check) >= len(refs) - 1 and np.all(info[at_first_check, 0] == 25), info[:, 0]
    rb.close(); ob.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_update_q_before_the_first_solve_keeps_the_setup_scaling(product_lib, oracle_lib, monkeypatch, family):
    """The cost scaling c depends on the q given at setup.  On the oracle, MPC instance 2 of seed 2 with q <- 3 q + 1 takes
    150 iterations through setup-then-update and 100 through a fresh setup with the new q: an engine that re-equilibrates
    on update misses the one-check bound."""
    probs, kernel, _ = _problem(oracle_lib, family, monkeypatch)
    args = ref.stack(probs)
    q3 = 3 * args[4] + 1
    rb = batch.ResidentBatch(product_lib, *args, **OPTS)
    ob = ref.OracleBatch(oracle_lib, probs, **OPTS)
    rb.update(q=q3); ob.update(q=q3)
    x, y, info = rb.solve()
    _check_kernel(product_lib, kernel)
    refs = ob.solve()
    if family.startswith("mpc"):
        fresh = ref.cold_oracle(oracle_lib, ref.with_vectors(probs, q=q3), **OPTS)
        assert (refs[2].info.iter, fresh[2].info.iter) == (150, 100)
    ref.compare(x, y, info, refs, OPTS, tag=f"{family}/q-before-first-solve")
    rb.close(); ob.close()


def test_warm_starting_pays_where_the_oracle_says_it_does(product_lib, oracle_lib):
    """16 MPC instances of seed 5, six solves with the perturbations of batch_resident_ref.closed_loop_steps between them.
    (a) every step of the handle matches the oracle model that was updated and re-solved; (b) over steps 1 .. 5 the handle's
    total of ADMM iterations is below the total of the cold one-shot batch.solve_batch on the same data -- and so is the
    oracle's warm total against its cold one (3 725 against 7 775 with this draw order, no instance-step with warm > cold:
    tests/test_batch_resident_host.py), so a failure names the side that broke."""
    probs = ref.mpc_instances(oracle_lib, 0, 16, 5)
    args = ref.stack(probs)
    steps = ref.closed_loop_steps(args[4], args[5], args[6])
    warm_ref, cold_ref = ref.closed_loop_oracle(oracle_lib, probs, steps, **OPTS)
    rb = batch.ResidentBatch(product_lib, *args, **OPTS)
    warm_total = cold_total = 0
    for k, (q, l, u) in enumerate(steps):
        if k:
            rb.update(q=q, l=l, u=u)
        x, y, info = rb.solve()
        ref.compare(x, y, info, warm_ref[k], OPTS, tag=f"closed loop step {k}")
        xc, yc, ic = batch.solve_batch(product_lib, args[0], args[1], args[2], args[3], q, l, u, **OPTS)
        ref.compare(xc, yc, ic, cold_ref[k], OPTS, tag=f"cold step {k}")
        print(f"step {k}: engine warm {int(info[:, 0].sum())} cold {int(ic[:, 0].sum())}; oracle warm "
              f"{sum(r.info.iter for r in warm_ref[k])} cold {sum(r.info.iter for r in cold_ref[k])}")
        if k:
            warm_total += int(info[:, 0].sum()); cold_total += int(ic[:, 0].sum())
    rb.close()
    ow = sum(r.info.iter for rs in warm_ref[1:] for r in rs); oc = sum(r.info.iter for rs in cold_ref[1:] for r in rs)
    assert ow < oc, (ow, oc)
    assert warm_total < cold_total, (warm_total, cold_total)


@pytest.mark.parametrize("family", ["mpc", "quad64", "rows300"])
def test_explicit_warm_start_follows_the_oracle(product_lib, oracle_lib, monkeypatch, family):
    """warm_start(x, y) with the solution of slightly different data, with x alone, with y alone -- host and device form --
    each against oq.warm_start on the oracle model; a warm start at the exact solution ends at the first check.
    max_iter is 8000 here: instance 3 of the 64 x 100 family needs 3550 iterations from zero and, started from x alone, meets
    the tolerance on the oracle at iteration 4000 exactly -- with the file's limit of 4000 its status would be decided by
    which side of eps the last residual is rounded to, not by the warm start."""
    opts = dict(OPTS, max_iter=8000)
    probs, kernel, _ = _problem(oracle_lib, family, monkeypatch)
    args = ref.stack(probs)
    count = len(probs)
    near = ref.cold_oracle(oracle_lib, ref.with_vectors(probs, q=1.02 * args[4]), **opts)
    xs = np.array([r.x for r in near]); ys = np.array([r.y for r in near])
    rb = batch.ResidentBatch(product_lib, *args, **opts)
    ob = ref.OracleBatch(oracle_lib, probs, **opts)
    dx = batch.DeviceArray(product_lib, count, rb.n).upload(xs); dy = batch.DeviceArray(product_lib, count, rb.m).upload(ys)
    for name, kw_eng, kw_ref in (("x and y", dict(x=xs, y=ys), dict(x=xs, y=ys)), ("x alone", dict(x=xs), dict(x=xs)),
                                 ("y alone", dict(y=ys), dict(y=ys)), ("x and y, device", dict(x=dx, y=dy), dict(x=xs, y=ys)),
                                 ("x alone, device", dict(x=dx), dict(x=xs)), ("y alone, device", dict(y=dy), dict(y=ys))):
        rb.warm_start(**kw_eng); ob.warm_start(**kw_ref)
        x, y, info = rb.solve()
        _check_kernel(product_lib, kernel)
        ref.compare(x, y, info, ob.solve(), opts, tag=f"{family}/warm start {name}")
    # at the solution of the handle's own data (tight reference): the first check terminates
    exact = ref.cold_oracle(oracle_lib, probs, **dict(opts, eps_abs=1e-9, eps_rel=1e-9))
    xe = np.array([r.x for r in exact]); ye = np.array([r.y for r in exact])
    rb.warm_start(x=xe, y=ye); ob.warm_start(x=xe, y=ye)
    x, y, info = rb.solve()
    refs = ob.solve()
    ref.compare(x, y, info, refs, opts, tag=f"{family}/warm start at the solution")
    assert all(r.info.iter == 25 for r in refs) and np.all(info[:, 0] == 25), info[:, 0]
    rb.close(); ob.close()


@pytest.mark.parametrize("family,scaling", [("mpc", 10), ("quad64", 10), ("quad64", 0), ("rows300", 10), ("rows300", 0)])
def test_matrix_value_updates_follow_the_oracle(product_lib, oracle_lib, monkeypatch, family, scaling):
    """Two rounds of update(Px=, Ax=) -- values times 1 +- 5 % noise, which keeps the diagonally dominant P of the families
    positive definite -- alone, then together with q and the bounds, then P alone: against oq.update(model, Px=, Ax=).
    (The noise on A leaves some instances of the generic families primal infeasible: their rounds pin that an instance
    without a solution starts its next solve from zero with the rho it ended on, as the oracle does.)
    scaling = 0 is run on the generic families only.  Without equilibration the MPC family is not comparable round after
    round: on instance 3 of seed 2 with these matrices a COLD solve of the one-shot kernel and of the oracle -- same data,
    same start, 425 iterations each -- end 3.3e-8 apart where every other instance ends 1e-12 apart, i.e. the instance
    amplifies rounding differences by eight orders of magnitude within one solve; a warm round starts from iterates that
    already differ by 1e-12 and takes another set of rho updates (measured: 375 iterations against the oracle's 400 in the
    round after the update, then 100 against 150)."""
    opts = dict(OPTS, scaling=scaling)
    probs, kernel, _ = _problem(oracle_lib, family, monkeypatch)
    args = ref.stack(probs)
    Px, Ax, q, l, u = args[2:]
    rng = np.random.default_rng(23)
    rb = batch.ResidentBatch(product_lib, *args, **opts)
    ob = ref.OracleBatch(oracle_lib, probs, **opts)
    width = np.where(np.isfinite(u - l), u - l, 0.0)
    noise = lambda a: a * (1 + 0.05 * (2 * rng.random(a.shape) - 1))
    rounds = [("first", dict()),
              ("P and A", dict(Px=noise(Px), Ax=noise(Ax))),
              ("P, A, q, bounds", dict(Px=noise(Px), Ax=noise(Ax), q=noise(q), l=l - 0.01 * width, u=u + 0.01 * width)),
              ("P alone", dict(Px=noise(Px)))]
    for name, upd in rounds:
        if upd:
            rb.update(**upd); ob.update(**upd)
        x, y, info = rb.solve()
        _check_kernel(product_lib, kernel)
        ref.compare(x, y, info, ob.solve(), opts, tag=f"{family}/scaling {scaling}/{name}")
    rb.close(); ob.close()


def test_statuses_carry_over_as_in_the_oracle(product_lib, oracle_lib):
    """Instance 2 (MPC, seed 2) made primal infeasible for one round (the construction of
    test_batch_detects_infeasible_instance), feasible again in the next: a NaN row and status -3 / 3, then the status and the
    iteration count of the oracle model that went through the same rounds (its store_solution resets the iterate of an
    instance without a solution, the rho the infeasible round adapted stays: the oracle takes 125 iterations where a cold
    solve takes 75); the other instances undisturbed."""
    probs = ref.mpc_instances(oracle_lib, 0, 4, 2)
    args = ref.stack(probs)
    l, u = args[5], args[6]
    lbad, ubad = l.copy(), u.copy()
    lbad[2, 60] = 5.0; ubad[2, 60] = 20.0
    lbad[2, 0] = ubad[2, 0] = -30.0
    rb = batch.ResidentBatch(product_lib, *args, **OPTS)
    ob = ref.OracleBatch(oracle_lib, probs, **OPTS)
    seen = []
    for name, upd in (("feasible", dict()), ("infeasible", dict(l=lbad, u=ubad)), ("feasible again", dict(l=l, u=u))):
        if upd:
            rb.update(**upd); ob.update(**upd)
        x, y, info = rb.solve()
        refs = ob.solve()
        ref.compare(x, y, info, refs, OPTS, tag=f"statuses/{name}")
        seen.append((refs[2].info.status_val, refs[2].info.iter))
        if name == "infeasible":
            assert int(info[2, 1]) in (-3, 3) and np.all(np.isnan(x[2])) and np.all(np.isnan(y[2]))
            assert all(int(info[i, 1]) == 1 for i in (0, 1, 3))
    assert seen == [(1, 75), (-3, 100), (1, 125)], seen  # the reference's own statement of the case
    rb.close(); ob.close()


def test_device_pointer_form_equals_host_pointer_form(product_lib, oracle_lib):
    """Two handles on the same data, one fed numpy arrays, one device arrays (DeviceArray and torch tensors), through
    updates of every kind, a warm start and device outputs: bit for bit."""
    import torch

    probs = ref.mpc_instances(oracle_lib, 0, 10, 5)
    args = ref.stack(probs)
    Px, Ax, q, l, u = args[2:]
    count = len(probs)
    rng = np.random.default_rng(31)
    hb = batch.ResidentBatch(product_lib, *args, **OPTS)
    db = batch.ResidentBatch(product_lib, *args, **OPTS)
    out = db.alloc()
    dev = lambda a: batch.DeviceArray(product_lib, *a.shape).upload(a)
    ten = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def both():
        xh, yh, ih = hb.solve()
        xd, yd, idv = db.solve(out=out)
        assert np.array_equal(xh, xd.numpy(), equal_nan=True) and np.array_equal(yh, yd.numpy(), equal_nan=True)
        assert np.array_equal(ih, idv.numpy())
        return xh, yh

    x0, y0 = both()
    q2 = q * (1 + 0.03 * rng.standard_normal(q.shape)); l2 = l - 0.01; u2 = u + 0.01
    hb.update(q=q2); db.update(q=dev(q2)); both()
    hb.update(l=l2, u=u2); db.update(l=ten(l2), u=ten(u2)); both()
    hb.update(u=u); db.update(u=dev(u)); both()
    Px2 = Px * 1.03; Ax2 = Ax * (1 + 0.02 * (2 * rng.random(Ax.shape) - 1))
    hb.update(Px=Px2, Ax=Ax2); db.update(Px=ten(Px2), Ax=dev(Ax2)); both()
    hb.warm_start(x=x0, y=y0); db.warm_start(x=dev(x0), y=ten(y0)); both()
    hb.warm_start(x=x0); db.warm_start(x=ten(x0)); both()
    # torch tensors as outputs
    tout = (torch.empty((count, hb.n), dtype=torch.float64, device="cuda:0"), torch.empty((count, hb.m), dtype=torch.float64, device="cuda:0"),
            torch.empty((count, 6), dtype=torch.float64, device="cuda:0"))
    xh, yh, ih = hb.solve()
    db.solve(out=tout)
    assert np.array_equal(xh, tout[0].cpu().numpy()) and np.array_equal(yh, tout[1].cpu().numpy()) and np.array_equal(ih, tout[2].cpu().numpy())
    hb.close(); db.close()


def test_handles_and_instances_are_independent(product_lib, oracle_lib):
    """Two handles of different shapes alive at once give what each gives alone; instance i of a batch of 64 equals
    instance i in a batch of one through the same sequence (no state crosses instances)."""
    mpc = ref.mpc_instances(oracle_lib, 0, 64, 5)
    margs = ref.stack(mpc)
    gargs, _ = _family(64, 100, 6, 640100)
    q2 = margs[4] * 1.05
    g2 = gargs[4] * 0.9

    def run(rb, qn):
        res = [rb.solve()]
        rb.update(q=qn)
        res.append(rb.solve())
        res.append(rb.solve())
        return res

    a = batch.ResidentBatch(product_lib, *margs, **OPTS); alone_a = run(a, q2); a.close()
    b = batch.ResidentBatch(product_lib, *gargs, **OPTS); alone_b = run(b, g2); b.close()
    a = batch.ResidentBatch(product_lib, *margs, **OPTS)
    b = batch.ResidentBatch(product_lib, *gargs, **OPTS)
    ra, rbb = [a.solve()], [b.solve()]
    a.update(q=q2); b.update(q=g2)
    ra.append(a.solve()); rbb.append(b.solve()); rbb.append(b.solve()); ra.append(a.solve())
    a.close(); b.close()
    for got, want in ((ra, alone_a), (rbb, alone_b)):
        for g, w in zip(got, want):
            assert all(np.array_equal(gi, wi, equal_nan=True) for gi, wi in zip(g, w))
    for i in (0, 17, 63):
        one = batch.ResidentBatch(product_lib, margs[0], margs[1], *[v[i:i + 1] for v in margs[2:]], **OPTS)
        single = run(one, q2[i:i + 1])
        one.close()
        for g, w in zip(single, alone_a):
            assert all(np.array_equal(gi[0], wi[i], equal_nan=True) for gi, wi in zip(g, w)), i


def test_handle_hygiene(product_lib, oracle_lib):
    """close() twice is harmless; each handle family refuses the other's calls; update_bounds with one l > u raises and
    the following solve reproduces the previous data's result."""
    probs = ref.mpc_instances(oracle_lib, 0, 6, 5)
    args = ref.stack(probs)
    l, u = args[5], args[6]
    rb = batch.ResidentBatch(product_lib, *args, **OPTS)
    first = rb.solve()
    second = rb.solve()
    lbad = l.copy(); lbad[4, 7] = u[4, 7] + 1.0
    with pytest.raises(oq.OSQPError, match="lower bound"):
        rb.update(l=lbad)          # checked by the library against the u it holds
    with pytest.raises(oq.OSQPError, match="lower bound"):
        rb.update(q=2 * args[4], l=lbad, u=u)  # nothing of a refused call is applied, q included
    dl = batch.DeviceArray(product_lib, *lbad.shape).upload(lbad)
    with pytest.raises(oq.OSQPError, match="lower bound"):
        rb.update(l=dl)
    third = rb.solve()
    # a handle that never saw the refused updates gives the same three results: they left no trace
    rb2 = batch.ResidentBatch(product_lib, *args, **OPTS)
    for want in (first, second, third):
        assert all(np.array_equal(a, b) for a, b in zip(want, rb2.solve()))
    rb2.close(); rb2.close()
    mb = batch.MpcBatch(product_lib, 8, 1, device=0, **OPTS)
    packed = mb.alloc()
    assert product_lib.osqp_amd_batch_mpc_solve(rb.handle, packed.data_ptr()) != 0
    assert b"osqp_amd_batch_mpc_create" in product_lib.osqp_amd_last_error()
    buf = batch.DeviceArray(product_lib, 8, 200)
    for call in (lambda: product_lib.osqp_amd_batch_update_lin_cost(mb.handle, buf.data_ptr(), 1),
                 lambda: product_lib.osqp_amd_batch_update_bounds(mb.handle, buf.data_ptr(), None, 1),
                 lambda: product_lib.osqp_amd_batch_update_matrices(mb.handle, buf.data_ptr(), None, 1),
                 lambda: product_lib.osqp_amd_batch_warm_start(mb.handle, buf.data_ptr(), None, 1),
                 lambda: product_lib.osqp_amd_batch_resolve(mb.handle, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1)):
        assert call() != 0
        assert b"osqp_amd_batch_setup" in product_lib.osqp_amd_last_error()
    rb.handle, keep = mb.handle, rb.handle  # the Python class on an MPC handle raises
    with pytest.raises(oq.OSQPError):
        rb.solve()
    rb.handle = keep
    mb.solve(packed)  # both handles still work
    rb.solve()
    mb.close(); rb.close(); rb.close()
