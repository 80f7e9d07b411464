"""The shared batch (k_batch_solve_shared, k_shared_warm, shared_check in osqp.jl_amd/csrc/batch_shared.hpp) held to the K-step
model of tests/batch_shared_step_ref.py on the GPU: after `warm_start(x0, y0)` a solve with max_iter = K and
check_termination = 0 runs exactly K iterations from a known state and returns D x_K, E y_K / c and the figures of the last
check, which are compared with K iterations in numpy.longdouble -- instance by instance, all 2 T + 3 of them, on the families
`EDGES` of tests/batch_shared_cases.py (every T, and every branch of the dense step on ldm and ntile) and the shape without
rows.  The bound is tau = 32 K n 2^-53 kappa_2(M) (the step reference has the derivation); a misplaced lane, padding row, T
stride or un-scaling is an error of 1e-2 and up.  tests/test_batch_shared_steps_host.py holds the families, the model and the
bound to what this file rests on, without a GPU.

Also here: the carry between solves (three solves of one iteration against one of three: the same bits -- the code is
built without contraction and both forms of zt = rho z - y, at the start of a solve and at the end of an iteration, read the same
stored rho, z and y), and every updatable setting but rho on a live handle against a fresh handle (bits) and the oracle.

FIGURES on an MI355X: worst kernel-vs-model error over the instances and x, y, pri_res, dua_res, obj_val, as a multiple of tau
  family            tau (K = 1)   K = 1, alpha = 1   worst other variant
  banded-2          8.6e-15       6.7e-02            3.9e-01   (obj_val after three iterations; x and y at most 8.4e-02)
  banded-15         4.9e-13       2.2e-03            3.5e-03
  banded-16         5.0e-13       2.9e-03            4.9e-03
  banded-32-eq      1.0e-09       1.7e-03            2.4e-03
  banded-128        9.9e-12       1.9e-04            4.1e-04
  banded-130-m400   8.3e-12       1.9e-04            8.3e-04
  banded-176-eq     6.3e-09       1.1e-05            1.9e-05
  banded-240        2.0e-11       1.9e-04            2.7e-04
  banded-241-eq     1.2e-08       7.4e-05            1.4e-04
  banded-200-m460   1.5e-11       1.7e-04            2.7e-04
  m0                3.1e-13       2.6e-03            2.9e-03
Under scaled_termination (K = 3): banded-15 2.7e-03, banded-176-eq 6.1e-06, m0 1.2e-03.  The three chained solves had the bits
of the one solve of three iterations on every family, in x, y and info columns 1 to 5."""
import numpy as np
import pytest

from osqp_jl_amd import batch
import batch_resident_ref as ref
import batch_shared_cases as S
import batch_shared_step_ref as SR

pytestmark = pytest.mark.gpu

FAMILIES = list(S.EDGES) + ["m0"]
STEP_OPTS = dict(S.OPTS, warm_start=True, check_termination=0)


def _same(a, b):
    return all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


def _make(lib, base, q, l, u, **opts):
    P, q0, A, l0, u0 = base
    sb = batch.SharedBatch(lib, P, A, q0, l0, u0, q.shape[0], **opts)
    sb.update(q=q, l=l if l.shape[1] else None, u=u if u.shape[1] else None)
    return sb


def _model(oracle_lib, name):
    base = SR.family(name)[0]
    scaling = SR.base_scaling(oracle_lib, (name, tuple(sorted(S.OPTS.items()))), base, **S.OPTS)
    return SR.model_of((name, None), base, scaling, rho=S.OPTS["rho"])


def _run(lib, name, variant, **settings):
    """The solves of a variant on a fresh handle -> (x, y, info) of the last one."""
    base, q, l, u = SR.family(name)
    solves, alpha, start = SR.VARIANTS[variant]
    x0, y0 = SR.starts(name, *q.shape, l.shape[1])
    sb = _make(lib, base, q, l, u, **dict(STEP_OPTS, max_iter=solves[0]))
    sb.update_settings(alpha=alpha, **settings)  # not at setup: the setting of a live handle is what the kernel reads
    sb.warm_start(x=x0 if "x" in start else None, y=y0 if "y" in start else None)
    for _ in solves:
        out = sb.solve()
    sb.close()
    return out


# ---- 1. K steps against the model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(SR.VARIANTS))
@pytest.mark.parametrize("name", FAMILIES)
def test_k_steps_are_inside_tau_of_the_model(product_lib, oracle_lib, name, variant):
    base, q, l, u = SR.family(name)
    solves, alpha, start = SR.VARIANTS[variant]
    x0, y0 = SR.starts(name, *q.shape, l.shape[1])
    mdl = _model(oracle_lib, name)
    want = SR.wants((name, variant, None, False), mdl, q, l, u, x0, y0, sum(solves), alpha, start)
    x, y, info = _run(product_lib, name, variant)
    r = np.array([SR.ratios(x[i], y[i], info[i, 2:5], w) for i, w in enumerate(want)])
    worst = r.max(axis=0)
    print(f"{name} {variant}: {len(want)} instances, kappa_2(M) {mdl.kappa:.1e}, tau {want[0]['tau']:.1e}, kernel vs model / tau: "
          f"x {worst[0]:.1e} y {worst[1]:.1e} pri_res {worst[2]:.1e} dua_res {worst[3]:.1e} obj_val {worst[4]:.1e}  WORST {worst.max():.1e}")
    assert np.all(info[:, 0] == solves[-1]), info[:, 0]
    assert np.all(info[:, 1] == SR.expected_status(name, variant)), info[:, 1]
    assert np.all(r <= 1.0), (np.argwhere(r > 1.0), r.max(axis=0))
    assert np.all(info[:, 5] == 0)


@pytest.mark.parametrize("name", ["banded-15", "banded-176-eq", "m0"])
def test_k_steps_under_scaled_termination(product_lib, oracle_lib, name):
    """scaled_termination = 1, set on the live handle: the same iterate, pri_res and dua_res in the scaled units."""
    variant = "K3-alpha1.6"
    base, q, l, u = SR.family(name)
    solves, alpha, start = SR.VARIANTS[variant]
    x0, y0 = SR.starts(name, *q.shape, l.shape[1])
    want = SR.wants((name, variant, None, True), _model(oracle_lib, name), q, l, u, x0, y0, sum(solves), alpha, start, True)
    x, y, info = _run(product_lib, name, variant, scaled_termination=1)
    r = np.array([SR.ratios(x[i], y[i], info[i, 2:5], w) for i, w in enumerate(want)])
    print(f"{name} scaled_termination: kernel vs model / tau (x, y, pri_res, dua_res, obj_val) {r.max(axis=0)}")
    assert np.all(info[:, 0] == 3) and np.all(info[:, 1] == -2)
    assert np.all(r <= 1.0), r.max(axis=0)
    plain = _run(product_lib, name, variant)
    assert _same(plain[:2], (x, y)) and not np.array_equal(plain[2][:, 3], info[:, 3])  # the flag changes the figures alone


# ---- 2. the carry between solves -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILIES)
def test_three_solves_of_one_iteration_are_one_solve_of_three(product_lib, name):
    """Both are inside tau of the model (the test above); here: the same bits in x and y, so the x, z and y a solve leaves in the
    tile record are exactly the ones the loop would have gone on with."""
    one, three = _run(product_lib, name, "K3-alpha1.6"), _run(product_lib, name, "K3-chained")
    assert np.all(one[2][:, 0] == 3) and np.all(three[2][:, 0] == 1)
    assert _same(one[:2], three[:2])
    assert _same((one[2][:, 1:],), (three[2][:, 1:],))  # and the figures of the last check


# ---- 3. settings on a live handle ------------------------------------------------------------------------------------------------
UPDATES = [dict(max_iter=60), dict(eps_abs=1e-3, eps_rel=1e-3), dict(alpha=1.0), dict(check_termination=7), dict(check_termination=1),
           dict(check_termination=0), dict(scaled_termination=1), dict(eps_prim_inf=1e-2, eps_dual_inf=1e-2)]
MATTERS = UPDATES[:4] + [dict(scaled_termination=1)]  # these change the results of these families (the oracle's too)


@pytest.mark.parametrize("name", ["banded-176-eq", "banded-15"])
def test_settings_updated_on_a_live_handle(product_lib, oracle_lib, name):
    """One setting after the other on one handle (warm_start = False: every solve is cold): the next solve has the bits of a
    fresh handle set up with the settings so far, and follows oracle models given the same `update_settings`."""
    base, q, l, u = S.boxed(name)
    opts = dict(S.OPTS, warm_start=False)
    sb = _make(product_lib, base, q, l, u, **opts)
    ob = S.OracleShared(oracle_lib, base, q.shape[0], **opts)
    ob.update(q=q, l=l, u=u)
    first = sb.solve()
    ref.compare(*first, ob.solve(), opts, tag=f"{name} default")
    previous = first
    for change in UPDATES:
        sb.update_settings(**change); ob.update_settings(**change)
        ob.update(q=q)  # the same q again: a settings update alone leaves the oracle the status of its previous solve
        opts.update(change)
        got = sb.solve()
        fresh = _make(product_lib, base, q, l, u, **opts)
        assert _same(got, fresh.solve()), change
        fresh.close()
        ref.compare(*got, ob.solve(), opts, tag=f"{name} {change}")
        its, check, max_iter = got[2][:, 0], opts.get("check_termination", 25), opts["max_iter"]
        print(f"{name} {change}: iter {its.astype(int)} status {got[2][:, 1].astype(int)}")
        assert np.all(its <= max_iter)
        if check:
            assert np.all((its % check == 0) | (its == max_iter)), its
        else:
            assert np.all(its == max_iter), its
        if change in MATTERS:
            assert not _same(got, previous), change  # the setting matters here: the twins do not agree trivially
        previous = got
    sb.close(); ob.close()
