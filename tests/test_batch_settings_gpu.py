"""Settings updates of the resident batch (`ResidentBatch.update_settings`, osqp_amd_batch_update_setting) on the GPU, on
the MPC family (8 instances) and chain(12, 6) (6 instances) of tests/batch_cert_cases.py -- both with infeasible members.
A setting changed after setup must act exactly as the same setting given at setup (twin handles, bit for bit), and a
sequence of changes must follow one oracle model per instance given the same `update_settings` calls."""
import numpy as np
import pytest

import osqp_jl_amd as oq
from osqp_jl_amd import batch
from osqp_jl_amd.interface import OSQPError
import batch_cert_cases as cases
import batch_resident_ref as ref

pytestmark = pytest.mark.gpu

OPTS = cases.OPTS
FAMILIES = ["mpc", "chain12"]


def _probs(oracle_lib, family):
    return cases.mpc(oracle_lib, 8) if family == "mpc" else cases.chain(12, 6)


def _same(a, b):
    return all(np.array_equal(s, t, equal_nan=True) for s, t in zip(a, b))


# (settings at setup of A, what update_settings changes before the first solve = settings at setup of B)
TWINS = [
    (dict(eps_abs=1e-3, eps_rel=1e-3), dict(eps_abs=1e-6, eps_rel=1e-6)),
    (dict(rho=0.1), dict(rho=1.0)),
    (dict(alpha=1.6), dict(alpha=1.2)),
    (dict(max_iter=4000), dict(max_iter=30)),
    (dict(check_termination=25), dict(check_termination=10)),
    (dict(scaled_termination=0), dict(scaled_termination=1)),
]


@pytest.mark.parametrize("twin", range(len(TWINS)), ids=[",".join(t[1]) for t in TWINS])
@pytest.mark.parametrize("family", FAMILIES)
def test_a_setting_updated_before_the_first_solve_is_the_setting_at_setup(product_lib, oracle_lib, family, twin):
    before, after = TWINS[twin]
    args = cases.stack(_probs(oracle_lib, family))
    A = batch.ResidentBatch(product_lib, *args, **dict(OPTS, **before))
    A.update_settings(**after)
    B = batch.ResidentBatch(product_lib, *args, **dict(OPTS, **after))
    ra, rb = A.solve(), B.solve()
    C = batch.ResidentBatch(product_lib, *args, **dict(OPTS, **before))
    rc = C.solve()
    A.close(); B.close(); C.close()
    print(family, after, "iter", ra[2][:, 0], "without the update", rc[2][:, 0])
    assert _same(ra, rb)
    assert not _same(ra, rc)  # the setting matters on this family: the twins do not agree trivially


def _oracle_settings(ob, **kw):
    for m in ob.models:
        oq.update_settings(m, **kw)


@pytest.mark.parametrize("family", FAMILIES)
def test_a_sequence_of_updates_follows_the_oracle(product_lib, oracle_lib, family):
    """solve; tighten eps, warm solve; rho = 1.0 and a new q, solve; max_iter = 10 and another q, solve (every instance
    stops at the limit: -2 at iteration 10); max_iter = 4000, warm_start = 0 and the first q again, solve.
    The q of the max_iter = 10 step is -q with the cost of the free direction of the dual infeasible members set to 0: with
    a cost there the checks made at the iteration limit find them dual infeasible (-4 at iteration 10, on the oracle too),
    without it they are bounded and run into the limit like the rest."""
    probs = _probs(oracle_lib, family)
    args = cases.stack(probs)
    q = args[4]
    rb = batch.ResidentBatch(product_lib, *args, **OPTS)
    ob = ref.OracleBatch(oracle_lib, probs, **OPTS)
    opts = dict(OPTS)
    q10 = -q
    q10[[i for i in range(len(probs)) if cases.kind(i) == 2], 96 if family == "mpc" else 0] = 0.0
    steps = [
        ("first", {}, None),
        ("tight", dict(eps_abs=1e-7, eps_rel=1e-7), None),
        ("rho", dict(rho=1.0), 2.0 * q + 0.5),
        ("max_iter10", dict(max_iter=10), q10),
        ("cold", dict(max_iter=4000, warm_start=0), q),
    ]
    adapted = 0
    for tag, change, qn in steps:
        if change:
            rb.update_settings(**change)
            _oracle_settings(ob, **change)
            opts.update(change)
        if qn is not None:
            rb.update(q=qn)
            ob.update(q=qn)
        x, y, info = rb.solve()
        refs = ob.solve()
        ref.compare(x, y, info, refs, opts, tag=f"{family}/{tag}")
        if tag == "first":
            adapted = int(np.sum(info[:, 5] > 0))
        if tag == "max_iter10":
            assert np.all(info[:, 1] == -2) and np.all(info[:, 0] == 10), info[:, :2]
    rb.close(); ob.close()
    assert adapted > 0  # the rho step replaced adapted values, not only the setting


@pytest.mark.parametrize("family", FAMILIES)
def test_rho_replaces_the_adapted_rho_of_every_instance(product_lib, oracle_lib, family):
    """After a solve that adapted rho, update_settings(rho = r) and a solve agree with the oracle models given the same call
    -- and differ from the solve of a twin handle that went on with its adapted values."""
    probs = _probs(oracle_lib, family)
    args = cases.stack(probs)
    rb, twin = batch.ResidentBatch(product_lib, *args, **OPTS), batch.ResidentBatch(product_lib, *args, **OPTS)
    ob = ref.OracleBatch(oracle_lib, probs, **OPTS)
    x, y, info = rb.solve()
    twin.solve()
    ref.compare(x, y, info, ob.solve(), OPTS, tag=f"{family}/first")
    assert np.any(info[:, 5] > 0), info[:, 5]
    qn = 1.5 * args[4] - 0.25
    for r in (0.02, 5.0):
        rb.update_settings(rho=r)
        _oracle_settings(ob, rho=r)
        rb.update(q=qn); twin.update(q=qn); ob.update(q=qn)
        x, y, info = rb.solve()
        ref.compare(x, y, info, ob.solve(), OPTS, tag=f"{family}/rho={r}")
        xt, yt, infot = twin.solve()
        print(f"{family} rho={r}: iter {info[:, 0]} twin without the update {infot[:, 0]}")
        assert not _same((x, y, info), (xt, yt, infot))
        qn = -qn
    rb.close(); twin.close(); ob.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_refused_updates_leave_the_handle_unchanged(product_lib, oracle_lib, family):
    args = cases.stack(_probs(oracle_lib, family))
    A, B = batch.ResidentBatch(product_lib, *args, **OPTS), batch.ResidentBatch(product_lib, *args, **OPTS)
    assert _same(A.solve(), B.solve())
    for bad, word in ((dict(eps_abs=-1e-3), "eps_abs"), (dict(eps_prim_inf=-1.0), "eps_prim_inf"), (dict(alpha=2), "alpha"),
                      (dict(max_iter=0), "max_iter"), (dict(rho=0), "rho"), (dict(max_iter=10.5), "max_iter"),
                      (dict(sigma=1e-3), "sigma cannot be updated or is not recognized"),
                      (dict(no_such_setting=1), "no_such_setting cannot be updated or is not recognized"),
                      (dict(warm_start=2), "warm_start"), (dict(polish_refine_iter=-1), "polish_refine_iter"),
                      (dict(check_termination=float("nan")), "check_termination"), (dict(delta=float("nan")), "delta")):
        with pytest.raises(OSQPError, match=word):
            A.update_settings(**bad)
    # the library's own answer to the names Python stops
    for name in (b"sigma", b"scaling", b"adaptive_rho", b"adaptive_rho_interval", b"linsys_solver", b"no_such_setting", b""):
        assert product_lib.osqp_amd_batch_update_setting(A.handle, name, 1.0) == 1
        assert b"cannot be updated or is not recognized" in product_lib.osqp_amd_last_error(), name
    assert product_lib.osqp_amd_batch_update_setting(A.handle, None, 1.0) == 1
    mpc_handle = batch.MpcBatch(product_lib, 4, seed=2, **OPTS)  # the other family's handle
    assert product_lib.osqp_amd_batch_update_setting(mpc_handle.handle, b"eps_abs", 1e-3) == 1
    assert b"osqp_amd_batch_setup" in product_lib.osqp_amd_last_error()
    mpc_handle.close()
    A.update_settings(time_limit=1e-9, verbose=1)  # accepted, stored, without effect
    qn = 0.5 * args[4]
    A.update(q=qn); B.update(q=qn)
    assert _same(A.solve(), B.solve())
    A.close(); B.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_polish_through_update_settings(product_lib, oracle_lib, family):
    args = cases.stack(_probs(oracle_lib, family))
    A, B = batch.ResidentBatch(product_lib, *args, **OPTS), batch.ResidentBatch(product_lib, *args, **OPTS)
    n0 = product_lib.osqp_amd_batch_polish_launches()
    A.update_settings(polish=1, polish_refine_iter=5)
    B.update_polish(1, 5)
    ra, rb = A.solve(), B.solve()
    assert product_lib.osqp_amd_batch_polish_launches() == n0 + 2
    sa, sb = A.polish_status(), B.polish_status()
    print(family, "status_polish", sa)
    assert np.any(sa == 1) and np.array_equal(sa, sb) and _same(ra, rb)
    assert A.polish_refine_iter == 5
    pa = A.certificates()
    A.update_settings(eps_abs=1e-4)  # no setting change touches the results of the last resolve
    assert np.array_equal(A.polish_status(), sa) and _same(A.certificates(), pa)
    A.update_settings(polish=0)
    B.update_polish(0, 5)
    assert _same(A.solve(), B.solve()) and np.all(A.polish_status() == 0)
    A.close(); B.close()
