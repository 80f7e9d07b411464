"""The K-step tests of the shared batch without a GPU (tests/batch_shared_step_ref.py, the families `EDGES` of
tests/batch_shared_cases.py): what tests/test_batch_shared_steps_gpu.py rests on.
(a) the plan: every family reaches the branch of the dense step its line in the table names (T, ldm, ntile);
(b) the oracle solves every family: all 2 T + 3 instances Solved in fewer than max_iter - 25 iterations, with different
    counts inside the first tile;
(c) the oracle against the longdouble model: warm-started, max_iter = K, check_termination = 0 -- every status
    Max_iter_reached, x, y, pri_res, dua_res and obj_val inside tau = 32 K n 2^-53 kappa_2(M), on the six variants of
    `VARIANTS` and once under scaled_termination;
(d) discrimination: two deliberately wrong models -- equality rows given plain rho, z relaxed without alpha -- are outside
    tau of the oracle on EVERY instance of every family that has the feature.

Measured when this file was written (printed by (c) and (d)): the oracle's worst ratio to tau over the variants and
instances, and for the wrong models the SMALLEST ratio to tau over their variants and instances:
  family            kappa_2(M)   tau (K = 1)   oracle / tau   plain rho / tau   z without alpha / tau
  banded-2          1.2e+00      8.6e-15       8.7e-02        -                 9.5e+11
  banded-15         9.3e+00      4.9e-13       3.2e-03        -                 7.9e+10
  banded-16         8.8e+00      5.0e-13       5.9e-03        -                 1.9e+11
  banded-32-eq      8.9e+03      1.0e-09       6.0e-06        6.8e+12           8.2e+04
  banded-128        2.2e+01      9.9e-12       1.1e-04        -                 6.7e+09
  banded-130-m400   1.8e+01      8.3e-12       3.0e-04        -                 5.2e+09
  banded-176-eq     1.0e+04      6.3e-09       6.5e-06        2.7e+12           4.2e+04
  banded-240        2.4e+01      2.0e-11       5.8e-05        -                 3.0e+09
  banded-241-eq     1.3e+04      1.2e-08       2.6e-05        2.3e+12           8.7e+03
  banded-200-m460   2.1e+01      1.5e-11       8.9e-05        -                 3.1e+09
  m0                2.6e+00      3.1e-13       2.6e-03        -                 -
On `banded-2` tau is 64 kappa_2 units of 2^-53 and the double arithmetic OUTSIDE the dense step is no longer small against it:
test_the_smallest_family_leaves_the_bound_to_the_iteration says what its seed was chosen for."""
import numpy as np
import pytest

from osqp_jl_amd import batch
import batch_shared_cases as S
import batch_shared_step_ref as SR

FAMILIES = list(S.EDGES) + ["m0"]


_family = SR.family


def _model(oracle_lib, name, wrong=None, **opts):
    base = _family(name)[0]
    opts = dict(S.OPTS, **opts)
    scaling = SR.base_scaling(oracle_lib, (name, tuple(sorted(opts.items()))), base, **opts)
    return SR.model_of((name, wrong), base, scaling, rho=S.OPTS["rho"], wrong=wrong)


_oracle = {}


def _oracle_run(oracle_lib, name, variant, scaled_termination=False):
    """[(x, y, (pri_res, dua_res, obj_val), status, iter)] of the oracle models of a family on a variant; once per process."""
    key = (name, variant, scaled_termination)
    if key not in _oracle:
        base, q, l, u = _family(name)
        solves, alpha, start = SR.VARIANTS[variant]
        x0, y0 = SR.starts(name, *q.shape, l.shape[1])
        opts = dict(S.OPTS, warm_start=True, check_termination=0, max_iter=solves[0], scaled_termination=int(scaled_termination))
        ob = S.OracleShared(oracle_lib, base, q.shape[0], **opts)
        ob.update(q=q, l=l, u=u)
        ob.update_settings(alpha=alpha)
        ob.warm_start(x=x0 if "x" in start else None, y=y0 if "y" in start else None)
        for k in solves:
            ob.update_settings(max_iter=k)
            res = ob.solve()
        _oracle[key] = [(np.array(r.x), np.array(r.y), (r.info.pri_res, r.info.dua_res, r.info.obj_val), r.info.status_val, r.info.iter)
                        for r in res]
        ob.close()
    return _oracle[key]


def _wants(oracle_lib, name, variant, wrong=None, scaled_termination=False):
    base, q, l, u = _family(name)
    solves, alpha, start = SR.VARIANTS[variant]
    x0, y0 = SR.starts(name, *q.shape, l.shape[1])
    mdl = _model(oracle_lib, name, wrong)
    return SR.wants((name, variant, wrong, scaled_termination), mdl, q, l, u, x0, y0, sum(solves), alpha, start, scaled_termination)


# ---- (a) the plan ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.EDGES))
def test_every_family_reaches_the_branch_its_line_names(product_lib, name):
    kind, shape, _, _, T, ldm, ntile = S.EDGES[name]
    base, q, l, u = S.boxed(name)
    n = shape[0]
    plan = batch.shared_plan(product_lib, base[0], base[2])  # host only: no device is touched
    print(name, plan)
    assert plan["T"] == T and q.shape == (2 * T + 3, n) and l.shape == (2 * T + 3, shape[1])
    assert ldm == 16 * ((n + 15) // 16) and ntile == ldm // 16
    assert plan["model_bytes"] >= 8 * ldm * ldm and plan["lds_bytes"] <= 160 * 1024


def test_the_shape_without_rows_has_two_full_tiles_and_a_partial_one(product_lib):
    base, q, l, u = SR.family("m0")
    T = batch.shared_plan(product_lib, base[0], base[2])["T"]
    assert q.shape[0] == SR.M0_COUNT == 2 * T + 3 and l.shape == (SR.M0_COUNT, 0)
    assert np.array_equal(q[:5], S.unconstrained()[1])  # instance i is the same in any batch


def test_the_families_cover_the_branches_of_the_dense_step():
    """Every T; ldm == 16 with and without padding; a whole number of 32-column chunks and a 16-column tail; no wavefront with
    two tiles, one wavefront with two, all but one, all; padding rows under ldm == 256; T = 4 at an odd multiple of 16."""
    E = S.EDGES.values()
    assert {e[4] for e in E} == {16, 8, 4}
    assert {e[1][0] for e in E if e[5] == 16} >= {2, 15, 16}
    assert any(e[5] % 32 == 0 for e in E) and any(e[5] % 32 == 16 and e[5] > 16 for e in E)
    assert {e[6] for e in E} >= {1, 2, 8, 9, 15, 16}
    assert any(e[5] == 256 and e[1][0] < 256 for e in E)
    assert any(e[4] == 4 and e[6] % 2 == 1 for e in E)
    assert any(e[4] == 8 and e[3] > 0 for e in E) and any(e[4] == 8 and e[3] == 0 for e in E)


# ---- (b) the oracle solves ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.EDGES))
def test_oracle_solves_every_instance_well_below_max_iter(oracle_lib, name):
    base, q, l, u = S.boxed(name)
    T = S.EDGES[name][4]
    refs = S.reference(oracle_lib, ("boxed", name), base, q, l, u, **S.OPTS)
    its = [r.info.iter for r in refs]
    print(name, its)
    assert len(refs) == 2 * T + 3 and all(r.info.status_val == 1 for r in refs)
    assert max(its) < S.OPTS["max_iter"] - 25
    assert len(set(its[:T])) > 1  # different stop iterations inside the first tile


# ---- (c) the oracle against the model -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILIES)
def test_oracle_is_inside_tau_of_the_model(oracle_lib, name):
    worst = {}
    for variant, (solves, alpha, start) in SR.VARIANTS.items():
        got, want = _oracle_run(oracle_lib, name, variant), _wants(oracle_lib, name, variant)
        assert [g[3] for g in got] == [SR.expected_status(name, variant)] * len(got), (variant, [g[3] for g in got])
        assert all(g[4] == solves[-1] for g in got)
        worst[variant] = np.max([SR.ratios(g[0], g[1], g[2], w) for g, w in zip(got, want)], axis=0)
    mdl = _model(oracle_lib, name)
    top = max(float(np.max(v)) for v in worst.values())
    print(f"{name}: kappa_2(M) {mdl.kappa:.1e}, tau(K = 1) {mdl.tau(1):.1e}, {len(got)} instances, oracle worst ratio to tau {top:.1e}")
    for variant, v in worst.items():
        print(f"  {variant:12s} x {v[0]:.1e}  y {v[1]:.1e}  pri_res {v[2]:.1e}  dua_res {v[3]:.1e}  obj_val {v[4]:.1e}")
    assert top <= 1.0, worst
    if mdl.n >= 15:  # the kernel has the bound to itself: the double arithmetic of the rest takes less than a hundredth of it
        assert top <= 0.01, worst


def test_the_smallest_family_leaves_the_bound_to_the_iteration(oracle_lib):
    """At n = 2 tau is 64 kappa units of 2^-53 and no longer dwarfs the roundings outside the dense step: y = rho (zh - z) carries
    about two roundings of zh ~ z, which the un-scaling E / c multiplies.  The seed of `banded-2` is one with max E <= 2 c, so
    that those stay below a tenth of tau (a seed with E = 66 puts the ORACLE at 3 tau: the bound then tests the seed)."""
    mdl = _model(oracle_lib, "banded-2")
    print(f"banded-2: E {mdl.E.astype(float)}, c {float(mdl.c):.3f}, kappa_2(M) {mdl.kappa:.2f}")
    assert float(np.max(mdl.E) / mdl.c) <= 2.0


@pytest.mark.parametrize("name", ["banded-15", "banded-176-eq", "m0"])
def test_oracle_is_inside_tau_of_the_model_under_scaled_termination(oracle_lib, name):
    got = _oracle_run(oracle_lib, name, "K3-alpha1.6", True)
    want = _wants(oracle_lib, name, "K3-alpha1.6", None, True)
    assert all(g[3] == -2 for g in got)
    worst = np.max([SR.ratios(g[0], g[1], g[2], w) for g, w in zip(got, want)], axis=0)
    print(f"{name} scaled_termination: worst ratios to tau (x, y, pri_res, dua_res, obj_val) {worst}")
    assert np.max(worst) <= 1.0
    plain = _wants(oracle_lib, name, "K3-alpha1.6")
    if name != "m0":  # the flag matters: the unscaled figures are not the scaled ones
        assert any(abs(float(w["pri_res"] - p["pri_res"])) > float(w["tau"] * w["scale"][0]) for w, p in zip(want, plain))


# ---- (d) discrimination -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k, e in S.EDGES.items() if e[3] > 0])
def test_equality_rows_given_plain_rho_break_the_bound(oracle_lib, name):
    assert _model(oracle_lib, name).equalities == S.EDGES[name][3]
    for variant in ("K1-alpha1.0", "K3-alpha1.6"):
        got, want = _oracle_run(oracle_lib, name, variant), _wants(oracle_lib, name, variant, "plain_rho")
        r = [max(SR.ratios(g[0], g[1], g[2], w)) for g, w in zip(got, want)]
        print(f"{name} {variant}: equality rows given plain rho, ratio to tau {min(r):.1e} .. {max(r):.1e}")
        assert min(r) > 1.0, r


@pytest.mark.parametrize("name", list(S.EDGES))
def test_z_relaxed_without_alpha_breaks_the_bound(oracle_lib, name):
    for variant in ("K1-alpha1.6", "K3-alpha1.6"):
        got, want = _oracle_run(oracle_lib, name, variant), _wants(oracle_lib, name, variant, "z_without_alpha")
        r = [max(SR.ratios(g[0], g[1], g[2], w)) for g, w in zip(got, want)]
        print(f"{name} {variant}: z relaxed without alpha, ratio to tau {min(r):.1e} .. {max(r):.1e}")
        assert min(r) > 1.0, r
    # with alpha = 1 the wrong model IS the right one: what breaks the bound above is the missing alpha and nothing else
    got, want = _oracle_run(oracle_lib, name, "K1-alpha1.0"), _wants(oracle_lib, name, "K1-alpha1.0", "z_without_alpha")
    assert max(max(SR.ratios(g[0], g[1], g[2], w)) for g, w in zip(got, want)) <= 1.0
