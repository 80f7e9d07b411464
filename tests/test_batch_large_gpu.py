"""The opt-in batched path for 128 < n <= 256 (osqp_amd_batch_large -> k_batch_solve_large) on the
GPU.  The cases and their host side are tests/batch_large_cases.py; tests/test_batch_large_host.py checks with the oracle
alone what the bounds used here rest on (every reference Solved and certified, a re-factorisation among them, the statuses of
the chain families, the margins of the gap family).

Per shape: (a) the kernel that ran is the new one, with the planned LDS bytes; (b) - (e) as tests/test_batch_entries_gpu.py
defines them; two identical calls give identical bits.  Then: patterns with n <= 128 go where they went and return the bits they
returned; statuses and certificates; the resident life cycle against one oracle model per instance; the gap rule at exact
iteration counts; the refusals of polish, adjoint and JVP."""
import numpy as np
import pytest
import scipy.sparse as sp

import osqp_jl_amd as oq
from osqp_jl_amd import batch
import batch_cert_cases as cert
import batch_entry_families as F
import batch_gap_cases as G
import batch_large_cases as L
import batch_resident_ref as ref

pytestmark = pytest.mark.gpu

OPTS = F.OPTS
LARGE_KERNEL = -2


def _same(a, b):
    return all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


# ---- the six shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [L.COUNT, 1], ids=["seven", "one"])
@pytest.mark.parametrize("i", range(len(L.SHAPES)), ids=L.SHAPE_IDS)
def test_shape(product_lib, oracle_lib, i, count):
    lib = product_lib
    rf = F.reference(L.case(i), oracle_lib)
    rows, probs = rf["rows"][:count], rf["probs"][:count]
    args = rf["args"][:2] + tuple(a[:count] for a in rf["args"][2:])
    plan = batch.large_plan(lib, *F.pattern(*L.SHAPES[i][:2]))
    x, y, info = batch.solve_batch(lib, *args, large=True, **OPTS)
    sched = batch.last_schedule(lib)
    again = batch.solve_batch(lib, *args, large=True, **OPTS)
    assert lib.osqp_amd_batch_large(0) == 0  # the call put the switch back

    iter_diff = [int(abs(info[k, 0] - r["iter"])) for k, r in enumerate(rows)]
    ratios = [F.criteria_ratios(*probs[k], x[k], y[k], OPTS["eps_abs"], OPTS["eps_rel"]) for k in range(count)]
    e_K = [(F.rel_err(x[k], r["xs"]), F.rel_err(y[k], r["ys"])) for k, r in enumerate(rows)]
    bound = [tuple(max(r["e_O"][j], r["e_O1"][j]) for j in (0, 1)) for r in rows]
    for k in range(count):
        print(f"{L.SHAPE_IDS[i]} inst {k}: status {int(info[k, 1])} iter {int(info[k, 0])}/{rows[k]['iter']} rho updates {int(info[k, 5])} "
              f"ratios {ratios[k][0]:.3f} {ratios[k][1]:.3f}  e_K / bound x {e_K[k][0] / bound[k][0]:.3f} y {e_K[k][1] / bound[k][1]:.3f}")
    # (a) the branch
    assert sched["entry"] == LARGE_KERNEL == lib.osqp_amd_batch_last_kernel(), sched
    assert sched["lds_bytes"] == plan["lds_bytes"] and sched["instances"] == count, (sched, plan)
    for k, r in enumerate(rows):
        # (b) status, (c) iterations: the oracle's
        assert r["status"] == "Solved" and int(info[k, 1]) == r["status_val"], (k, info[k, :2], r["status"])
        assert iter_diff[k] <= F.CHECK, (k, info[k, 0], r["iter"])
        # (d) the stopping rule, re-evaluated
        assert max(ratios[k]) <= 2.0, (k, ratios[k])
        # (e) against the exact optimum: within twice the oracle's own error at its last or its previous check
        assert r["certified"]
        assert e_K[k][0] <= 2.0 * bound[k][0], (k, "x", e_K[k][0], bound[k][0])
        assert e_K[k][1] <= 2.0 * bound[k][1], (k, "y", e_K[k][1], bound[k][1])
    assert _same((x, y, info), again)
    if L.SHAPES[i][1][0] == 256 and count == L.COUNT:
        assert info[:, 5].max() >= 1  # a re-factorisation at the cap: every later iteration read the second inverse


# ---- unchanged below the limit -----------------------------------------------------------------------------------------------
BELOW = ["count7-e2-banded-n64", "e9-banded-n128-m192", "order-col33", "n128-unforced"]


@pytest.mark.parametrize("cid", BELOW)
def test_unchanged_below_the_limit(product_lib, oracle_lib, monkeypatch, cid):
    """A four-wavefront entry, the tightest fit at n = 128, the 512-thread kernel, and order-n129's neighbour at n = 128 as it
    comes: the same schedule and the same bits with the switch on as with it off."""
    lib = product_lib
    if cid == "n128-unforced":
        force, args = None, F.instances(F.pattern("banded", (128, 192, 4)), 6, 3100)[0]
    else:
        case = F.CASES[F.CASE_IDS.index(cid)]
        force, args = case["force"], F.case_problems(case, oracle_lib)[0]
    if force is None:
        monkeypatch.delenv("OSQP_AMD_BATCH_QUAD_CFG", raising=False)
    else:
        monkeypatch.setenv("OSQP_AMD_BATCH_QUAD_CFG", str(force))
    off = batch.solve_batch(lib, *args, **OPTS)
    sched_off = batch.last_schedule(lib)
    on = batch.solve_batch(lib, *args, large=True, **OPTS)
    sched_on = batch.last_schedule(lib)
    print(cid, sched_off)
    assert sched_on == sched_off and sched_off["entry"] != LARGE_KERNEL
    if cid != "n128-unforced":
        assert sched_off["entry"] == F.CASES[F.CASE_IDS.index(cid)]["expect"]
    assert np.all(off[2][:, 1] == 1)
    assert _same(off, on)


# ---- statuses and certificates -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", range(len(cert.VARIANTS)), ids=["default", "unscaled", "scaled_termination"])
@pytest.mark.parametrize("n,extra", L.CHAINS)
def test_statuses_and_certificates(product_lib, oracle_lib, n, extra, variant):
    opts = dict(cert.OPTS, **cert.VARIANTS[variant])
    args, probs = L.chain_family(n, extra)
    refs = [F.oracle_solve(oracle_lib, p, **opts) for p in probs]
    rb = batch.ResidentBatch(product_lib, *args, large=True, **opts)
    x, y, info = rb.solve()
    assert product_lib.osqp_amd_batch_last_kernel() == LARGE_KERNEL
    p, d = rb.certificates()
    pr, dr = rb.certificates(rows=[4, 1, 2])  # the gather of a selection
    assert _same((pr, dr), (p[[4, 1, 2]], d[[4, 1, 2]]))
    rb.close()
    ref.compare(x, y, info, refs, opts, f"chain{n}/{variant}")
    assert [r.info.status_val for r in refs] == [1, -3, -4, 1, -3, -4]
    for i, r in enumerate(refs):
        if cert.kind(i) == 0:
            assert np.all(np.isfinite(x[i])) and np.all(np.isnan(p[i])) and np.all(np.isnan(d[i])), i
            continue
        assert np.all(np.isnan(x[i])) and np.all(np.isnan(y[i])), i
        assert np.all(np.isnan(d[i] if cert.kind(i) == 1 else p[i])), i
        if not opts.get("scaled_termination", 0):  # (the criteria are stated in the caller's units)
            cert.check_certificate(int(info[i, 1]), p[i], d[i], probs[i], opts, tag=f"chain{n}/{variant}/{i}")


@pytest.mark.parametrize("n,extra", L.CHAINS)
def test_indefinite_p_is_non_convex(product_lib, oracle_lib, n, extra):
    probs = L.indefinite(n, extra)
    r = F.oracle_solve(oracle_lib, probs[0], **L.INDEFINITE_OPTS)
    x, y, info = batch.solve_batch(product_lib, *cert.stack(probs), large=True, **L.INDEFINITE_OPTS)
    print(n, "oracle", r.info.status_val, r.info.iter, "kernel", info[0, :2])
    assert product_lib.osqp_amd_batch_last_kernel() == LARGE_KERNEL
    assert r.info.status_val == -7 and int(info[0, 1]) == -7
    assert abs(int(info[0, 0]) - r.info.iter) <= F.CHECK
    assert np.all(np.isnan(x)) and np.all(np.isnan(y))


# ---- resident life cycle ----------------------------------------------------------------------------------------------------------
LIFE = [0, 3]  # banded (129, 193, 4) and random (256, 384, 7)


def _dev(lib, a):
    return batch.DeviceArray(lib, a.shape[0], a.shape[1]).upload(a)


@pytest.mark.parametrize("i", LIFE, ids=[L.SHAPE_IDS[k] for k in LIFE])
def test_resident_life_cycle_against_the_oracle(product_lib, oracle_lib, i):
    lib = product_lib
    kind, sargs, seed = L.SHAPES[i]
    args, probs = F.instances(F.pattern(kind, sargs), L.COUNT, seed)
    Px, Ax, q, l, u = args[2:]
    rng = np.random.default_rng(seed + 1)
    rb = batch.ResidentBatch(lib, *args, large=True, **OPTS)
    dv = batch.ResidentBatch(lib, *args, large=True, **OPTS)  # the same calls in their device-pointer forms
    assert lib.osqp_amd_batch_large(0) == 0
    ob = ref.OracleBatch(oracle_lib, probs, **OPTS)

    def both(tag):
        got = rb.solve()
        assert lib.osqp_amd_batch_last_kernel() == LARGE_KERNEL
        out = dv.solve(out=dv.alloc())
        ref.compare(*got, ob.solve(), OPTS, f"{L.SHAPE_IDS[i]}/{tag}")
        assert _same(got, [o.numpy() for o in out]), tag
        return got

    x0, y0, _ = both("setup -> solve")
    q2 = q * (1 + 0.05 * rng.standard_normal(q.shape))
    shift = 0.02 * rng.standard_normal(l.shape)
    l2, u2 = l + shift, u + shift
    rb.update(q=q2, l=l2, u=u2); dv.update(q=_dev(lib, q2), l=_dev(lib, l2), u=_dev(lib, u2)); ob.update(q=q2, l=l2, u=u2)
    both("update(q, l, u) -> warm re-solve")
    Px2 = Px * (1 + 0.02 * rng.random(Px.shape))  # every entry of an instance grows by at most 2 %: P stays diagonally dominant
    Ax2 = Ax * (1 + 0.05 * rng.standard_normal(Ax.shape))
    rb.update(Px=Px2, Ax=Ax2); dv.update(Px=_dev(lib, Px2), Ax=_dev(lib, Ax2)); ob.update(Px=Px2, Ax=Ax2)
    both("update(Px, Ax) -> re-solve")
    xw, yw = 0.8 * x0, 0.8 * y0
    rb.warm_start(x=xw, y=yw); dv.warm_start(x=_dev(lib, xw), y=_dev(lib, yw)); ob.warm_start(x=xw, y=yw)
    both("warm_start(x, y)")
    ob.close()

    # a selection of 3 of 7: the selected get the bits of a whole-batch call with the same data; the other four are left bit
    # for bit -- x, y, info of a following whole solve equal those of a twin that never saw the selection
    sel, rest = [5, 0, 3], [1, 2, 4, 6]
    twin = batch.ResidentBatch(lib, *args, large=True, **OPTS)      # never sees the selection
    whole = batch.ResidentBatch(lib, *args, large=True, **OPTS)     # gets the selection's data through whole-batch calls
    sub = batch.ResidentBatch(lib, *args, large=True, **OPTS)       # host form of the selection
    sdev = batch.ResidentBatch(lib, *args, large=True, **OPTS)      # device form of the selection
    for h in (twin, whole, sub, sdev):
        h.solve()
    q3, l3 = q.copy(), l.copy()
    q3[sel] = q[sel] * 0.97
    l3[sel] = l[sel] - 0.01
    whole.update(q=q3, l=l3)
    sub.update(q=q3[sel], l=l3[sel], rows=sel)
    sdev.update(q=_dev(lib, q3[sel]), l=_dev(lib, l3[sel]), rows=sel)
    w = whole.solve()
    s = sub.solve(rows=sel)
    assert lib.osqp_amd_batch_last_kernel() == LARGE_KERNEL and batch.last_schedule(lib)["instances"] == len(sel)
    sd = sdev.solve(out=sdev.alloc(len(sel)), rows=sel)
    assert _same([a[sel] for a in w], s), "selected: the bits of the whole-batch call"
    assert _same(s, [o.numpy() for o in sd]), "selected: device form"
    # warm start of the selection: the bits of a whole-batch warm start on the selected, nothing on the others
    xw3, yw3 = 0.9 * w[0], 0.9 * w[1]
    whole.warm_start(x=xw3, y=yw3)
    sub.warm_start(x=xw3[sel], y=yw3[sel], rows=sel)
    sdev.warm_start(x=_dev(lib, xw3[sel]), y=_dev(lib, yw3[sel]), rows=sel)
    w2 = whole.solve(rows=sel)
    assert _same(w2, sub.solve(rows=sel)) and _same(w2, [o.numpy() for o in sdev.solve(out=sdev.alloc(len(sel)), rows=sel)])
    t = twin.solve()
    for h in (sub, sdev):
        got = h.solve()
        assert _same([a[rest] for a in got], [a[rest] for a in t]), "the other four: untouched records"
    for h in (rb, dv, twin, whole, sub, sdev):
        h.close()


def test_settings_duality_on_a_large_handle(product_lib, oracle_lib):
    args, probs = F.instances(F.pattern(*L.SHAPES[1][:2]), 3, L.SHAPES[1][2])
    rb = batch.ResidentBatch(product_lib, *args, large=True, **OPTS)
    x, y, info = rb.solve()
    dual = rb.duality()
    for i, (P, q, A, l, u) in enumerate(probs):
        Pf = (sp.triu(P) + sp.triu(P, 1).T)
        prim = float(0.5 * x[i] @ (Pf @ x[i]) + q @ x[i])
        assert abs(dual[i, 0] - prim) <= 1e-9 * max(1.0, abs(prim)), (i, dual[i], prim)
        assert abs(dual[i, 2]) <= 1e-3 * max(1.0, abs(prim)), (i, dual[i])
    rb.update_settings(max_iter=30, warm_start=False)
    _, _, info2 = rb.solve()
    assert np.all(info2[:, 0] == 30) and np.all(np.isin(info2[:, 1], (-2, 2)))
    rb.close()


# ---- the gap rule -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [False, True], ids=["off", "on"])
def test_gap_rule(product_lib, oracle_lib, rule):
    args, probs = L.pf_family()
    tr = L.pf_trace(oq, oracle_lib)
    assert args[1].shape == (147, 146)
    rb = batch.ResidentBatch(product_lib, *args, large=True, **G.SETTINGS)
    if rule:
        rb.duality_gap_check()
    x, y, info = rb.solve()
    refusals = rb.gap_refusals()
    rb.close()
    assert product_lib.osqp_amd_batch_last_kernel() == LARGE_KERNEL
    for i, row in enumerate(tr):
        print(f"rule {rule} inst {i}: iter {int(info[i, 0])} status {int(info[i, 1])} refusals {refusals[i]:.0f} | K_off {row['K_off']} K_on {row['K_on']}")
    for i, row in enumerate(tr):
        want = row["K_on"] if rule else row["K_off"]
        assert int(info[i, 0]) == want and int(info[i, 1]) == 1, (i, info[i, :2], want)
        between = [k for k in row["checks"] if row["K_off"] <= k < row["K_on"]]
        assert refusals[i] == (len(between) if rule else 0), (i, refusals[i], between)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", LIFE, ids=[L.SHAPE_IDS[k] for k in LIFE])
def test_polish_adjoint_jvp_are_refused_and_leave_the_handle_usable(product_lib, i):
    """At n = 256 M does not fit the LDS; at n = 129 it would, but the substitutions of those kernels hold at most 128
    variables: the same check refuses both, before anything is launched."""
    import torch

    from osqp_jl_amd import qp_layer

    lib = product_lib
    kind, sargs, seed = L.SHAPES[i]
    args, _ = F.instances(F.pattern(kind, sargs), 3, seed)
    msg = "instance too large to polish"
    with pytest.raises(oq.OSQPError, match=msg):
        batch.ResidentBatch(lib, *args, large=True, **dict(OPTS, polish=True))
    rb = batch.ResidentBatch(lib, *args, large=True, **OPTS)
    twin = batch.ResidentBatch(lib, *args, large=True, **OPTS)
    first = rb.solve()
    assert _same(first, twin.solve())
    counts = lambda: (lib.osqp_amd_batch_polish_launches(), lib.osqp_amd_batch_adjoint_launches(), lib.osqp_amd_batch_jvp_launches())
    before = counts()
    with pytest.raises(oq.OSQPError, match=msg):
        rb.adjoint(dx=np.ones((rb.count, rb.n)))
    with pytest.raises(oq.OSQPError, match=msg):
        rb.jvp(q=np.ones((rb.count, rb.n)))
    with pytest.raises(oq.OSQPError, match=msg):
        rb.update_polish(True)
    layer = qp_layer.BatchQPLayer(rb, large=True)
    q = torch.tensor(args[4], dtype=torch.float64, device="cuda", requires_grad=True)
    x, _ = layer(q=q)  # forward works ...
    with pytest.raises(oq.OSQPError, match=msg):  # ... backward is the library's refusal
        x.sum().backward()
    assert counts() == before
    twin.update(q=args[4]); twin.solve()  # what the layer's forward did
    assert _same(rb.solve(), twin.solve())
    rb.close(); twin.close()


def test_n257_is_refused_naming_256(product_lib):
    args, _ = F.instances(F.banded(257, 385, 4), 1, 1)
    with pytest.raises(oq.OSQPError, match="n <= 256"):
        batch.solve_batch(product_lib, *args, large=True, **OPTS)
    with pytest.raises(oq.OSQPError, match="n <= 256"):
        batch.ResidentBatch(product_lib, *args, large=True, **OPTS)
    assert product_lib.osqp_amd_batch_large(0) == 0
