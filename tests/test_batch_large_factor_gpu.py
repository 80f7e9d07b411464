"""Polish, adjoint and JVP on resident handles with 128 < n <= 256 (osqp_amd_batch_large_factor: the LARGE forms of
k_batch_polish, k_batch_adjoint, k_batch_jvp with the factor in the instance's global scratch) on the
GPU.  Shapes, oracle runs and incoming gradients are tests/batch_large_factor_cases.py; tests/test_batch_large_factor_host.py
checks with the oracle alone what is assumed here (every Solved instance polish-accepted, non-degenerate active sets) and
records MEASURED, the figures of the numpy models against their references.

References: polish -- one oracle model per instance with polish = True; derivatives -- `batch_adjoint_ref.exact` /
`batch_jvp_ref.exact` on the GPU's OWN returned x, y and act, as the n <= 128 tests are built.
Bound of a kernel against its reference, relative to max(1, max|reference|): per shape 1000 x MEASURED[shape] of its model
(another summation order on well-conditioned active sets: the rule of tests/test_batch_adjoint_gpu.py), never above 1e-9.
The polish test also asserts that polished and unpolished x differ by more than 100 x the bound on the constrained shapes:
otherwise agreement with the oracle would not show that polish ran.

FIGURES measured on the MI355X (the first test of each kind prints those of a run), worst over the cases, against the
bounds of 7.2e-13 (m = 0) to 2.4e-11:
  polish vs oracle     x 1.1e-15, y 1.8e-14 (banded-256x512x6 and banded-129x193x4: 1.6e-14; bound 1.3e-11 / 1.4e-11), polished
                       residuals 1.1e-14 (random-255x300x7 under scaling = 0), objective 2.0e-15; status_polish equal on every
                       instance of every case; instance 5 of random-255x300x7 under scaling = 0 ends with status 2 on both
                       sides and keeps the twin's bits;
                       polished vs unpolished x 7.3e-5 .. 3.1e-4 per constrained case (at least 3e6 x the bound)
  adjoint vs exact     9.4e-16 (m = 1) .. 1.9e-14 (banded-256x512x6, bound 2.0e-11)
  JVP vs exact         1.0e-15 (m = 1) .. 5.5e-14 (random-256x384x7, bound 2.4e-11); duality with the adjoint <= 5.6e-17
  jacobian, n = 129    forward vs reverse 2.2e-16
  m = 0                polished x 9.6e-16, adjoint 9.0e-16, JVP 9.6e-16 (bounds 7.2e-13, 9.0e-13, 9.0e-13)
Every figure is a factor 250 or more inside its bound (the closest: JVP on random-144x200x7, 2.6e-14 against 6.8e-12)."""
import numpy as np
import pytest

import osqp_jl_amd as oq
from osqp_jl_amd import batch
import batch_adjoint_ref as adj
import batch_jvp_ref as jv
import batch_large_factor_cases as C
from test_batch_large_factor_host import MEASURED

pytestmark = pytest.mark.gpu

CAP = 1e-9
NDIR = NCOT = 3
MSG = "instance too large to polish"
POLISH_CASES = [(i, v) for i in range(len(C.SHAPES)) for v in (range(3) if i in C.ALL_VARIANTS else (0,))]
POLISH_CASES.append((2, 1))  # random(255, 300, 7) under scaling = 0: instance 5 ends with status 2 and is left alone
POLISH_IDS = [f"{C.SHAPE_IDS[i]}-{C.VARIANT_IDS[v]}" for i, v in POLISH_CASES]
WITH_ROWS = [0, 1, 2, 3, 4, 5]  # the shapes with m > 0


def bound(i, kind):
    return min(CAP, 1000 * MEASURED[C.SHAPE_IDS[i]][("polish", "adjoint", "jvp").index(kind)])


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _same_all(a, b):
    return all(_same(u, v) for u, v in zip(a, b))


def _counts(lib):
    return (lib.osqp_amd_batch_polish_launches(), lib.osqp_amd_batch_adjoint_launches(), lib.osqp_amd_batch_jvp_launches())


def _handle(lib, i, variant=0, count=C.COUNT, **kw):
    args = C.problems(i)[0]
    args = args[:2] + tuple(a[:count] for a in args[2:])
    return batch.ResidentBatch(lib, *args, large=True, **dict(C.opts_of(variant), **kw))


# ---- polish ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,variant", POLISH_CASES, ids=POLISH_IDS)
def test_polish_follows_the_oracle(product_lib, oracle_lib, i, variant):
    lib, sid, B = product_lib, C.SHAPE_IDS[i], bound(i, "polish")
    runs = C.oracle_runs(oracle_lib, i, variant)
    refs = [r["polished"] for r in runs]
    rb = _handle(lib, i, variant, large_factor=True, polish=True)  # setup with polish = 0, the switch, update_polish(True)
    twin = _handle(lib, i, variant)
    assert np.all(rb.polish_status() == 0)
    before = _counts(lib)
    x, y, info = rb.solve()  # polishes on its first solve
    st = rb.polish_status()
    x0, y0, info0 = twin.solve()
    assert _counts(lib) == (before[0] + 1, before[1], before[2])
    rb.solve()
    assert _counts(lib)[0] == before[0] + 2  # one per resolve
    rb.close(); twin.close()
    rst = np.array([r.info.status_polish for r in refs])
    both = [k for k in range(len(refs)) if st[k] == 1 and rst[k] == 1]
    ex = max([C.rel(x[k], refs[k].x) for k in both], default=0.0)
    ey = max([C.rel(y[k], refs[k].y) for k in both], default=0.0)
    er = max([max(abs(info[k, 2] - refs[k].info.pri_res), abs(info[k, 3] - refs[k].info.dua_res)) for k in both], default=0.0)
    eo = max([abs(info[k, 4] - refs[k].info.obj_val) / max(1.0, abs(refs[k].info.obj_val)) for k in both], default=0.0)
    moved = [C.rel(x[k], x0[k]) for k in both]
    print(f"{sid}/{C.VARIANT_IDS[variant]}: status {info[:, 1].astype(int).tolist()} status_polish gpu {st.astype(int).tolist()} oracle {rst.tolist()}; "
          f"polished vs oracle rel dx {ex:.2e} dy {ey:.2e} residuals {er:.2e} objective {eo:.2e} (bound {B:.1e}); polished vs unpolished x "
          f"{min(moved, default=0):.1e} .. {max(moved, default=0):.1e}")
    assert np.array_equal(info[:, 1], [r.info.status_val for r in refs])
    assert np.array_equal(st, rst)
    assert np.array_equal(info[:, [0, 1, 5]], info0[:, [0, 1, 5]])  # iter, status, rho_updates: the solve's
    assert len(both) >= 6
    assert ex <= B and ey <= B and er <= B and eo <= B, (ex, ey, er, eo, B)
    if i in C.CONSTRAINED:
        assert max(moved) > 100 * B, (max(moved), B)
    for k in range(len(refs)):
        if st[k] != 1:
            assert _same(x[k], x0[k]) and _same(y[k], y0[k]) and _same(info[k], info0[k]), (sid, k)


# ---- one handle per shape for the derivative tests ---------------------------------------------------------------------------
_runs = {}


def _run(lib, oracle_lib, i):
    """Default settings, polished resolve, then on that state: the adjoint (whole, NCOT cotangents, each alone) and the JVP
    (NDIR directions, each alone)."""
    if i not in _runs:
        probs = C.problems(i)[1]
        rb = _handle(lib, i, large_factor=True, polish=True)
        x, y, info = rb.solve()
        m = rb.m
        gx, gy = C.incoming(i)
        rng = np.random.default_rng(8000 + i)
        gx3, gy3 = np.concatenate([gx[None], rng.standard_normal((NCOT - 1,) + gx.shape)]), np.concatenate([gy[None], rng.standard_normal((NCOT - 1,) + gy.shape)])
        dy = lambda a: a if m else None
        g = rb.adjoint(dx=gx, dy=dy(gy))
        g3 = rb.adjoint(dx=gx3, dy=dy(gy3))
        g_alone = [rb.adjoint(dx=gx3[c], dy=dy(gy3[c])) for c in range(NCOT)]
        d = C.tangents(i, NDIR)
        if not m:
            d = {k: v for k, v in d.items() if k in ("q", "Px")}
        t = rb.jvp(**d)
        t_alone = [rb.jvp(**{k: v[j] for k, v in d.items()}) for j in range(NDIR)]
        _runs[i] = dict(rb=rb, probs=probs, x=x, y=y, info=info, gx=gx, gy=gy, gx3=gx3, gy3=gy3, g=g, g3=g3, g_alone=g_alone, d=d, t=t, t_alone=t_alone)
    return _runs[i]


# ---- adjoint ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", WITH_ROWS, ids=[C.SHAPE_IDS[i] for i in WITH_ROWS])
def test_adjoint_agrees_with_exact(product_lib, oracle_lib, i):
    r = _run(product_lib, oracle_lib, i)
    g, info, B = r["g"], r["info"], bound(i, "adjoint")
    solved = np.flatnonzero(info[:, 1] == 1)
    worst, used = 0.0, []
    for k in solved:
        P, q, A, l, u = r["probs"][k]
        if g["status"][k] != 1 or not adj.nondegenerate(A, g["act"][k], len(q)):
            continue
        want = adj.exact(P, A, r["x"][k], r["y"][k], g["act"][k], r["gx"][k], r["gy"][k])
        worst = max(worst, adj.rel_err({w: g[w][k] for w in adj.GRADS}, want))
        used.append(int(k))
    print(f"{C.SHAPE_IDS[i]}: Solved {len(solved)}, compared {used}, adjoint vs exact worst rel {worst:.2e} (bound {B:.1e})")
    assert len(solved) == C.COUNT and np.all(g["status"][solved] == 1)
    assert len(used) >= 5
    assert worst <= B, worst


@pytest.mark.parametrize("i", WITH_ROWS, ids=[C.SHAPE_IDS[i] for i in WITH_ROWS])
def test_adjoint_cotangents_forms_and_rows(product_lib, oracle_lib, i):
    lib = product_lib
    r = _run(lib, oracle_lib, i)
    rb, g, g3 = r["rb"], r["g"], r["g3"]
    # cotangent c of an ncot call: the bits of a one-cotangent call (cotangent 0 is the pair of `g`)
    for c, one in enumerate(r["g_alone"]):
        for w in adj.GRADS:
            assert g3[w].shape == (NCOT,) + one[w].shape and _same(g3[w][c], one[w]), (c, w)
        assert _same(g3["act"], one["act"]) and _same(g3["status"], one["status"])
    assert all(_same(g3[w][0], g[w]) for w in adj.GRADS)
    # host and device forms
    cols = dict(q=rb.n, l=rb.m, u=rb.m, Px=rb.nnzP, Ax=rb.nnzA, act=rb.m, status=1)
    dev = {k: batch.DeviceArray(lib, rb.count, c) for k, c in cols.items()}
    dgx, dgy = (batch.DeviceArray(lib, *a.shape).upload(a) for a in (r["gx"], r["gy"]))
    assert rb.adjoint(dx=dgx, dy=dgy, out=dev) is dev
    for k in cols:
        assert _same(dev[k].numpy().reshape(g[k].shape), g[k]), k
    for a in list(dev.values()) + [dgx, dgy]:
        a.free()
    # a selection of two instances: the rows of the whole call
    sel = [5, 2]
    part = rb.adjoint(dx=r["gx"][sel], dy=r["gy"][sel], rows=sel)
    for k in part:
        assert _same(part[k], g[k][sel]), k
    assert _same_all(rb.adjoint(dx=r["gx"], dy=r["gy"]).values(), g.values())  # a second call: the bits of the first


def test_adjoint_refuses_a_stale_instance_by_name_without_a_launch(product_lib, oracle_lib):
    lib = product_lib
    rb = _handle(lib, 1, large_factor=True)
    rb.solve()
    gx, gy = C.incoming(1)
    q = C.problems(1)[0][4]
    rb.update(q=q[[3]] * 1.01, rows=[3])
    before = _counts(lib)
    with pytest.raises(oq.OSQPError, match="instance 3 of the batch holds no current solution"):
        rb.adjoint(dx=gx, dy=gy)
    with pytest.raises(oq.OSQPError, match="instance 3 of the batch holds no current solution"):
        rb.jvp(q=gx)
    assert _counts(lib) == before
    assert np.all(rb.adjoint(dx=gx[[0, 1]], dy=gy[[0, 1]], rows=[0, 1])["status"] == 1)  # the others are current
    rb.close()


# ---- JVP -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", WITH_ROWS, ids=[C.SHAPE_IDS[i] for i in WITH_ROWS])
def test_jvp_agrees_with_exact_and_with_the_adjoint(product_lib, oracle_lib, i):
    r = _run(product_lib, oracle_lib, i)
    t, g, d, info = r["t"], r["g"], r["d"], r["info"]
    B, BD = bound(i, "jvp"), bound(i, "jvp") + bound(i, "adjoint")
    solved = np.flatnonzero(info[:, 1] == 1)
    worst = gap = 0.0
    used = []
    for k in solved:
        P, q, A, l, u = r["probs"][k]
        if t["status"][k] != 1 or not jv.nondegenerate(A, t["act"][k], len(q)):
            continue
        used.append(int(k))
        for j in range(NDIR):
            dk = jv.direction(d, j, k)
            worst = max(worst, jv.rel_err(t["x"][j, k], t["y"][j, k], *jv.exact(P, A, r["x"][k], r["y"][k], t["act"][k], dk)))
        # <g, J d> = <J' g, d> with the device adjoint of (gx, gy), relative to the sum of the |terms| of both sides
        gap = max(gap, jv.duality_gap(r["gx"][k], r["gy"][k], t["x"][0, k], t["y"][0, k], {w: g[w][k] for w in adj.GRADS}, jv.direction(d, 0, k)))
    print(f"{C.SHAPE_IDS[i]}: compared {used}, jvp vs exact worst rel {worst:.2e} (bound {B:.1e}), duality with the adjoint {gap:.2e} (bound {BD:.1e})")
    assert t["x"].shape == (NDIR,) + r["x"].shape and t["y"].shape == (NDIR,) + r["y"].shape
    assert np.all(t["status"][solved] == 1) and _same(t["act"], g["act"])
    assert len(used) >= 5
    assert worst <= B, worst
    assert gap <= BD, gap
    for j, one in enumerate(r["t_alone"]):  # the directions are independent
        assert _same(t["x"][j], one["x"]) and _same(t["y"][j], one["y"]), j
        assert _same(t["act"], one["act"]) and _same(t["status"], one["status"])


def test_jvp_forms_and_rows(product_lib, oracle_lib):
    lib = product_lib
    r = _run(lib, oracle_lib, 3)
    rb, t, d = r["rb"], r["t"], r["d"]
    sel = [6, 1]
    part = rb.jvp(**{k: v[:, sel] for k, v in d.items()}, rows=sel)
    assert _same(part["x"], t["x"][:, sel]) and _same(part["y"], t["y"][:, sel]) and _same(part["act"], t["act"][sel])
    one = {k: batch.DeviceArray(lib, rb.count, v.shape[2]).upload(v[0]) for k, v in d.items()}
    out = dict(x=batch.DeviceArray(lib, rb.count, rb.n), y=batch.DeviceArray(lib, rb.count, rb.m))
    rb.jvp(**one, out=out)
    assert _same(out["x"].numpy(), t["x"][0]) and _same(out["y"].numpy(), t["y"][0])
    for a in list(one.values()) + list(out.values()):
        a.free()


def test_jacobian_forward_and_reverse_agree(product_lib, oracle_lib):
    r = _run(product_lib, oracle_lib, 0)  # n = 129
    rb = r["rb"]
    rows3 = {"x": [0, 64, 128]}
    B = bound(0, "jvp") + bound(0, "adjoint")
    auto = rb.jacobian(of=("x",), wrt=("q", "l"), mode="auto", out_rows=rows3)
    fwd = rb.jacobian(of=("x",), wrt=("q", "l"), mode="forward", out_rows=rows3)
    rev = rb.jacobian(of=("x",), wrt=("q", "l"), mode="reverse", out_rows=rows3)
    worst = 0.0
    for key in (("x", "q"), ("x", "l")):
        assert auto[key].shape == (rb.count, 3, rb.n if key[1] == "q" else rb.m)
        assert _same(auto[key], rev[key])  # three cotangents against n + m directions: reverse
        worst = max(worst, C.rel(fwd[key], rev[key]))
    print(f"jacobian n = 129: forward vs reverse worst rel {worst:.2e} (bound {B:.1e})")
    assert np.all(auto["status"] == 1)
    assert worst <= B, worst


# ---- no constraints, a single row --------------------------------------------------------------------------------------------
def test_a_batch_without_constraints(product_lib, oracle_lib):
    i = 6
    lib = product_lib
    r = _run(lib, oracle_lib, i)
    g, t, x = r["g"], r["t"], r["x"]
    refs = [q["polished"] for q in C.oracle_runs(oracle_lib, i)]
    assert sorted(g) == ["Px", "q", "status"] and sorted(t) == ["status", "x"]
    assert np.all(r["info"][:, 1] == 1) and np.all(g["status"] == 1) and np.all(t["status"] == 1)
    ex = max(C.rel(x[k], refs[k].x) for k in range(C.COUNT))
    ea = ej = 0.0
    for k, (P, q, A, l, u) in enumerate(r["probs"]):
        none = np.zeros(0)
        want = adj.exact(P, A, x[k], none, np.zeros(0, int), r["gx"][k], none)
        ea = max(ea, adj.rel_err(dict(q=g["q"][k], Px=g["Px"][k], l=[], u=[], Ax=[]), want))
        for j in range(NDIR):
            dk = dict(q=r["d"]["q"][j, k], Px=r["d"]["Px"][j, k])
            ej = max(ej, C.rel(t["x"][j, k], jv.exact(P, A, x[k], none, np.zeros(0, int), dk)[0]))
    print(f"m = 0: polished x vs oracle {ex:.2e} (bound {bound(i, 'polish'):.1e}), adjoint {ea:.2e} ({bound(i, 'adjoint'):.1e}), jvp {ej:.2e} ({bound(i, 'jvp'):.1e})")
    assert ex <= bound(i, "polish") and ea <= bound(i, "adjoint") and ej <= bound(i, "jvp")
    for c, one in enumerate(r["g_alone"]):
        assert _same(r["g3"]["q"][c], one["q"]) and _same(r["g3"]["Px"][c], one["Px"])


def test_a_single_row(product_lib, oracle_lib):
    r = _run(product_lib, oracle_lib, 5)
    g, t = r["g"], r["t"]
    assert g["l"].shape == (C.COUNT, 1) and t["y"].shape == (NDIR, C.COUNT, 1)
    active = g["act"][:, 0] != 0
    print("m = 1: act", g["act"][:, 0].tolist())
    assert np.all(g["l"][~active] == 0) and np.all(g["u"][~active] == 0) and np.all(t["y"][:, ~active] == 0)
    assert np.all(g["l"][g["act"][:, 0] > 0] == 0) and np.all(g["u"][g["act"][:, 0] < 0] == 0)


# ---- the scratch is the solve's --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 3], ids=[C.SHAPE_IDS[0], C.SHAPE_IDS[3]])
def test_the_scratch_is_shared_with_the_solve(product_lib, oracle_lib, i):
    """The factor is built where the solve kernel keeps its inverse.  rb: solve, adjoint, JVP, a polishing resolve, then -- cold,
    so that the polished record does not enter -- adjoint and JVP once more and a plain solve; twin: the three solves alone.
    The plain solves agree bit for bit, a second adjoint returns the bits of the first, and so does a handle whose scratch
    has held nothing but the solve's inverse."""
    lib = product_lib
    gx, gy = C.incoming(i)
    rb, twin = _handle(lib, i, large_factor=True), _handle(lib, i)
    assert _same_all(rb.solve(), twin.solve())
    g1 = rb.adjoint(dx=gx, dy=gy)
    rb.jvp(q=gx)
    rb.update_polish(True)
    polished = rb.solve()
    plain = twin.solve()
    assert np.all(rb.polish_status() == 1) and not _same(polished[0], plain[0])
    rb.update_polish(False)
    rb.update_settings(warm_start=False); twin.update_settings(warm_start=False)
    g2 = rb.adjoint(dx=gx, dy=gy)
    rb.jvp(q=gx)
    assert _same_all(rb.adjoint(dx=gx, dy=gy).values(), g2.values())
    assert _same_all(rb.solve(), twin.solve())
    rb.close(); twin.close()
    fresh = _handle(lib, i, large_factor=True)
    fresh.solve()
    assert _same_all(fresh.adjoint(dx=gx, dy=gy).values(), g1.values())
    fresh.close()


# ---- life cycle ------------------------------------------------------------------------------------------------------------------
def test_life_cycle_of_the_switch(product_lib, oracle_lib):
    lib = product_lib
    gx, gy = C.incoming(1)
    rb = _handle(lib, 1)
    twin = _handle(lib, 1)
    first = rb.solve()
    assert _same_all(first, twin.solve())

    def refused():
        before = _counts(lib)
        with pytest.raises(oq.OSQPError, match=MSG):
            rb.adjoint(dx=gx, dy=gy)
        with pytest.raises(oq.OSQPError, match=MSG):
            rb.jvp(q=gx)
        with pytest.raises(oq.OSQPError, match=MSG):
            rb.update_polish(True)
        assert _counts(lib) == before

    refused()
    assert rb.large_factor(True) is False
    before = _counts(lib)
    g = rb.adjoint(dx=gx, dy=gy)
    t = rb.jvp(q=gx)
    rb.update_polish(True)
    assert np.all(g["status"] == 1) and np.all(t["status"] == 1)
    assert _counts(lib) == (before[0], before[1] + 1, before[2] + 1)
    assert rb.large_factor(False) is True
    refused()
    assert _same_all(rb.solve(), twin.solve())  # polish went off with the switch: the plain solve, the same bits
    assert np.all(rb.polish_status() == 0)
    rb.close(); twin.close()
    small = batch.ResidentBatch(lib, *C.F.instances(C.F.pattern("banded", (128, 192, 4)), 2, 1)[0], **C.F.OPTS)
    with pytest.raises(oq.OSQPError, match="128 < n <= 256"):
        small.large_factor(True)
    small.close()


# ---- torch -----------------------------------------------------------------------------------------------------------------------
def test_torch_layer_backward_and_forward_mode(product_lib, oracle_lib):
    import torch
    from torch.autograd import forward_ad

    from osqp_jl_amd.qp_layer import BatchQPLayer

    args = C.problems(1)[0]
    rb = _handle(product_lib, 1)
    layer = BatchQPLayer(rb, large=True, large_factor=True)
    dev = torch.device("cuda:0")
    q = torch.tensor(args[4], device=dev, requires_grad=True)
    x, _ = layer(q=q)
    x.sum().backward()
    assert _same(q.grad.cpu().numpy(), rb.adjoint(dx=np.ones((rb.count, rb.n)), want=("q",))["q"])
    tq = C.incoming(1)[0]
    with forward_ad.dual_level():
        xd, _ = layer(q=forward_ad.make_dual(q.detach(), torch.tensor(tq, device=dev)))
        tx = forward_ad.unpack_dual(xd).tangent
        assert tx is not None and _same(tx.cpu().numpy(), rb.jvp(q=tq)["x"])
    rb.close()


def test_close_the_shared_handles():
    for r in _runs.values():
        r["rb"].close()
    _runs.clear()
