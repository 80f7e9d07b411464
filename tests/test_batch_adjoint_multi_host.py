"""The host side of several cotangents per adjoint launch (osqp_amd_batch_adjoint_multi, _multi_rows; the leading axis of
`ResidentBatch.adjoint`) and of `ResidentBatch.jacobian`, without a GPU:
(a) the declarations of the two entry points, and what `adjoint` hands to the library -- on a handle without a device, with
    the recording stand-in of test_batch_subset_deriv_host.py;
(b) the assembly of `jacobian`, with `adjoint` / `jvp` of the handle replaced by numpy stand-ins built on
    `batch_adjoint_ref.exact` and `batch_jvp_ref.exact`: reverse and forward mode against each other's keys and shapes and
    against the Jacobian built column by column from central differences of `active_set_solution` in q, l, u.  The solution
    of a fixed active set is affine in these, so h = 1e-4 has no truncation error; the bound and the instance counts are
    those of test_batch_adjoint_host.py (a): 100 x MEASURED_A[family], MIN_NONDEGENERATE;
(c) unit cotangents -- what `jacobian` feeds the kernel -- stay inside the family bounds of the kernel's model: `model`
    against `exact` with every e_j of (x, y), <= 1000 x MEASURED_C[family] (the GPU test's bound).
Measured when this file was written, worst figure (bound):
  (b) reverse / forward against differences: tiny 5.6e-12 / 5.6e-12 (1.3e-6), ineq 2.7e-10 / 2.7e-10 (5.5e-7)
  (c) tiny 1.1e-15 (1.0e-12), ineq 3.4e-14 (8.9e-12), wide300 3.1e-12 (3.3e-9), tri128 2.6e-14 (8.7e-12)"""
import os

import numpy as np
import pytest

from osqp_jl_amd import batch
from osqp_jl_amd import types as T
import batch_adjoint_ref as adj
import batch_jvp_ref as jv
from test_batch_adjoint_host import MEASURED_A, MEASURED_C, _usable
from test_batch_subset_deriv_host import COUNT, M, N, NNZA, NNZP, _Dev, _handle

MULTI_SYMBOLS = {"osqp_amd_batch_adjoint_multi": 12, "osqp_amd_batch_adjoint_multi_rows": 14}


# ---- (a) declarations and what the library is handed ----
def test_the_two_entries_are_declared():
    """ncot before the arrays; the *_rows form has rows, k directly after the handle and ncot next."""
    for name, nargs in MULTI_SYMBOLS.items():
        assert name in T.EXT_SYMBOLS, name
        restype, argtypes = T.EXT_SYMBOLS[name]
        assert restype is T.c_int and len(argtypes) == nargs and argtypes[-1] is T.c_int, (name, argtypes)
    whole, rows = (T.EXT_SYMBOLS[name][1] for name in MULTI_SYMBOLS)
    assert whole[1] is T.c_int and whole[:1] + whole[2:] == T.EXT_SYMBOLS["osqp_amd_batch_adjoint"][1]
    assert rows[1] is T.c_int_p and rows[2] is T.c_int and rows[3] is T.c_int and rows[:1] + rows[3:] == whole
    assert rows[:3] + rows[4:] == T.EXT_SYMBOLS["osqp_amd_batch_adjoint_rows"][1]


def test_the_header_declares_them():
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "osqp_amd.h")).read()
    assert "c_int osqp_amd_batch_adjoint_multi(osqp_amd_batch *batch, c_int ncot, const c_float *dx, const c_float *dy," in header
    assert "c_int osqp_amd_batch_adjoint_multi_rows(osqp_amd_batch *batch, const c_int *rows, c_int k, c_int ncot, const c_float *dx," in header


def test_the_library_exports_them(product_lib):
    for name in MULTI_SYMBOLS:
        fn = getattr(product_lib, name)  # AttributeError: not exported
        assert fn.restype is T.c_int and list(fn.argtypes) == list(T.EXT_SYMBOLS[name][1])
    buf = np.zeros(4)
    before = product_lib.osqp_amd_batch_adjoint_launches()
    assert product_lib.osqp_amd_batch_adjoint_multi(None, 2, buf.ctypes.data, None, buf.ctypes.data, None, None, None, None, None, None, 0) == 1
    assert b"handle" in product_lib.osqp_amd_last_error()
    assert product_lib.osqp_amd_batch_adjoint_launches() == before


def test_three_dimensional_cotangents_call_the_multi_entries():
    rb = _handle()
    dx, dy = np.ones((3, COUNT, N)), np.ones((3, COUNT, M))
    g = rb.adjoint(dx=dx, dy=dy)
    (name, k, got, rest), = rb.lib.calls
    assert name == "osqp_amd_batch_adjoint_multi" and k is None
    assert len(rest) == 11 and rest[0] == 3 and rest[-1] == 0 and all(p is not None for p in rest[1:10])
    assert {key: g[key].shape for key in g} == dict(q=(3, COUNT, N), l=(3, COUNT, M), u=(3, COUNT, M), Px=(3, COUNT, NNZP),
                                                      Ax=(3, COUNT, NNZA), act=(COUNT, M), status=(COUNT,))
    assert g["act"].dtype == np.int64 and g["status"].dtype == np.int64
    rb.lib.calls.clear()
    sel = [6, 0]
    g = rb.adjoint(dx=np.ones((4, 2, N)), want=("q", "Ax"), rows=sel)  # a selection, a want subset, no dy
    (name, k, got, rest), = rb.lib.calls
    assert name == "osqp_amd_batch_adjoint_multi_rows" and k == 2 and got == sel
    assert len(rest) == 11 and rest[0] == 4 and rest[1] is not None and rest[2] is None
    assert rest[3] is not None and rest[4:7] == (None,) * 3 and rest[7] is not None
    assert {key: g[key].shape for key in g} == dict(q=(4, 2, N), Ax=(4, 2, NNZA), act=(2, M), status=(2,))
    rb.lib.calls.clear()
    g = rb.adjoint(dy=np.ones((1, COUNT, M)), want=("l",))  # one cotangent with a leading axis is still the multi entry
    assert rb.lib.calls[0][0] == "osqp_amd_batch_adjoint_multi" and rb.lib.calls[0][3][0] == 1 and g["l"].shape == (1, COUNT, M)


def test_two_dimensional_cotangents_call_the_old_entries_with_their_old_arguments():
    rb = _handle()
    dx, dy = np.ones((COUNT, N)), np.ones((COUNT, M))
    g = rb.adjoint(dx=dx, dy=dy)
    gs = rb.adjoint(dx=dx[:2], rows=[5, 1], want=("q",))
    (n1, k1, s1, r1), (n2, k2, s2, r2) = rb.lib.calls
    assert n1 == "osqp_amd_batch_adjoint" and len(r1) == 10 and r1[0] == dx.ctypes.data and r1[1] == dy.ctypes.data and r1[-1] == 0
    assert n2 == "osqp_amd_batch_adjoint_rows" and (k2, s2) == (2, [5, 1]) and len(r2) == 10 and r2[1] is None
    assert g["q"].shape == (COUNT, N) and gs["q"].shape == (2, N) and gs["status"].shape == (2,)


def test_device_form_with_a_leading_axis():
    rb = _handle()
    out = dict(q=_Dev(2, COUNT, N), Ax=_Dev(2, COUNT, NNZA), act=_Dev(COUNT, M), status=_Dev(COUNT, 1))
    assert rb.adjoint(dx=_Dev(2, COUNT, N), dy=_Dev(2, COUNT, M), want=("q", "Ax"), out=out) is out
    (name, k, got, rest), = rb.lib.calls
    assert name == "osqp_amd_batch_adjoint_multi" and rest[0] == 2 and rest[-1] == 1 and rest[1:4] == (4096,) * 3
    out_rows = dict(q=_Dev(2, 3, N))
    assert rb.adjoint(dx=_Dev(2, 3, N), want=("q",), out=out_rows, rows=[4, 0, 2]) is out_rows
    assert rb.lib.calls[1][0] == "osqp_amd_batch_adjoint_multi_rows" and rb.lib.calls[1][3][0] == 2


def test_shape_errors_are_raised_before_the_library_is_called():
    rb = _handle()
    with pytest.raises(ValueError, match="dimensions"):  # mixed dimensions
        rb.adjoint(dx=np.ones((2, COUNT, N)), dy=np.ones((COUNT, M)))
    with pytest.raises(ValueError, match="dimensions"):
        rb.adjoint(dx=np.ones((1, 2, COUNT, N)))
    with pytest.raises(ValueError, match="same number of cotangents"):  # differing ncot
        rb.adjoint(dx=np.ones((2, COUNT, N)), dy=np.ones((3, COUNT, M)))
    with pytest.raises(ValueError, match="ncot"):  # ncot = 0
        rb.adjoint(dx=np.ones((0, COUNT, N)))
    with pytest.raises(ValueError, match="ncot"):
        rb.adjoint(dx=_Dev(0, COUNT, N), want=("q",), out=dict(q=_Dev(0, COUNT, N)))
    with pytest.raises(ValueError, match="dx"):  # the whole batch's rows with a selection
        rb.adjoint(dx=np.ones((2, COUNT, N)), rows=[1, 2])
    with pytest.raises(ValueError, match=r"out\['q'\]"):  # an `out` without the leading axis
        rb.adjoint(dx=_Dev(2, COUNT, N), want=("q",), out=dict(q=_Dev(COUNT, N)))
    with pytest.raises(ValueError, match=r"out\['Ax'\]"):  # ... with another ncot
        rb.adjoint(dx=_Dev(2, COUNT, N), want=("q", "Ax"), out=dict(q=_Dev(2, COUNT, N), Ax=_Dev(3, COUNT, NNZA)))
    with pytest.raises(ValueError, match=r"out\['act'\]"):  # act is per instance
        rb.adjoint(dx=_Dev(2, COUNT, N), want=("q",), out=dict(q=_Dev(2, COUNT, N), act=_Dev(2, COUNT, M)))
    with pytest.raises(ValueError, match="both"):  # host and device mixed
        rb.adjoint(dx=_Dev(2, COUNT, N), dy=np.ones((2, COUNT, M)), out=dict(q=_Dev(2, COUNT, N)))
    assert rb.lib.calls == []


# ---- (b) the assembly of jacobian ----
class _Exact:
    """A handle whose `adjoint` and `jvp` are the exact dense solves on the active-set solutions of the non-degenerate
    instances of a family; the calls are counted by the number of solves they carry."""

    def __init__(self, oracle_lib, family):
        self.use = _usable(oracle_lib, family)
        self.sols = [adj.active_set_solution(*p, s["act"]) for _, p, s in self.use]
        self.rb = rb = object.__new__(batch.ResidentBatch)
        P, q, A, l, u = self.use[0][1]
        (pi, _), (ai, _) = adj.patterns(P, A)
        rb.n, rb.m, rb.nnzP, rb.nnzA, rb.count = len(q), len(l), len(pi), len(ai), len(self.use)
        rb.lib, rb.handle, rb.device = None, None, 0
        rb.adjoint, rb.jvp = self.adjoint, self.jvp
        self.solves = dict(adjoint=[], jvp=[])

    def _rows(self, rows):
        return range(len(self.use)) if rows is None else [int(i) for i in rows]

    def adjoint(self, dx=None, dy=None, want=adj.GRADS, out=None, rows=None):
        rows, rb = self._rows(rows), self.rb
        first = dx if dx is not None else dy
        ncot = first.shape[0]
        assert first.ndim == 3 and first.shape[1] == len(rows) and out is None
        self.solves["adjoint"].append(ncot)
        cols = dict(q=rb.n, l=rb.m, u=rb.m, Px=rb.nnzP, Ax=rb.nnzA)
        res = {k: np.empty((ncot, len(rows), cols[k])) for k in want}
        act = np.empty((len(rows), rb.m), dtype=np.int64)
        for p, i in enumerate(rows):
            (_, (P, q, A, l, u), s), (x, y) = self.use[i], self.sols[i]
            act[p] = s["act"]
            for c in range(ncot):
                g = adj.exact(P, A, x, y, s["act"], np.zeros(rb.n) if dx is None else dx[c, p], np.zeros(rb.m) if dy is None else dy[c, p])
                for k in want:
                    res[k][c, p] = g[k]
        res.update(act=act, status=np.ones(len(rows), dtype=np.int64))
        return res

    def jvp(self, q=None, l=None, u=None, Px=None, Ax=None, out=None, rows=None):
        rows, rb = self._rows(rows), self.rb
        given = {k: v for k, v in zip(jv.TANGENTS, (q, l, u, Px, Ax)) if v is not None}
        ndir = next(iter(given.values())).shape[0]
        assert all(v.ndim == 3 and v.shape[:2] == (ndir, len(rows)) for v in given.values()) and out is None
        self.solves["jvp"].append(ndir)
        res = dict(x=np.empty((ndir, len(rows), rb.n)), y=np.empty((ndir, len(rows), rb.m)))
        act = np.empty((len(rows), rb.m), dtype=np.int64)
        for p, i in enumerate(rows):
            (_, (P, pq, A, pl, pu), s), (x, y) = self.use[i], self.sols[i]
            act[p] = s["act"]
            for d in range(ndir):
                res["x"][d, p], res["y"][d, p] = jv.exact(P, A, x, y, s["act"], {k: v[d, p] for k, v in given.items()})
        res.update(act=act, status=np.ones(len(rows), dtype=np.int64))
        return res

    def differences(self, h=1e-4):
        """{(o, w): [count x cols(o) x cols(w)]} for o in (x, y), w in (q, l, u), column by column from central differences
        of the active-set solution."""
        rb = self.rb
        cols = dict(q=rb.n, l=rb.m, u=rb.m)
        J = {(o, w): np.empty((rb.count, dict(x=rb.n, y=rb.m)[o], cols[w])) for o in ("x", "y") for w in cols}
        for i, (_, (P, q, A, l, u), s) in enumerate(self.use):
            base = dict(q=q, l=l, u=u)
            for w in cols:
                for b in range(cols[w]):
                    e = np.zeros(cols[w]); e[b] = h
                    (xp, yp), (xm, ym) = (adj.active_set_solution(P, *(base[k] + (sign * e if k == w else 0.0) for k in ("q",)), A,
                                                                  *(base[k] + (sign * e if k == w else 0.0) for k in ("l", "u")), s["act"])
                                          for sign in (1.0, -1.0))
                    J[("x", w)][i, :, b], J[("y", w)][i, :, b] = (xp - xm) / (2 * h), (yp - ym) / (2 * h)
        return J


_exact = {}


def _family(oracle_lib, family):
    if family not in _exact:
        e = _Exact(oracle_lib, family)
        _exact[family] = (e, e.differences())
    return _exact[family]


def _worst(J, want):
    return max(float(np.max(np.abs(J[key] - want[key]))) / max(1.0, float(np.max(np.abs(want[key])))) for key in want)


@pytest.mark.parametrize("family", ["tiny", "ineq"])
def test_jacobian_in_both_modes_agrees_with_differences_of_the_active_set_solution(oracle_lib, family):
    e, fd = _family(oracle_lib, family)
    rb = e.rb
    rev = rb.jacobian(of=("x", "y"), wrt=("q", "l", "u"), mode="reverse")
    fwd = rb.jacobian(of=("x", "y"), wrt=("q", "l", "u"), mode="forward")
    assert sorted(map(str, rev)) == sorted(map(str, fwd)) == sorted(map(str, list(fd) + ["act", "status"]))
    for key in fd:
        assert rev[key].shape == fwd[key].shape == fd[key].shape, key
    assert rev["act"].shape == fwd["act"].shape == (rb.count, rb.m) and rev["status"].shape == fwd["status"].shape == (rb.count,)
    assert np.array_equal(rev["act"], np.array([s["act"] for _, _, s in e.use])) and np.all(rev["status"] == 1)
    w_rev, w_fwd = _worst(rev, fd), _worst(fwd, fd)
    print(f"(b) {family}: {rb.count} instances, jacobian vs central differences worst rel: reverse {w_rev:.2e}, forward {w_fwd:.2e} "
          f"(bound {100 * MEASURED_A[family]:.1e})")
    assert rb.count >= adj.MIN_NONDEGENERATE[family]
    assert w_rev <= 100 * MEASURED_A[family], w_rev
    assert w_fwd <= 100 * MEASURED_A[family], w_fwd


def test_jacobian_out_rows_chunks_and_selection(oracle_lib):
    e, _ = _family(oracle_lib, "tiny")
    rb = e.rb
    for mode in ("reverse", "forward"):
        full = rb.jacobian(of=("x", "y"), wrt=("q", "u"), mode=mode)
        e.solves["adjoint"].clear(); e.solves["jvp"].clear()
        one = rb.jacobian(of=("x", "y"), wrt=("q", "u"), mode=mode, chunk=1)  # independent launches, concatenated
        assert sorted(map(str, one)) == sorted(map(str, full)) and all(np.array_equal(one[k], full[k]) for k in full), mode
        total = rb.n + rb.m
        assert e.solves == (dict(adjoint=[1] * total, jvp=[]) if mode == "reverse" else dict(adjoint=[], jvp=[1] * total))
        e.solves["adjoint"].clear(); e.solves["jvp"].clear()
        rb.jacobian(of=("x", "y"), wrt=("q", "u"), mode=mode, chunk=3)  # a chunk that straddles the two segments
        assert e.solves["adjoint" if mode == "reverse" else "jvp"] == [3, 3, 2]
        pick = dict(x=[4, 1], y=[2])
        part = rb.jacobian(of=("x", "y"), wrt=("q", "u"), mode=mode, out_rows=pick)
        for (o, w) in [(o, w) for o in ("x", "y") for w in ("q", "u")]:
            assert part[(o, w)].shape == (rb.count, len(pick[o]), dict(q=rb.n, u=rb.m)[w])
            assert np.array_equal(part[(o, w)], full[(o, w)][:, pick[o], :]), (mode, o, w)
        sel = [rb.count - 1, 0, 2]
        some = rb.jacobian(of=("x",), wrt=("l",), mode=mode, rows=sel, out_rows=dict(x=[3]))
        assert sorted(map(str, some)) == sorted(map(str, [("x", "l"), "act", "status"])) and some["status"].shape == (3,)
        assert np.array_equal(some[("x", "l")], rb.jacobian(of=("x",), wrt=("l",), mode=mode)[("x", "l")][sel][:, [3], :])


def test_auto_takes_the_mode_with_fewer_solves(oracle_lib):
    e, _ = _family(oracle_lib, "tiny")
    rb = e.rb  # n = 5, m = 3
    for kw, mode, solves in ((dict(of=("x",), wrt=("q", "l", "u")), "adjoint", 5),  # 5 outputs against 11 columns
                             (dict(of=("x", "y"), wrt=("q",)), "jvp", 5),  # 8 outputs against 5 columns
                             (dict(of=("x", "y"), wrt=("q", "l", "u"), out_rows=dict(x=[0], y=[1, 2])), "adjoint", 3),
                             (dict(of=("x",), wrt=("q",)), "adjoint", 5)):  # a tie: reverse
        e.solves["adjoint"].clear(); e.solves["jvp"].clear()
        auto = rb.jacobian(**kw)
        assert e.solves == {mode: [solves], ("jvp" if mode == "adjoint" else "adjoint"): []}, kw
        named = rb.jacobian(mode="reverse" if mode == "adjoint" else "forward", **kw)
        assert all(np.array_equal(auto[k], named[k]) for k in named)


def test_jacobian_checks_its_arguments(oracle_lib):
    e, _ = _family(oracle_lib, "tiny")
    rb = e.rb
    e.solves["adjoint"].clear(); e.solves["jvp"].clear()
    for kw, word in ((dict(of=("z",)), "of"), (dict(of=()), "of"), (dict(wrt=("q", "x")), "wrt"), (dict(mode="both"), "mode"),
                     (dict(out_rows=dict(y=[0])), "out_rows"), (dict(out_rows=dict(x=[5])), "out_rows"),
                     (dict(out_rows=dict(x=[0.5])), "out_rows"), (dict(chunk=0), "chunk"), (dict(rows=[0, 0]), "repeated")):
        with pytest.raises(ValueError, match=word):
            rb.jacobian(**kw)
    assert e.solves == dict(adjoint=[], jvp=[])


# ---- (c) unit cotangents stay inside the family bounds ----
@pytest.mark.parametrize("family,step", [("tiny", 1), ("ineq", 1), ("wide300", 7), ("tri128", 7)])
def test_model_agrees_with_exact_on_unit_cotangents(oracle_lib, family, step):
    use = _usable(oracle_lib, family)
    worst = 0.0
    for i, (P, q, A, l, u), s in use:
        n, m = len(q), len(l)
        for j in range(0, n + m, step):
            e = np.zeros(n + m); e[j] = 1.0
            got = adj.model(P, q, A, l, u, *s["state"], e[:n], e[n:])
            assert got["status"] == 1
            worst = max(worst, adj.rel_err(got, adj.exact(P, A, got["x"], got["y"], got["act"], e[:n], e[n:])))
    print(f"(c) {family}: {len(use)} instances, every {step}th unit cotangent, model vs exact worst rel {worst:.2e} "
          f"(bound {1000 * MEASURED_C[family]:.1e})")
    assert len(use) >= adj.MIN_NONDEGENERATE[family]
    assert worst <= 1000 * MEASURED_C[family], worst
