"""Inputs of the tests of polish, adjoint and JVP on resident handles with 128 < n <= 256 (osqp_amd_batch_large_factor, DESIGN.md
section 13.2; test_batch_large_factor_host.py, test_batch_large_factor_gpu.py; not a test module): the shapes -- the six of
batch_large_cases.py and an n = 130 batch without constraints --, the Python transcription of the LDS layout of the LARGE forms
of the three kernels (csrc/batch_polish.hpp make_layout with csrc/batch_large_factor.hpp lds_doubles), the oracle runs the
tests share (once per process, never modified) and the figures of the three numpy models against their references.  No GPU
needed."""
import functools

import numpy as np
import scipy.sparse as sp

import osqp_jl_amd as oq
import batch_adjoint_ref as adj
import batch_entry_families as F
import batch_jvp_ref as jv
import batch_large_cases as L
import batch_polish_ref as pol

COUNT = L.COUNT
NOCON = ("nocon", (130,), 3006)                      # n = 130, m = 0: the pattern of P of random(130, 1, 7), no rows
SHAPES = list(L.SHAPES) + [NOCON]
SHAPE_IDS = list(L.SHAPE_IDS) + ["nocon-130"]
CONSTRAINED = [0, 1, 2, 3, 4]                        # the shapes whose polish moves x by far more than the bound
VARIANTS = [dict(), dict(scaling=0), dict(scaled_termination=1)]
VARIANT_IDS = ["default", "unscaled", "scaled_termination"]
ALL_VARIANTS = [0, 3, 4]                             # n = 129 and both n = 256 shapes run the three variants, the rest the first
NB, PT, LDS_LIMIT = 32, 256, 160 * 1024


def pattern(i):
    kind, args, _ = SHAPES[i]
    if kind == "nocon":
        pat_P, _ = F.random(args[0], 1, 7)
        return F._finish(pat_P, sp.csc_matrix((0, args[0])))
    return F.pattern(kind, args)


@functools.lru_cache(None)
def problems(i, count=COUNT):
    """(what ResidentBatch takes, [(P, q, A, l, u)]) of shape i: the instances of the solve tests (batch_large_cases)."""
    return F.instances(pattern(i), count, SHAPES[i][2])


def lds_bytes(n, m, nnzA, nnzF):
    """make_layout(n, m, nnzA, nnzF, large = true): every slot rounded up to an even number of doubles; in the slot of M the
    panel [NB x (n | 1)], its pivots [NB], the inverse of a diagonal block [NB x NB] and a block result [NB]."""
    even = lambda k: (k + 1) & ~1
    work = NB * (n | 1) + NB + NB * NB + NB
    return 8 * (even(work) + even(nnzA) + even(nnzF) + 5 * even(n) + 6 * even(m) + even(4 * (PT // 64)))


def opts_of(variant):
    return dict(F.OPTS, **VARIANTS[variant])


# ---- the oracle, once per (shape, variant) ------------------------------------------------------------------------------------
_runs = {}


def oracle_runs(oracle_lib, i, variant=0):
    """Per instance of shape i under VARIANTS[variant]: dict(plain, polished (results of a polish = 0 / polish = 1 model),
    state0 (D, E, c and the scaled iterate the polish = 0 solve left), state1 (the same of the polish = 1 model), act (the
    classification of state1 by the rule of the derivative kernels))."""
    key = (i, variant)
    if key not in _runs:
        opts, out = opts_of(variant), []
        scaling = opts.get("scaling", 10)
        for P, q, A, l, u in problems(i)[1]:
            plain, polished = oq.Model(oracle_lib), oq.Model(oracle_lib)
            oq.setup(plain, P=P, q=q, A=A, l=l, u=u, polish=False, **opts)
            oq.setup(polished, P=P, q=q, A=A, l=l, u=u, polish=True, **opts)
            r0, r1 = oq.solve(plain), oq.solve(polished)
            s0, s1 = pol.oracle_state(plain, len(q), len(l), scaling), pol.oracle_state(polished, len(q), len(l), scaling)
            D, E, c, xs, zs, ys = s1
            _, _, _, ls, us = pol.scale_data(P, q, A, l, u, D, E, c)
            out.append(dict(plain=r0, polished=r1, state0=s0, state1=s1, act=adj.classify(zs, ys, ls, us)))
            oq.clean(plain); oq.clean(polished)
        _runs[key] = out
    return _runs[key]


def incoming(i):
    """The incoming gradients (g_x [count x n], g_y [count x m]) of shape i."""
    n, m = pattern(i)[1].shape[1], pattern(i)[1].shape[0]
    rng = np.random.default_rng(7000 + i)
    return rng.standard_normal((COUNT, n)), rng.standard_normal((COUNT, m))


def tangents(i, ndir):
    """Directions in all of q, l, u, Px, Ax of shape i: dict of [ndir x count x cols] (batch_jvp_ref.tangents)."""
    return jv.tangents("large-" + SHAPE_IDS[i], ndir, problems(i)[1])


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(b)))) if b.size else 0.0


def model_figures(oracle_lib, i):
    """(polish model vs oracle, adjoint model vs exact, JVP model vs exact): the worst figure of each over the instances of
    shape i under default settings, relative to max(1, max|reference|); the polish figure covers x, y of the accepted
    instances and asserts the status on all."""
    probs, runs = problems(i)[1], oracle_runs(oracle_lib, i)
    gx, gy = incoming(i)
    d = tangents(i, 1)
    fp = fa = fj = 0.0
    for k, ((P, q, A, l, u), r) in enumerate(zip(probs, runs)):
        if r["plain"].info.status_val != 1:
            continue
        out = pol.polish(P, q, A, l, u, *r["state0"], r["plain"].info.pri_res, r["plain"].info.dua_res)
        assert out["status"] == r["polished"].info.status_polish, (SHAPE_IDS[i], k)
        if out["status"] == 1:
            fp = max(fp, rel(out["x"], r["polished"].x), rel(out["y"], r["polished"].y))
        if not adj.nondegenerate(A, r["act"], len(q)):
            continue
        got = adj.model(P, q, A, l, u, *r["state1"], gx[k], gy[k])
        assert got["status"] == 1 and np.array_equal(got["act"], r["act"])
        fa = max(fa, adj.rel_err(got, adj.exact(P, A, got["x"], got["y"], got["act"], gx[k], gy[k])))
        dk = jv.direction(d, 0, k)
        gj = jv.model(P, q, A, l, u, *r["state1"], dk)
        fj = max(fj, jv.rel_err(gj["tx"], gj["ty"], *jv.exact(P, A, gj["x"], gj["y"], gj["act"], dk)))
    return fp, fa, fj
