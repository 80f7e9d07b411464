"""Host helpers of the entry tests of the batched path (tests/test_batch_entries_host.py, tests/test_batch_entries_gpu.py):

  * `table()`: the rows of OQ_QUAD_ENTRIES, parsed out of osqp.jl_amd/csrc/batch_common.hpp, in try order;
  * deterministic pattern builders (`banded`, `spiked`, `random`) and `instances` on a pattern;
  * `predict`: a transcription into Python of what the host schedule of the four-wavefront kernel decides for a pattern
    (DevicePattern::build / build_quad in csrc/batch_sched.hpp, quad::make_layout in csrc/batch_quad.hpp): which entry takes
    it, the two-ended first phase, the term slots, the LDS bytes.  The GPU test holds the device's own report
    (osqp_amd_batch_last_schedule) to it, number by number;
  * `exact_optimum`, `rel_err`, `criteria_ratios`: an optimum that does not come from ADMM, and the measures against it;
  * `CASES`: the one list of cases both test files walk, and `reference(case, oracle_lib)`: the oracle's runs and the exact
    optima of a case, computed once per process.

No GPU needed."""
import functools
import os
import re
import warnings

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

import osqp_jl_amd as oq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble

OPTS = dict(verbose=False, eps_abs=1e-5, eps_rel=1e-5, adaptive_rho_interval=50, max_iter=4000)  # the suite's (test_batch_gpu.OPTS)
TIGHT = dict(OPTS, eps_abs=1e-8, eps_rel=1e-8, max_iter=8000)
CHECK = 25                # check_termination of both (the default)
LDS_LIMIT = 80 * 1024     # build_quad: two QPs per compute unit
QT, RECB, FIXED_BW = 256, 64, 19
MPC_N, MPC_M, MPC_NNZA = 100, 200, 800  # the MPC family (batch_common.hpp: NX 6, NU 4, TT 10)


# ---- the table -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def table():
    """[(number, NH, KC, KE, CH, fixed, kernel)] of the X(...) rows of OQ_QUAD_ENTRIES, in the order of the header."""
    text = open(os.path.join(ROOT, "osqp.jl_amd", "csrc", "batch_common.hpp")).read()
    body = text[text.index("#define OQ_QUAD_ENTRIES(X)"):]
    body = body[:body.index("struct QuadEntry")]
    rows = re.findall(r"\bX\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*([01])\s*,\s*(\w+)\s*\)", body)
    return [(int(a), int(b), int(c), int(d), int(e), f == "1", k) for a, b, c, d, e, f, k in rows]


def entry(number):
    return next(r for r in table() if r[0] == number)


# ---- patterns: (pat_P upper triangle with a full diagonal, pat_A), CSC, all values one ------------------------------------------
def _start(i, n, m, w):
    return int(round(i * (n - w) / max(m - 1, 1)))


def _finish(pat_P, pat_A):
    out = []
    for M in (pat_P, pat_A):
        M = sp.csc_matrix(M, copy=True)  # (the caller's values stay as they are)
        M.sum_duplicates()
        M.sort_indices()
        M.data[:] = 1.0
        out.append(M)
    return tuple(out)


def banded(n, m, w):
    """Row i of A holds w consecutive columns starting at round(i (n - w) / (m - 1)); P is tridiagonal."""
    rows = np.repeat(np.arange(m), w)
    cols = np.concatenate([np.arange(_start(i, n, m, w), _start(i, n, m, w) + w) for i in range(m)])
    A = sp.csc_matrix((np.ones(len(rows)), (rows, cols)), shape=(m, n))
    P = sp.triu(sp.diags([np.ones(n - 1), np.ones(n), np.ones(n - 1)], [-1, 0, 1]), format="csc")
    return _finish(P, A)


def spiked(n, m, w, long_row=0, long_col=0):
    """`banded`, with row m // 4 widened to `long_row` consecutive columns centred on its band and / or column 3 n // 4
    lengthened to `long_col` consecutive rows centred on the rows that hold it (both clipped to the matrix: a row has at most
    n entries, a column at most m)."""
    _, A = banded(n, m, w)
    A = A.tolil()
    if long_row:
        i = m // 4
        s = max(0, min(n - long_row, _start(i, n, m, w) - long_row // 2))
        A[i, s:s + long_row] = 1.0
    if long_col:
        j = (3 * n) // 4
        i0 = max(0, min(m - long_col, int(round(j * (m - 1) / max(n - w, 1))) - long_col // 2))
        A[i0:i0 + long_col, j] = 1.0
    return _finish(banded(n, m, w)[0], A.tocsc())


def random(n, m, seed):
    """The pattern of test_batch_gpu._family: a random symmetric P with a full diagonal (density 3 / n), a random A (4 / n)."""
    rng = np.random.default_rng(seed)
    S = sp.random(n, n, density=min(1.0, 3.0 / n), random_state=rng, format="csc")
    S.data[:] = 1.0
    P = sp.triu(S + S.T + sp.eye(n), format="csc")
    A = sp.random(m, n, density=min(1.0, 4.0 / max(n, 1)), random_state=rng, format="csc")
    return _finish(P, A)


def longest(pat_A):
    """(longest column, longest row) of A."""
    A = sp.csc_matrix(pat_A)
    return int(np.diff(A.indptr).max()), int(np.diff(A.tocsr().indptr).max())


def instances(pattern, count, seed):
    """`count` strictly convex QPs on the pattern, values as in test_batch_gpu._family(..., equalities=False): P diagonally
    dominant, A standard normal, bounds A x0 -+ (0.05 + U(0, 1)).  Returns (what solve_batch takes, [(P, q, A, l, u)])."""
    pat_P, pat_A = pattern
    n, m = pat_A.shape[1], pat_A.shape[0]
    rng = np.random.default_rng(seed)
    Px, Ax, qs, ls, us, probs = [], [], [], [], [], []
    for _ in range(count):
        U = pat_P.copy()
        U.data = 0.3 * rng.standard_normal(U.nnz)
        full = (U + U.T).tolil()
        row_sum = np.asarray(abs(U + U.T).sum(axis=1)).ravel()
        full.setdiag(row_sum + 0.1 + rng.random(n))
        P = sp.triu(full.tocsc(), format="csc")
        P.sort_indices()
        assert np.array_equal(P.indices, pat_P.indices) and np.array_equal(P.indptr, pat_P.indptr)
        A = pat_A.copy()
        A.data = rng.standard_normal(A.nnz)
        x0 = rng.standard_normal(n)
        w = 0.05 + rng.random(m)
        q = rng.standard_normal(n)
        l, u = A @ x0 - w, A @ x0 + w
        Px.append(P.data.copy()); Ax.append(A.data.copy()); qs.append(q); ls.append(l); us.append(u)
        probs.append((P, q, A, l, u))
    args = (pat_P, pat_A, np.array(Px), np.array(Ax).reshape(count, pat_A.nnz), np.array(qs), np.array(ls).reshape(count, m),
            np.array(us).reshape(count, m))
    return args, probs


def stack(probs):
    """What solve_batch takes, from per-instance problems that share a pattern (the MPC instances of the oracle's generator)."""
    P0, A0 = sp.triu(probs[0][0], format="csc"), sp.csc_matrix(probs[0][2])
    return (P0, A0, np.array([sp.triu(p[0]).tocsc().data for p in probs]), np.array([p[2].data for p in probs]),
            np.array([p[1] for p in probs]), np.array([p[3] for p in probs]), np.array([p[4] for p in probs]))


# ---- the host schedule, transcribed --------------------------------------------------------------------------------------------
def layout(n, m, nnzA, nnzF, NH, KC, KE, CH):
    """(offset of the pattern tables, total bytes) of quad::make_layout."""
    nh2 = 2 * ((NH + 15) & ~15)
    kch = (((KC + 1) // 2) + 1 + 3) & ~3
    kep = (KE + 3) & ~3
    pbstride = nh2 + 2
    o = (nnzA + KC + 2) * 8 + nnzF * 8 + 16
    o = (o + 15) & ~15
    o += max(2 * nh2 + 4 * n, 4 * pbstride) * 8
    o += 4 * n * 8
    o = (o + 15) & ~15
    o += (m + 1) * RECB + m * 8 + m * 8 + 2 * 4 * 8 * 8 + 24 * 8
    o += (m + 3) & ~3
    o += ((n + 1) * 2 + 3) & ~3
    o += (nnzF * 2 + 3) & ~3
    colstart = o
    o += QT * 2
    o = (o + 7) & ~7
    o += QT * kch * 2 + QT * 4
    o = (o + 15) & ~15
    o += max(QT * kep * 4, (CH * n + 1) * 8)
    return colstart, o


def predict(pattern, only=-1):
    """What DevicePattern::build decides for the pattern (`only`: OSQP_AMD_BATCH_QUAD_CFG): dict(entry, p1_top, p1_bot, bw,
    ns, kew, lds_bytes) for the first entry that takes it, dict(entry=-1, refused={number: reason}) when none does."""
    pat_P, pat_A = pattern
    n, m = pat_A.shape[1], pat_A.shape[0]
    Pd = (pat_P + pat_P.T).toarray() != 0
    Ad = pat_A.toarray() != 0
    terms = Ad.T.astype(np.int64) @ Ad.astype(np.int64)  # terms[i, j]: the rows columns i and j of A share
    M = np.eye(n, dtype=bool) | Pd | (terms > 0)
    nnzA, nnzF = int(Ad.sum()), int(Pd.sum())
    col_len, row_len = Ad.sum(axis=0), Ad.sum(axis=1)
    max_col, max_row = (int(col_len.max()), int(row_len.max())) if m and nnzA else (0, 0)
    mpc = n == MPC_N and m == MPC_M and nnzA == MPC_NNZA and nnzF == MPC_N
    refused = {}
    for num, NH, KC, KE, CH, fixed, _ in table():
        if (only >= 0 and num != only) or (fixed and not mpc):
            continue
        if n > 2 * NH:
            refused[num] = "n"; continue
        if m > QT or m == 0 or nnzA == 0:
            refused[num] = "rows"; continue
        if max_col > KC:
            refused[num] = "longest column"; continue
        if max_row > KE:
            refused[num] = "longest row"; continue
        colstart, total = layout(n, m, nnzA, nnzF, NH, KC, KE, CH)
        if colstart > 65535 or (nnzA + 1) * 8 > 65535:
            refused[num] = "LDS bytes below the pattern tables"; continue
        if total > LDS_LIMIT:
            refused[num] = "LDS bytes (%d)" % total; continue
        perm = [i if i < NH else n - 1 - (i - NH) for i in range(n)]
        over = [0]

        def count(first, last):
            cnt = 0
            for a in range(first, last + 1):
                pa = perm[a]
                if any(M[pa, perm[j]] for j in range(last + 1, n)) or any(M[pa, perm[j]] for j in range(first)):
                    return cnt
                for j in range(a, last + 1):
                    if M[pa, perm[j]]:
                        over[0] = max(over[0], j - a)
                cnt = a - first + 1
            return cnt

        top = count(0, min(n, NH) - 1)
        bot = count(NH, n - 1) if n > NH else 0
        nb = (NH + 15) // 16
        cap = (nb - 1) * 16 if nb > 1 else NH
        top, bot = min(top, cap), min(bot, cap)
        if top + bot < 8 or (fixed and over[0] > FIXED_BW):
            top = bot = 0
            perm = list(range(n))
        ch2 = CH // 2
        nwin = (NH + ch2 - 1) // ch2
        pm = np.array(perm)
        size = terms[np.ix_(pm, pm)] + Pd[np.ix_(pm, pm)] + np.eye(n, dtype=np.int64)  # terms of position (i, j), kernel's numbering
        ns = 0
        for cw in range(nwin):
            rows_w = [i for i in range(n) if (i - (i // NH) * NH) // ch2 == cw]
            sizes = size[rows_w].ravel()
            sizes = -np.sort(-sizes[sizes > 0], kind="stable")
            load = np.zeros(QT, dtype=np.int64)
            for g in sizes:
                load[int(np.argmin(load))] += g   # the first of the least loaded threads
            ns = max(ns, int(load.max()) if len(sizes) else 0)
        ns = max(4, (ns + 3) & ~3)
        if ns > 64:
            refused[num] = "assembly terms"; continue
        order = np.argsort(-row_len, kind="stable")  # lane L holds the L-th longest row
        kew = [int(row_len[order[64 * k:64 * k + 64]].max()) if m > 64 * k else 0 for k in range(4)]
        return dict(entry=num, p1_top=top, p1_bot=bot, bw=over[0], ns=ns, kew=kew, lds_bytes=total, refused=refused)
    return dict(entry=-1, refused=refused)


# ---- an optimum that does not come from ADMM, and the measures against it ------------------------------------------------------------
def oracle_solve(oracle_lib, prob, **opts):
    P, q, A, l, u = prob
    mdl = oq.Model(oracle_lib)
    oq.setup(mdl, P=P, q=q, A=A, l=l, u=u, **opts)
    r = oq.solve(mdl)
    oq.clean(mdl)
    return r


def exact_optimum(P, q, A, l, u, oracle_lib=None):
    """(x*, y*, certified) of min 1/2 x'Px + q'x, l <= Ax <= u with P positive definite (upper triangle given): the active set
    from an oracle solve at eps 1e-9 with polish (|y| above 1e-6 of its largest entry), then the equality-constrained KKT system
    by LU in float64 with four refinement steps on longdouble residuals.  certified: the inactive rows lie strictly inside
    their bounds, the multipliers have the sign of their side and the KKT residual is at rounding level -- the point then IS
    the unique optimum, whatever the oracle did on the way."""
    if oracle_lib is None:
        oracle_lib = oq.load_library(oq.ORACLE_LIB_PATH)
    r = oracle_solve(oracle_lib, (P, q, A, l, u), verbose=False, eps_abs=1e-9, eps_rel=1e-9, polish=True, max_iter=20000,
                     adaptive_rho_interval=50)
    n, m = len(q), len(l)
    nan = np.full(n, np.nan), np.full(m, np.nan), False
    if not np.all(np.isfinite(r.y)):
        return nan
    Pf = (sp.triu(P) + sp.triu(P, 1).T).toarray()
    Ad = sp.csc_matrix(A).toarray()
    thr = 1e-6 * float(np.max(np.abs(r.y))) if m else 0.0
    lo, up = r.y < -thr, r.y > thr
    if thr == 0.0:
        lo, up = r.y < 0, r.y > 0
    act = lo | up
    k = int(act.sum())
    Aa = Ad[act]
    K = np.block([[Pf, Aa.T], [Aa, np.zeros((k, k))]])
    rhs = np.concatenate([-np.asarray(q, dtype=float), np.where(up, u, l)[act]])
    KL, rL = K.astype(LD), rhs.astype(LD)
    try:  # dependent active rows (the multipliers are not unique then): nothing to certify
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", sla.LinAlgWarning)
            lu = sla.lu_factor(K)
            w = sla.lu_solve(lu, rhs).astype(LD)
            for _ in range(4):
                w = w + sla.lu_solve(lu, (rL - KL @ w).astype(float)).astype(LD)
    except (sla.LinAlgError, ValueError):
        return nan
    res = float(np.max(np.abs(rL - KL @ w)))
    xs, ys = w[:n], np.zeros(m, dtype=LD)
    ys[act] = w[n:]
    Ax = Ad.astype(LD) @ xs
    ok = bool(res <= 1e-12 * max(1.0, float(np.max(np.abs(rhs)))) and np.all(Ax[~act] > l[~act]) and np.all(Ax[~act] < u[~act]) and
              np.all(ys[up] > 0) and np.all(ys[lo] < 0))
    return xs, ys, ok


def rel_err(v, vstar):
    v, vstar = np.asarray(v, dtype=LD), np.asarray(vstar, dtype=LD)
    return float(np.max(np.abs(v - vstar)) / max(LD(1.0), np.max(np.abs(vstar)))) if len(vstar) else 0.0


def criteria_ratios(P, q, A, l, u, x, y, eps_abs, eps_rel):
    """OSQP's unscaled stopping rule re-evaluated from the raw data in longdouble, with the full symmetric P rebuilt from its
    triangle and z = clip(A x, l, u): (pri_res / eps_pri, dua_res / eps_dua)."""
    Pf = (sp.triu(P) + sp.triu(P, 1).T).toarray().astype(LD)
    Ad = sp.csc_matrix(A).toarray().astype(LD)
    x, y, q = np.asarray(x, dtype=LD), np.asarray(y, dtype=LD), np.asarray(q, dtype=LD)
    Ax = Ad @ x
    z = np.clip(Ax, np.asarray(l, dtype=LD), np.asarray(u, dtype=LD))
    Px, Aty = Pf @ x, Ad.T @ y
    pri, dua = np.max(np.abs(Ax - z)), np.max(np.abs(Px + q + Aty))
    eps_pri = eps_abs + eps_rel * max(np.max(np.abs(Ax)), np.max(np.abs(z)))
    eps_dua = eps_abs + eps_rel * max(np.max(np.abs(Px)), np.max(np.abs(Aty)), np.max(np.abs(q)))
    return float(pri / eps_pri), float(dua / eps_dua)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
BUILDERS = dict(banded=banded, spiked=spiked, random=random)
# which family of shapes a table row gets, by its public number.  A row added to the table gets its line here (and so its
# cases) with it: test_every_run_time_shaped_row_has_cases fails until it does.
FAMILY = {1: "narrow", 2: "narrow", 3: "narrow", 10: "narrow", 5: "narrow", 4: "entry4", 6: "wide", 7: "wide", 8: "wide", 9: "wide"}
RANDOM_SEED = {1: 7, 2: 7, 3: 7, 10: 10, 5: 7}  # of the random pattern at n = 2 NH (the host test checks it fits the entry's bounds;
                                                  # seed 10 at n = 100: the longest column is exactly entry 10's 12)


# instances of the generator's seed 5.  The MPC family has equality rows, and on many of its instances the active rows are
# linearly dependent (a state pinned by the dynamics sits on its box as well): x* is unique, the multipliers are not, and
# exact_optimum has nothing to certify.  These are the first six on which it certifies and the other conditions of
# test_conditions_on_the_inputs hold under both settings.
MPC_INSTANCES = (18, 23, 45, 53, 58, 66)
# seeds of the instances of a case: 1000 + its position in the list, except where that seed breaks a condition of
# test_conditions_on_the_inputs (on the smallest shapes the oracle lands within 1e-9 of the optimum on some instances; one
# instance of order-m256 takes more than half the iteration limit, its seed is in the list below)
SEED = {"e4-row13-n50": 3000, "e6-row24-n17": 3000, "e6-col24-n17": 3001, "e6-col24-n16": 3000, "e6-row32-n32": 3000}


def _case(cid, kind, args, expect, force=None, count=6, opts=OPTS, tight=False, seed=0, exceeds=0, phase=None, full_lanes=False,
          refused=None):
    """kind / args: the builder and its arguments ("mpc": the generator's instances); expect: the entry that must run;
    force: OSQP_AMD_BATCH_QUAD_CFG or None; exceeds: a bound of narrower entries the longest column or row must lie above;
    phase: "on" (banded, spiked), "off" (random) or None (nothing stated: the fixed shape); refused: what the error message of
    the batched entry point must hold where it takes no such shape at all."""
    n, m = (MPC_N, MPC_M) if kind == "mpc" else (args[0], args[1])
    assert kind != "mpc" or len(args) == count
    return dict(id=cid, kind=kind, args=tuple(args), n=n, m=m, expect=expect, force=force, count=count, opts=opts, tight=tight,
                seed=seed, exceeds=exceeds, phase=phase, full_lanes=full_lanes, refused=refused)


def _row_phase(n, NH, long_row):
    """Whether a first phase can exist next to a long row.  The row couples every pair of the min(long_row, n) variables it
    spans, and with more than NH variables a span of 17 or more reaches into both row halves: none of its variables is a
    pivot whose fill stays inside its own quadrant.  That leaves the variables outside the span, and the schedule wants 8
    first-phase pivots before it switches the phase on (build_quad: p1_top + p1_bot < 8)."""
    return "off" if n > NH and n - min(long_row, n) < 8 else "on"


def _cases():
    out = []
    for num, NH, KC, KE, CH, fixed, _ in table():
        if fixed:
            out.append(_case("e%d-mpc" % num, "mpc", MPC_INSTANCES, num, seed=5))
            out.append(_case("e%d-mpc-tight" % num, "mpc", MPC_INSTANCES, num, seed=5, opts=TIGHT, tight=True))
            continue
        fam = FAMILY.get(num)
        if fam is None:
            continue
        mine = []
        sizes = (2 * NH, 2 * NH - 1, NH + 1, NH)
        if fam == "narrow":
            for n in sizes:
                mine.append(_case("e%d-banded-n%d" % (num, n), "banded", (n, 3 * n // 2, 4), num, num, phase="on"))
            n = 2 * NH
            mine.append(_case("e%d-random-n%d" % (num, n), "random", (n, 3 * n // 2, RANDOM_SEED[num]), num, num, phase="off"))
        elif fam == "entry4":
            mine.append(_case("e%d-banded7-n100" % num, "banded", (100, 200, 7), num, None, phase="on", exceeds=12))
            mine.append(_case("e%d-banded7-n99" % num, "banded", (99, 198, 7), num, None, phase="on", exceeds=12))
            for n in sizes:
                mine.append(_case("e%d-row13-n%d" % (num, n), "spiked", (n, n, 4, 13, 0), num, num, phase="on", exceeds=12))
        elif fam == "wide":
            for n in sizes:
                # (a row holds at most n entries: at n <= 24 the long row is the whole row; it exceeds 16 from n = 17 on)
                mine.append(_case("e%d-row24-n%d" % (num, n), "spiked", (n, n, 4, 24, 0), num, num, phase=_row_phase(n, NH, 24), exceeds=16 if n > 16 else 0))
                mine.append(_case("e%d-col24-n%d" % (num, n), "spiked", (n, n, 4, 0, 24), num, num, phase="on", exceeds=16 if n > 16 else 0))
                if n <= 24:  # m = n cannot hold a column of 24: the same with 32 rows, so that a long column runs at this n too
                    mine.append(_case("e%d-col24-n%d-m32" % (num, n), "spiked", (n, 32, 4, 0, 24), num, num, phase="on", exceeds=16))
            n = 2 * NH
            mine.append(_case("e%d-row32-n%d" % (num, n), "spiked", (n, n, 4, 32, 0), num, num, phase=_row_phase(n, NH, 32), exceeds=31))
        first = next(c for c in mine if c["n"] == 2 * NH)
        mine.append(dict(first, id=first["id"] + "-tight", opts=TIGHT, tight=True))
        out += mine
    # try order and fall-through, unforced: the entry is asserted exactly
    out += [
        _case("order-col16", "spiked", (64, 64, 4, 0, 16), 2, phase="on"),
        _case("order-col17", "spiked", (64, 64, 4, 0, 17), 7, phase="on", exceeds=16),
        _case("order-row12", "spiked", (100, 100, 4, 12, 0), 10, phase="on"),
        _case("order-row13", "spiked", (100, 100, 4, 13, 0), 4, phase="on", exceeds=12),
        _case("order-col33", "spiked", (64, 64, 4, 0, 33), -1, exceeds=32),
        # (n = 129 is beyond the batched path altogether: osqp_amd_batch_solve refuses it with its message, it launches nothing)
        _case("order-n129", "banded", (129, 193, 4), -1, refused="n <= 128"),
        _case("order-m257", "banded", (32, 257, 3), -1),
        _case("order-m256", "banded", (32, 256, 3), 6, phase="on", exceeds=16, full_lanes=True, seed=2000),
    ]
    # the tightest fit of the list: 304 bytes below the LDS limit
    out.append(_case("e9-banded-n128-m192", "banded", (128, 192, 4), 9, 9, phase="on"))
    # batch sizes: one narrow and one wide case again, with one instance and with seven
    for count in (1, 7):
        out.append(_case("count%d-e2-banded-n64" % count, "banded", (64, 96, 4), 2, 2, count=count, phase="on"))
        out.append(_case("count%d-e9-col24-n128" % count, "spiked", (128, 128, 4, 0, 24), 9, 9, count=count, phase="on", exceeds=16))
    for i, c in enumerate(out):
        c["seed"] = c["seed"] or SEED.get(c["id"], 1000 + i)
    assert len({c["id"] for c in out}) == len(out)
    return out


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]


@functools.lru_cache(None)
def pattern(kind, args):
    return BUILDERS[kind](*args)


def case_problems(case, oracle_lib):
    """(what solve_batch takes, [(P, q, A, l, u)]) of a case."""
    if case["kind"] == "mpc":
        from test_gpu_parity import _data_to_scipy

        probs = []
        for i in case["args"]:
            d = oracle_lib.oracle_generate(2, 100, i, case["seed"])
            probs.append(_data_to_scipy(d.contents))
            oracle_lib.oracle_data_free(d)
        return stack(probs), probs
    return instances(pattern(case["kind"], case["args"]), case["count"], case["seed"])


_REFERENCE = {}


def reference(case, oracle_lib):
    """The host side of a case, computed once per process and shared (nothing in it is changed afterwards): the instances,
    and per instance the oracle's run under the case's settings (status, iter, x, y), its rel_err to the exact optimum e_O, the
    same for the run stopped one check earlier e_O1 (e_O where it stopped at its first check), its criteria ratios, and the
    exact optimum with its certificate."""
    key = case["id"]
    if key in _REFERENCE:
        return _REFERENCE[key]
    args, probs = case_problems(case, oracle_lib)
    opts = case["opts"]
    rows = []
    for prob in probs:
        r = oracle_solve(oracle_lib, prob, **opts)
        xs, ys, ok = exact_optimum(*prob, oracle_lib=oracle_lib)
        row = dict(status=r.info.status, status_val=r.info.status_val, iter=int(r.info.iter), x=r.x.copy(), y=r.y.copy(), xs=xs, ys=ys,
                   certified=ok)
        if r.info.status == "Solved" and ok:
            row["ratios"] = criteria_ratios(*prob, r.x, r.y, opts["eps_abs"], opts["eps_rel"])
            row["e_O"] = (rel_err(r.x, xs), rel_err(r.y, ys))
            row["e_O1"] = row["e_O"]
            if r.info.iter > CHECK:
                r1 = oracle_solve(oracle_lib, prob, **dict(opts, max_iter=int(r.info.iter) - CHECK, check_termination=0))
                if np.all(np.isfinite(r1.x)):
                    row["e_O1"] = (rel_err(r1.x, xs), rel_err(r1.y, ys))
                    row["iter1"] = int(r1.info.iter)
        rows.append(row)
    _REFERENCE[key] = dict(args=args, probs=probs, rows=rows)
    return _REFERENCE[key]
