"""Inputs of the tests of the gap stopping rule inside the batched kernels (test_batch_gap_rule_host.py,
test_batch_gap_rule_gpu.py; not a test module): the portfolio families pf(n, k) on which the rule moves some instances and not
others, the families on which it moves none, and the CPU procedure that says where every instance stops with the rule off
(K_off) and on (K_on) -- the oracle's iterates and the numpy statement of the gap (duality_ref.py), never the engine under
test.  DESIGN.md section 19 carries the table this module produces."""
import ctypes as C

import numpy as np
import scipy.sparse as sp

import batch_entry_families as fam
import batch_resident_ref as ref
import duality_ref
import qp_zoo
from duality_cases import CHECK, MAX_CHECKS, RULE_EPS, RULE_SETTINGS

SETTINGS = dict(RULE_SETTINGS, scaling=10)   # eps 1e-3, adaptive_rho_interval 25, ten Ruiz passes
MARGIN = 0.05                                # no ratio of a traced check lies within 1 +- MARGIN

# name -> (n, k, instances, the entry of the four-wavefront kernel that takes the pattern; -1: the 512-thread kernel)
PF = {"pf16": (16, 2, 8, 1), "pf24": (24, 3, 6, 6), "pf60": (60, 6, 6, -1), "pf12": (12, 2, 4, 1)}
# seed of instance i: 100 + i, except where that instance breaks a condition of test_batch_gap_rule_host.py
SEED = {("pf16", 7): 109, ("pf24", 1): 157, ("pf24", 4): 152, ("pf12", 1): 125, ("pf12", 3): 134}


def pf_pattern(n, k):
    """F of qp_zoo.portfolio(n, k, seed=1), drawn as there: its stored entries are the pattern of every instance."""
    rng = np.random.default_rng(1)
    F = sp.random(n, k, density=0.5, random_state=rng, data_rvs=rng.standard_normal, format="csc")
    F.sort_indices()
    return F


def pf_problem(n, k, seed):
    """One instance (P, q, A, l, u) on the pattern of qp_zoo.portfolio(n, k, seed=1): the values of F's stored entries, D and mu
    from default_rng(seed) -- standard normal, random(n) sqrt(k), standard normal, in that order; q = [-mu; 0],
    P = diag(2 D, 2 I); bounds as in that problem."""
    rng = np.random.default_rng(seed)
    F = pf_pattern(n, k)
    F.data = rng.standard_normal(F.nnz)
    D = rng.random(n) * np.sqrt(k)
    mu = rng.standard_normal(n)
    P = sp.diags(np.concatenate([2 * D, 2 * np.ones(k)])).tocsc()
    A = sp.vstack([
        sp.hstack([F.T, -sp.eye(k)]),
        sp.hstack([sp.csc_matrix(np.ones((1, n))), sp.csc_matrix((1, k))]),
        sp.hstack([sp.eye(n), sp.csc_matrix((n, k))]),
    ], format="csc")
    A.sort_indices()
    q = np.concatenate([-mu, np.zeros(k)])
    l = np.concatenate([np.zeros(k), [1.0], np.zeros(n)])
    u = np.concatenate([np.zeros(k), [1.0], np.ones(n)])
    return P, q, A, l, u


def pf_instances(name):
    """(what ResidentBatch takes, [(P, q, A, l, u)]) of a portfolio family: instance i is pf_problem(n, k, 100 + i), or of the
    seed SEED names for it."""
    n, k, count, _ = PF[name]
    probs = [pf_problem(n, k, SEED.get((name, i), 100 + i)) for i in range(count)]
    for p in probs[1:]:
        assert np.array_equal(p[2].indices, probs[0][2].indices) and np.array_equal(p[2].indptr, probs[0][2].indptr)
    return ref.stack(probs), probs


def pattern_of(args):
    return fam._finish(args[0], args[1])


def forced_entries(name):
    """The run-time-shaped entries of the four-wavefront kernel that take the family when forced (OSQP_AMD_BATCH_QUAD_CFG):
    the narrow ones and entry 4 for pf16, the wide ones for pf24, as far as `predict` accepts the pattern; entry 10, whose
    rows hold at most 12 entries, for pf12 (the family is there for it)."""
    families = {"pf16": ("narrow", "entry4"), "pf24": ("wide",), "pf12": ()}[name]
    pat = pattern_of(pf_instances(name)[0])
    nums = [10] if name == "pf12" else [num for num, f in fam.FAMILY.items() if f in families]
    return sorted(num for num in nums if fam.predict(pat, num)["entry"] == num)


def fixed_family(name, oracle_lib):
    """The families on which rule on and rule off must agree bit for bit: (what ResidentBatch takes, [(P, q, A, l, u)])."""
    if name == "mpc":
        probs = ref.mpc_instances(oracle_lib, 0, 8, 2)
        return ref.stack(probs), probs
    if name == "banded":
        return fam.instances(fam.banded(128, 192, 4), 3, 11)
    assert name == "random"
    return fam.instances(fam.random(32, 48, 7), 3, 12)


FIXED = ("mpc", "banded", "random")


def as_dict(prob):
    P, q, A, l, u = prob
    return dict(P=P, q=q, A=A, l=l, u=u)


class _Scaling(C.Structure):  # the oracle's private scaling record (oracle/osqp_oracle.c: scaling_t)
    _fields_ = [("c", C.c_double), ("cinv", C.c_double), ("D", C.POINTER(C.c_double)), ("Dinv", C.POINTER(C.c_double)),
                ("E", C.POINTER(C.c_double)), ("Einv", C.POINTER(C.c_double))]


def _oracle_iterate(oq, oracle_lib, prob, **settings):
    """(status, iter, x, y, (D, E, c)) of one oracle solve; D, E, c: the scaling the oracle used (ones without scaling)."""
    P, q, A, l, u = prob
    n, m = len(q), len(l)
    mdl = oq.Model(oracle_lib)
    oq.setup(mdl, P=sp.triu(P, format="csc"), q=q, A=A, l=l, u=u, **settings)
    r = oq.solve(mdl)
    D, E, c = np.ones(n), np.ones(m), 1.0
    if settings.get("scaling", 10):
        sc = C.cast(mdl.workspace.contents.scaling, C.POINTER(_Scaling)).contents
        D, E, c = np.array(sc.D[:n]), np.array(sc.E[:m]), float(sc.c)
    out = (r.info.status, int(r.info.iter), np.array(r.x, dtype=float), np.array(r.y, dtype=float), (D, E, c))
    oq.clean(mdl)
    return out


def ratios(prob, x, y, eps, scaling=None):
    """(pri, dua, gap): residuals and |gap| over their bounds at eps_abs = eps_rel = eps.  scaling = (D, E, c): in the scaled
    units (scaled_termination = 1) -- the same formulas on c D P D, c D q, E A D, E l, E u and D^-1 x, c E^-1 y."""
    p = as_dict(prob)
    if scaling is not None:
        D, E, c = scaling
        Dm, Em = sp.diags(D), sp.diags(E)
        Pf = duality_ref.full_P(p["P"])
        big = np.abs(p["l"]) >= duality_ref.INF_BOUND, np.abs(p["u"]) >= duality_ref.INF_BOUND
        p = dict(P=(c * (Dm @ Pf @ Dm)).tocsc(), q=c * D * p["q"], A=(Em @ sp.csc_matrix(p["A"]) @ Dm).tocsc(),
                 l=np.where(big[0], p["l"], E * p["l"]), u=np.where(big[1], p["u"], E * p["u"]))
        x, y = x / D, c * y / E
    pri, eps_pri, dua, eps_dua = qp_zoo.kkt_check(p, x, y, eps)
    return float(pri / eps_pri), float(dua / eps_dua), float(duality_ref.gap_ratio(p, x, y, eps))


_traces = {}


def trace_one(oq, oracle_lib, prob, settings):
    """rule_trace_batch for one instance."""
    scaled_units = bool(settings.get("scaled_termination", 0)) and bool(settings["scaling"])
    status, K_off, _, _, _ = _oracle_iterate(oq, oracle_lib, prob, **settings)
    row = dict(status=status, K_off=K_off, K_on=None, checks={})
    if status == "Solved" and K_off % CHECK == 0:
        for k in range(CHECK, K_off + CHECK * MAX_CHECKS, CHECK):
            st, it, x, y, sc = _oracle_iterate(oq, oracle_lib, prob, **dict(settings, eps_abs=1e-14, eps_rel=1e-14, max_iter=k))
            assert st == "Max_iter_reached" and it == k, (st, it, k)
            pri, dua, gap = ratios(prob, x, y, RULE_EPS, sc if scaled_units else None)
            row["checks"][k] = dict(pri=pri, dua=dua, gap=gap, x=x, y=y)
            if k >= K_off and gap < 1.0:
                row["K_on"] = k
                break
    return row


def rule_trace_batch(oq, oracle_lib, family, **extra):
    """The procedure of duality_cases.rule_trace, run per instance of a family (a name of PF or of FIXED): K_off = where the
    oracle stops on the residuals alone; for every check k from the FIRST (k = CHECK) on, the oracle's iterate after exactly k
    iterations (max_iter = k, eps = 1e-14: nothing stops it, adaptive rho does not look at eps) and its three ratios at
    RULE_EPS in numpy (in the scaled units with scaled_termination = 1); K_on = the first k >= K_off whose gap ratio is below
    1.  Returns [dict(K_off, K_on, status, checks = {k: dict(pri, dua, gap, x, y)})], one per instance, once per process.
    `extra`: settings on top of SETTINGS (scaling=0, scaled_termination=1)."""
    key = (family, tuple(sorted(extra.items())))
    if key in _traces:
        return _traces[key]
    probs = pf_instances(family)[1] if family in PF else fixed_family(family, oracle_lib)[1]
    settings = dict(SETTINGS, **extra)
    out = [trace_one(oq, oracle_lib, prob, settings) for prob in probs]
    _traces[key] = out
    return out


APPROX = ("pf24", 1)  # the instance of the approximate-pass test


def approximate_limits(row):
    """The iteration limits of the approximate-pass test for an instance the rule moves: one iteration before K_on, and one
    iteration after K_off (the gap is still above its bound, but not above ten times it)."""
    return [row["K_on"] - 1, row["K_off"] + 1]


def approximate_verdict(oq, oracle_lib, family, inst, max_iter):
    """What a solve of instance `inst` limited to max_iter iterations (no check is due at max_iter; every earlier check goes
    on) must report: the status after the two passes of the check at the limit -- the exact pass at RULE_EPS, then the
    approximate one at 10 RULE_EPS, three ratios each -- on the oracle's iterate at that iteration.  Returns (status, the
    ratios at RULE_EPS, at 10 RULE_EPS)."""
    assert max_iter % CHECK != 0
    prob = pf_instances(family)[1][inst]
    st, it, x, y, _ = _oracle_iterate(oq, oracle_lib, prob, **dict(SETTINGS, eps_abs=1e-14, eps_rel=1e-14, max_iter=max_iter))
    assert st == "Max_iter_reached" and it == max_iter
    exact = ratios(prob, x, y, RULE_EPS)
    approx = ratios(prob, x, y, 10 * RULE_EPS)
    if max(exact) < 1.0:
        return "Solved", exact, approx
    return ("Solved_inaccurate" if max(approx) < 1.0 else "Max_iter_reached"), exact, approx
