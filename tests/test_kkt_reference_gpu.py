"""The direct back-end's KKT solve (op 3 of osqp_amd_apply) against an exact host reference (kkt_reference.py) -- not against
another form of the factorisation -- for every form of it, on one workspace through the events that rewrite the factor:

  1. setup;  2. update_settings(rho=0.731);
  3. a full value update of P and A (P -> D P D, D a random positive diagonal in [0.5, 2]: PSD kept, every entry changed
     differently; A -> A o (1 + 0.3 xi));
  4. an update of an index subset (the entries of P that touch a random tenth of the variables, a random third of A's);
  5. a bounds update that turns inequality rows into equalities and free rows and equalities back into inequalities (their rho
     changes: csrc/engine.hip update_rho_vec_from_bounds, a refactorisation);
  6. a second rho update;
and then an update to an indefinite P, which must be refused.  After events 3 and 4 the workspace's own products A x, A'y and
P x (ops 0 / 1 / 2) are checked against scipy too: a broken nnz-index map shows there, a broken factor only in the solve.
Workspaces are unscaled with a fixed rho (scaling=0, adaptive_rho=False): the reference's matrix is the caller's.

Bounds (kkt_reference.py): (a) backward error <= BACKWARD = 1e-10, (b) z~ = A x~ to IDENTITY = 1e-9, (c) forward distance to
SuperLU <= FORWARD = 1e-9 -- every form, every structure.  Measured worst case on an MI355X per form, over its structures and
events, (a) / (b) / (c), the cases of BY_CONDITION left out of (a):
  default                   5.0e-11 / 7.2e-11 / 1.9e-13   (edge patterns: 6.2e-11 / 7.4e-11 / 1.8e-14)
  level                     4.2e-11 / 7.1e-11 / 3.4e-11
  level-supernodes          3.2e-13 / 4.2e-16 / 4.3e-15
  lds-3, lds-3-lean         1.2e-12, 2.0e-13 / 1.4e-12 / 1.5e-13
  lds-64, lds-64-lean       3.1e-13, 2.5e-13 / 2.7e-13 / 1.3e-13
  global-split, -panel      1.5e-11, 1.6e-12 / 1.1e-12 / 1.4e-13
  dense-top-lds             2.5e-13 / 5.0e-16 / 1.1e-15
  dense-top-global, no-tree 4.7e-14, 1.9e-12 / 1.1e-12 / 1.3e-13
  tree-persistent           2.1e-12 / 4.2e-12 / 1.8e-13
  tree-oversub-1, -2        3.7e-12, 1.6e-13 / 7.3e-12 / 2.1e-13
  dense-sym-0, -1           (all in BY_CONDITION)
  edge patterns, supernodes 5.8e-11 / 1.2e-10 / 4.4e-11
Each case of BY_CONDITION measures (a) above 1e-10 and goes through an explicitly inverted block -- the dense top block of the
level schedule (>= 512 pivots on equality_qp, the dense trailing block of random-200, lp, dense-row-and-column), the forced dense
top over the supernodes, the 3 x 3 blocks of svm's supernodes next to its free rows -- whose error grows with the block's
condition number.  It is held to (a') instead: ||w - w_ref|| / ||w_ref|| <= cond(K, w) * 1e-10.  Worst (a) / cond(K, w) /
forward error in w / its share of the (a') bound (worst of two runs; the estimator starts from random vectors):
  default:  random-200 6.7e-10 / 59 / 1.1e-10 / 0.045;  equality-600 4.1e-10 / 230 / 1.9e-10 / 0.012;
            equality-1100 1.8e-10 / 270 / 3.3e-10 / 0.015;  lp 1.5e-10 / 12 / 5.3e-11 / 0.091;
            dense-row-and-column 3.2e-10 / 39 / 1.7e-11 / 0.0094
  level:    random-200 6.8e-10 / 36 / 5.1e-11 / 0.044;  equality-600 3.0e-10 / 200 / 1.8e-10 / 0.017
  lds-3-lean, svm            2.1e-10 / 7.7 / 6.1e-16 / 1.8e-6
  dense-top-global, random-200 6.9e-10 / 37 / 3.8e-11 / 0.015
  dense-sym-0: equality-600 3.8e-10 / 280 / 2.1e-10 / 0.011;  equality-1100 1.5e-10 / 390 / 2.0e-10 / 0.0091
  dense-sym-1: equality-600 3.0e-10 / 180 / 2.9e-10 / 0.023;  equality-1100 1.5e-10 / 290 / 2.7e-10 / 0.011
The module takes 9 - 11 s with an MI355X, host work included (9.5 s in the last run)."""
import re
import zlib

import numpy as np
import pytest
import scipy.sparse as sp

import qp_zoo
from kkt_events import Workspace as _Workspace  # the event driver (shared with test_pcg_reference_gpu.py)
from test_multifrontal_gpu import _random_problem

pytestmark = pytest.mark.gpu

STRUCTURES = {
    "control": lambda: qp_zoo.control(nx=8, nu=4, T=400),
    "grid2d": lambda: qp_zoo.grid2d(40),
    "grid3d-9": lambda: qp_zoo.grid3d(9),
    "grid3d-14": lambda: qp_zoo.grid3d(14),  # fronts beyond LDS at the default thresholds
    "portfolio": lambda: qp_zoo.portfolio(n=300, k=10),
    "svm": lambda: qp_zoo.svm(n=20, m=150),
    "random-200": lambda: _random_problem(np.random.default_rng(6), 200, 150, 0.02),
    "equality-600": lambda: qp_zoo.equality_qp(600),    # a dense block of >= 512 pivots (block sweeps), not a multiple of the tile
    "equality-1100": lambda: qp_zoo.equality_qp(1100),
}

_SN = {"OSQP_AMD_SNODE": "2"}
_DENSE_TOP = dict(_SN, OSQP_AMD_SNODE_MAX="16", OSQP_AMD_SN_DENSE="2")
# name: (environment, what the statistics must show, structures)
FORMS = {
    "default": ({}, lambda st: True, sorted(STRUCTURES)),
    "level": ({"OSQP_AMD_SNODE": "0", "OSQP_AMD_MF": "0", "OSQP_AMD_SN_DENSE": "0"},
              lambda st: st[19] == 0 and st[22] == 0, ["control", "grid2d", "svm", "random-200", "equality-600"]),
    "level-supernodes": (dict(_SN, OSQP_AMD_MF="0"), lambda st: st[19] >= 1 and st[22] == 0, ["portfolio", "grid3d-9"]),
    "lds-3": (dict(_SN, OSQP_AMD_SNODE_MAX="3", OSQP_AMD_LEAN="0"), lambda st: st[19] >= 1 and st[22] == 1 and st[23] == 0,
              ["control", "grid2d"]),
    "lds-3-lean": (dict(_SN, OSQP_AMD_SNODE_MAX="3", OSQP_AMD_LEAN="1"), lambda st: st[19] >= 1 and st[22] == 1 and st[23] == 1,
                   ["random-200", "svm"]),
    "lds-64": (dict(_SN, OSQP_AMD_SNODE_MAX="64", OSQP_AMD_LEAN="0"), lambda st: st[19] >= 1 and st[22] == 1 and st[23] == 0,
               ["portfolio", "grid3d-9"]),
    "lds-64-lean": (dict(_SN, OSQP_AMD_SNODE_MAX="64", OSQP_AMD_LEAN="1"), lambda st: st[19] >= 1 and st[22] == 1 and st[23] == 1,
                    ["control", "portfolio"]),
    "global-split": (dict(_SN, OSQP_AMD_SNODE_MAX="16", OSQP_AMD_MF_MAX_FRONT="8", OSQP_AMD_MFB_SPLIT="1", OSQP_AMD_MF_SHARE_MIN="3"),
                     lambda st: st[19] >= 1 and st[22] == 1, ["grid3d-9", "grid3d-14", "control"]),
    "global-panel": (dict(_SN, OSQP_AMD_SNODE_MAX="16", OSQP_AMD_MF_MAX_FRONT="8", OSQP_AMD_MFB_SPLIT="0", OSQP_AMD_MF_SHARE_MIN="3"),
                     lambda st: st[19] >= 1 and st[22] == 1, ["grid2d", "grid3d-14", "random-200"]),
    "dense-top-lds": (dict(_DENSE_TOP, OSQP_AMD_SN_DENSE_MAX="24", OSQP_AMD_MF_SHARE_MIN="3"),
                      lambda st: st[22] == 1 and 1 <= st[25] <= 24, ["grid2d", "portfolio"]),
    "dense-top-global": (dict(_DENSE_TOP, OSQP_AMD_SN_DENSE_MAX="150", OSQP_AMD_MF_MAX_FRONT="12", OSQP_AMD_SNODE_TOP="1"),
                         lambda st: st[22] == 1 and 1 <= st[25] <= 150, ["grid3d-9", "random-200"]),
    "dense-top-global-no-tree": (dict(_DENSE_TOP, OSQP_AMD_SN_DENSE_MAX="150", OSQP_AMD_MF_MAX_FRONT="12", OSQP_AMD_SNODE_TOP="1",
                                      OSQP_AMD_SNODE_TREE="0"),
                                 lambda st: st[22] == 1 and 1 <= st[25] <= 150, ["grid2d", "control"]),
    # the one-launch tree with persistent workgroups: a launch of at most 128 of them takes every supernode from level 1 on
    "tree-persistent": (dict(_SN, OSQP_AMD_SNODE_MAX="3", OSQP_AMD_SNODE_TREE_PERSIST="1", OSQP_AMD_SNODE_TREE_CAP="128"),
                        lambda st: st[19] > 2 and st[22] == 1, ["control", "grid2d"]),
    # (no dense top over the supernodes, which the fronts beyond LDS bring by default: it would take the levels out of the launch)
    "tree-oversub-1": (dict(_SN, OSQP_AMD_SNODE_MAX="3", OSQP_AMD_MF_MAX_FRONT="8", OSQP_AMD_SN_DENSE="0", OSQP_AMD_SNODE_TREE_OVERSUB="1"),
                       lambda st: st[19] > 2 and st[22] == 1, ["grid3d-9", "control"]),
    "tree-oversub-2": (dict(_SN, OSQP_AMD_SNODE_MAX="3", OSQP_AMD_MF_MAX_FRONT="8", OSQP_AMD_SN_DENSE="0", OSQP_AMD_SNODE_TREE_OVERSUB="2"),
                       lambda st: st[19] > 2 and st[22] == 1, ["grid3d-14", "grid2d"]),
    "dense-sym-0": ({"OSQP_AMD_DENSE_SYM": "0"}, lambda st: st[25] >= 512, ["equality-600", "equality-1100"]),
    "dense-sym-1": ({"OSQP_AMD_DENSE_SYM": "1"}, lambda st: st[25] >= 512, ["equality-600", "equality-1100"]),
}
CASES = [(form, s) for form, (_, _, structures) in FORMS.items() for s in structures]


def _fronts_beyond_lds(err):
    m = re.search(r"\[fronts\] beyond LDS: (\d+) fronts", err)
    return int(m[1]) if m else -1


def _tree(err):
    """(on, first level, threads, persistent workgroups) of the one-launch tree (csrc/direct.hip supernodes_on_device)."""
    m = re.search(r"one-launch tree (on|off): from level (\d+) of \d+, (\d+) threads, (\d+) persistent workgroups", err)
    return (m[1] == "on", int(m[2]), int(m[3]), int(m[4])) if m else None


def _tree_cap_oversubscribed(k):
    """The launch of the one-launch tree may hold k times the workgroups the device holds at once."""
    def ok(err):
        m = re.search(r"(\d+) / (\d+) resident workgroups of 1024 threads per compute unit \(forward / backward\), (\d+) compute units, "
                      r"launch of at most (\d+)", err)
        return m is not None and int(m[4]) == k * min(int(m[1]), int(m[2])) * int(m[3])
    return ok


# what the setup trace (OSQP_AMD_SETUP_TRACE) must show for a knob to have done what it is there for -- no statistic shows it
TRACES = {
    "lds-3": [lambda err: _fronts_beyond_lds(err) == 0],
    "lds-64": [lambda err: _fronts_beyond_lds(err) == 0],
    "global-split": [lambda err: _fronts_beyond_lds(err) > 0],
    "global-panel": [lambda err: _fronts_beyond_lds(err) > 0],
    # persistent workgroups: 128 of them take every supernode from level 1 on (more of them than that above level 0)
    "tree-persistent": [lambda err: _fronts_beyond_lds(err) == 0, lambda err: _tree(err) == (True, 1, 512, 128)],
    # the cap of the launch applies where fronts go through global memory; at these sizes every supernode fits under either cap
    "tree-oversub-1": [lambda err: _fronts_beyond_lds(err) > 0, lambda err: _tree(err)[0], _tree_cap_oversubscribed(1)],
    "tree-oversub-2": [lambda err: _fronts_beyond_lds(err) > 0, lambda err: _tree(err)[0], _tree_cap_oversubscribed(2)],
}

# (form, structure) whose backward error (a) measures above kkt_reference.BACKWARD: each goes through an explicitly inverted block
# and is held to (a') instead -- its forward error no larger than a backward error of BACKWARD allows at the solve's condition
BY_CONDITION = {
    ("default", "random-200"), ("default", "equality-600"), ("default", "equality-1100"),
    ("level", "random-200"), ("level", "equality-600"),
    ("lds-3-lean", "svm"),
    ("dense-top-global", "random-200"),
    ("dense-sym-0", "equality-600"), ("dense-sym-0", "equality-1100"), ("dense-sym-1", "equality-600"), ("dense-sym-1", "equality-1100"),
    ("default", "lp"), ("default", "dense-row-and-column"),
}


def _run_case(lib, monkeypatch, capfd, env, form_ran, traces, prob, form, structure):
    """Sets the form up, asserts through the statistics (and the setup trace where no statistic tells) that it is the one that
    runs, goes through the events."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if traces:
        monkeypatch.setenv("OSQP_AMD_SETUP_TRACE", "1")
        capfd.readouterr()
    what = f"{form} / {structure}"
    w = _Workspace(lib, prob, what, zlib.crc32(what.encode()), (form, structure) in BY_CONDITION)
    try:
        st = w.stats()
        assert st[0] == 0 and form_ran(st), (what, "levels / supernode levels / fronts / lean / dense", st[5], st[19], st[22], st[23], st[25])
        if traces:
            err = capfd.readouterr().err
            for k, ok in enumerate(traces):
                assert ok(err), (what, k, _fronts_beyond_lds(err), _tree(err))
            monkeypatch.delenv("OSQP_AMD_SETUP_TRACE")
        refused = w.run()
    finally:
        w.close()
    return w, refused


@pytest.mark.parametrize("form,structure", CASES)
def test_kkt_solves_match_the_reference(product_lib, monkeypatch, capfd, form, structure):
    env, form_ran, _ = FORMS[form]
    w, refused = _run_case(product_lib, monkeypatch, capfd, env, form_ran, TRACES.get(form), STRUCTURES[structure](), form, structure)
    assert refused


def _edge(name):
    """Small hand-built problems at the edges of the assembly (k_diag_init, k_scatter_P / _A, k_rho_vec, the permutations)."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))

    def psd(n, dens):
        M = sp.random(n, n, density=dens, random_state=rng, data_rvs=rng.standard_normal)
        return sp.triu((M @ M.T + 0.1 * sp.eye(n)).tocsc(), format="csc")

    def box(m, eq=0.2):
        l, u = -rng.random(m) - 0.1, rng.random(m) + 0.1
        e = rng.random(m) < eq
        u[e] = l[e]
        return l, u

    if name == "empty-rows-and-lone-variables":  # rows 3, 10, 17 of A empty; variables 25 - 29 in neither A nor P
        n, m = 30, 25
        P = sp.block_diag([psd(25, 0.1), sp.csc_matrix((5, 5))], format="csc")
        A = sp.random(m, 25, density=0.2, random_state=rng, data_rvs=rng.standard_normal, format="lil")
        A[[3, 10, 17], :] = 0
        A = sp.hstack([A.tocsc(), sp.csc_matrix((m, 5))], format="csc")
        A.eliminate_zeros()
        l, u = box(m)
    elif name == "free-and-equality-rows":  # rho^-1 = 1e6 next to rho^-1 = 1e-3 / rho in one matrix
        n, m = 30, 40
        P = psd(n, 0.1)
        A = sp.random(m, n, density=0.15, random_state=rng, data_rvs=rng.standard_normal, format="csc")
        l, u = box(m, 0.0)
        l[:10], u[:10] = -np.inf, np.inf
        u[10:20] = l[10:20]
    elif name == "explicit-zeros":  # stored zeros in P (diagonal and off-diagonal) and A that the full update makes non-zero
        n, m = 20, 15
        d = rng.uniform(0.5, 2.0, n)
        d[::3] = 0.0
        P = sp.csc_matrix((np.append(d, 0.0), (np.append(np.arange(n), 1), np.append(np.arange(n), 2))), shape=(n, n))
        A = sp.random(m, n, density=0.3, random_state=rng, data_rvs=rng.standard_normal, format="csc")
        A.data[::4] = 0.0
        l, u = box(m)
    elif name == "lp":  # P = 0: pivots of sigma alone
        n, m = 30, 40
        P = sp.csc_matrix((n, n))
        A = sp.vstack([sp.random(m - n, n, density=0.2, random_state=rng, data_rvs=rng.standard_normal), sp.eye(n)], format="csc")
        l, u = box(m)
    elif name == "dense-row-and-column":
        n, m = 60, 40
        P = psd(n, 0.05)
        A = sp.random(m, n, density=0.05, random_state=rng, data_rvs=rng.standard_normal, format="lil")
        A[5, :] = rng.standard_normal(n)
        A[:, 7] = rng.standard_normal((m, 1))
        A = A.tocsc()
        l, u = box(m)
    elif name == "n=1":
        n = 1
        P = sp.csc_matrix([[2.0]])
        A = sp.csc_matrix([[1.0], [3.0], [-1.0], [0.5]])
        l, u = np.array([-1.0, 0.5, -np.inf, -2.0]), np.array([1.0, 0.5, np.inf, 2.0])
    elif name == "m=0":
        n = 25
        P = psd(n, 0.1)
        A = sp.csc_matrix((0, n))
        l = u = np.zeros(0)
    else:
        raise KeyError(name)
    return dict(P=P, q=rng.standard_normal(n), A=A, l=l, u=u)


EDGES = ["empty-rows-and-lone-variables", "free-and-equality-rows", "explicit-zeros", "lp", "dense-row-and-column", "n=1", "m=0"]


@pytest.mark.parametrize("form", ["default", "supernodes"])
@pytest.mark.parametrize("name", EDGES)
def test_edge_patterns_match_the_reference(product_lib, monkeypatch, name, form):
    prob = _edge(name)
    if name == "explicit-zeros":
        assert np.sum(prob["P"].data == 0) == 8 and np.sum(prob["A"].data == 0) > 0
    env, form_ran = (_SN, lambda st: st[19] >= 1) if form == "supernodes" else ({}, lambda st: True)
    w, refused = _run_case(product_lib, monkeypatch, None, env, form_ran, None, prob, form, name)
    assert refused == (name != "lp")
    if name == "explicit-zeros":
        assert np.all(w.P.data != 0) and np.all(w.A.data != 0)  # (the updates did reach what was stored as zero)
