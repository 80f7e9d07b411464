"""Reference side of the resident-batch tests: one oracle `Model` per instance, driven through the same sequence of
setup / update / warm_start / solve calls as the `ResidentBatch` under test, and the comparison the batched tests
already use between the kernels and the oracle.  No GPU needed: tests/test_batch_resident_host.py exercises this half
on its own."""
import numpy as np
import scipy.sparse as sp

import osqp_jl_amd as oq
from test_gpu_parity import _data_to_scipy

OPTS = dict(verbose=False, eps_abs=1e-5, eps_rel=1e-5, adaptive_rho_interval=50, max_iter=4000)


def mpc_instances(oracle_lib, first, count, seed):
    probs = []
    for i in range(first, first + count):
        d = oracle_lib.oracle_generate(2, 100, i, seed)
        probs.append(_data_to_scipy(d.contents))
        oracle_lib.oracle_data_free(d)
    return probs


def stack(probs):
    """(P0, A0, Px, Ax, q, l, u): the shared pattern and the [count x .] arrays `ResidentBatch` / `solve_batch` take."""
    P0, _, A0, _, _ = probs[0]
    Px = np.array([sp.triu(p[0]).tocsc().data for p in probs]).reshape(len(probs), -1)
    Ax = np.array([p[2].data for p in probs]).reshape(len(probs), -1)
    q = np.array([p[1] for p in probs]); l = np.array([p[3] for p in probs]); u = np.array([p[4] for p in probs])
    return P0, A0, Px, Ax, q, l.reshape(len(probs), -1), u.reshape(len(probs), -1)


class OracleBatch:
    """A list of oracle models, one per instance, with the call surface of `batch.ResidentBatch`."""

    def __init__(self, oracle_lib, probs, **opts):
        self.models = []
        for P, q, A, l, u in probs:
            m = oq.Model(oracle_lib)
            oq.setup(m, P=P, q=q, A=A, l=l, u=u, **opts)
            self.models.append(m)

    def update(self, q=None, l=None, u=None, Px=None, Ax=None):
        for i, m in enumerate(self.models):
            oq.update(m, **{k: v[i] for k, v in dict(q=q, l=l, u=u, Px=Px, Ax=Ax).items() if v is not None})

    def warm_start(self, x=None, y=None):
        for i, m in enumerate(self.models):
            oq.warm_start(m, x=None if x is None else x[i], y=None if y is None else y[i])

    def solve(self):
        return [oq.solve(m) for m in self.models]

    def close(self):
        for m in self.models:
            oq.clean(m)
        self.models = []


def cold_oracle(oracle_lib, probs, **opts):
    """Fresh setup + solve of every instance."""
    ob = OracleBatch(oracle_lib, probs, **opts)
    res = ob.solve()
    ob.close()
    return res


def with_vectors(probs, q=None, l=None, u=None):
    """The per-instance problems with row i of the given [count x .] arrays in place of their vectors."""
    return [(P, pq if q is None else q[i], A, pl if l is None else l[i], pu if u is None else u[i])
            for i, (P, pq, A, pl, pu) in enumerate(probs)]


def compare(x, y, info, refs, opts, tag=""):
    """The tolerances of tests/test_batch_gpu.py between the batched kernels and the oracle: status equal, iteration counts
    within one check, solutions of Solved instances within 50 max(eps_abs, 1e-7) relative to max(1, |ref|); NaN rows where
    the oracle has no solution.  Prints the figures before it asserts."""
    check = int(opts.get("check_termination", 25))
    tol = 50 * max(opts.get("eps_abs", 1e-3), 1e-7)
    for i, r in enumerate(refs):
        ex = float(np.max(np.abs(x[i] - r.x))) if r.info.status_val == 1 else float("nan")
        ey = float(np.max(np.abs(y[i] - r.y))) if r.info.status_val == 1 and len(r.y) else 0.0
        print(f"{tag} inst {i}: status {int(info[i, 1])}/{r.info.status_val} iter {int(info[i, 0])}/{r.info.iter} dx {ex:.2e} dy {ey:.2e}")
        assert int(info[i, 1]) == r.info.status_val, (tag, i, info[i, :2], r.info.status)
        assert abs(r.info.iter - info[i, 0]) <= check, (tag, i, info[i, 0], r.info.iter)
        if r.info.status_val == 1:
            assert ex <= tol * max(1.0, float(np.max(np.abs(r.x)))), (tag, i, ex)
            if len(r.y):
                assert ey <= tol * max(1.0, float(np.max(np.abs(r.y)))), (tag, i, ey)
        elif r.info.status_val in (-3, 3, -4, 4):
            assert np.all(np.isnan(x[i])), (tag, i)


def closed_loop_steps(q, l, u, steps=6, seed=7):
    """The perturbation family of the warm-start test: instance by instance, after solve k (k = 0 .. steps - 2)
    l[0:6] = u[0:6] = l[0:6] + 0.01 N(0, 1) (k % 2), then q[0:6] *= 1 + 0.02 N(0, 1), drawn from default_rng(seed) in that
    order.  Returns [(q_k, l_k, u_k)] for k = 0 .. steps - 1 (step 0: the data as given)."""
    rng = np.random.default_rng(seed)
    count = q.shape[0]
    out = [(q.copy(), l.copy(), u.copy()) for _ in range(steps)]
    for i in range(count):
        qi, li, ui = q[i].copy(), l[i].copy(), u[i].copy()
        for k in range(steps - 1):
            li[0:6] = li[0:6] + 0.01 * rng.standard_normal(6) * (k % 2)
            ui[0:6] = li[0:6]
            qi[0:6] *= 1 + 0.02 * rng.standard_normal(6)
            out[k + 1][0][i], out[k + 1][1][i], out[k + 1][2][i] = qi, li, ui
    return out


def closed_loop_oracle(oracle_lib, probs, steps, **opts):
    """(warm results per step, cold results per step): one model per instance updated and re-solved, against a fresh
    setup + solve of the same data."""
    ob = OracleBatch(oracle_lib, probs, **opts)
    warm, cold = [], []
    for k, (q, l, u) in enumerate(steps):
        if k:
            ob.update(q=q, l=l, u=u)
        warm.append(ob.solve())
        cold.append(cold_oracle(oracle_lib, with_vectors(probs, q, l, u), **opts))
    ob.close()
    return warm, cold
