"""Drives a library (the engine, or the CPU oracle) through a run of pcg_reference.py: the same cases, settings and event
values as the host model's (the values of an event are taken from the reference's record of the run, not drawn again).
Used by test_pcg_reference_host.py (oracle), test_pcg_reference_gpu.py and _pcg_form_worker.py (engine)."""
import ctypes as C

import numpy as np

import osqp_jl_amd as oq
import pcg_reference as pr

EPS = pr.EPS


def iterate(m):
    """The current iterate (osqp_amd_get_iterate), not the stored solution."""
    n, mm = oq.dimensions(m)
    x, y = np.empty(n), np.empty(max(mm, 1))
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert m.lib.osqp_amd_get_iterate(m.workspace, p(x), p(y)) == 0
    return x, y[:mm]


def assert_form(m, panels, what, shift=6):
    """The indirect back-end runs, and the products of A, A' and P are on the panel kernels where the form demands them (a
    matrix with columns beyond one panel of 2^shift, with rows and entries) and on the CSR kernel everywhere else."""
    assert oq.stats(m)[0] == 2, (what, "not the indirect back-end", oq.stats(m)[0])
    n, mm = oq.dimensions(m)
    for which, (rows, cols) in enumerate(((mm, n), (n, mm), (n, n))):
        lay = oq.spmv_layout(m, which)
        want = 2 if panels and rows > 0 and lay["nnz"] > 0 and cols > (1 << shift) else 0
        assert lay["kernel"] == want and (not want or lay["shift"] == shift), (what, which, lay)


def apply_event(m, kind, payload):
    if kind == "q":
        oq.update_q(m, payload)
    elif kind == "rho":
        oq.update_settings(m, rho=payload)
    elif kind == "values":
        Px, Px_idx, Ax, Ax_idx = payload
        Px = None if Px is None or len(Px) == 0 else Px
        Ax = None if Ax is None or len(Ax) == 0 else Ax
        oq.update(m, Px=Px, Px_idx=None if Px is None else Px_idx, Ax=Ax, Ax_idx=None if Ax is None else Ax_idx)
    elif kind == "bounds":
        oq.update(m, l=payload[0], u=payload[1])
    elif kind == "warm_start":
        oq.warm_start(m, x=payload[0], y=payload[1])
    elif kind == "alpha":
        oq.update_settings(m, alpha=payload)
    elif kind != "none":
        raise KeyError(kind)


def drive(lib, name, run, calls, linsys_solver, after_setup=None, get_iterate=False):
    """One workspace through `run` on case `name`; `calls` is the reference's record (pcg_reference.reference_run).  Returns one
    dict per solve call: x, y, status, iter, pri_res, dua_res, rho_updates, stats (and the iterate after the last call)."""
    c = pr.case(name)
    s = pr.run_settings(run, name)
    m = oq.Model(lib)
    oq.setup(m, P=c["P"], q=c["q"], A=c["A"], l=c["l"], u=c["u"], linsys_solver=linsys_solver, scaling=0, rho=c["rho"], verbose=False,
             polish=False, eps_abs=EPS, eps_rel=EPS, **s)
    out = []
    try:
        if after_setup is not None:
            after_setup(m)
        for call in calls:
            apply_event(m, call["kind"], call["payload"])
            r = oq.solve(m)
            out.append(dict(x=r.x.copy(), y=r.y.copy(), status=r.info.status, iter=r.info.iter, pri_res=r.info.pri_res, dua_res=r.info.dua_res,
                            rho_updates=r.info.rho_updates, stats=np.array(oq.stats(m))))
        if get_iterate:
            out[-1]["iterate_x"], out[-1]["iterate_y"] = iterate(m)
    finally:
        oq.clean(m)
    return out


def trajectory_distance(got, calls):
    """The same for every iterate of two records of the host model."""
    d = 0.0
    for g, r in zip(got, calls):
        for (xa, ya), (xb, yb) in zip(g["trajectory"], r["trajectory"]):
            d = max(d, distance(xa, xb), distance(ya, yb))
    return d


def distance(a, ref):
    """max |a - ref| relative to max(1, |ref|inf); 0 for empty vectors."""
    if ref.size == 0:
        return 0.0
    if not np.all(np.isfinite(a)):
        return np.inf
    return float(np.max(np.abs(a - ref)) / max(1.0, float(np.max(np.abs(ref)))))


def errors(got, calls):
    """Worst distances of a driven run to the reference's record, over its calls: x, y, pri_res, dua_res -- each relative to
    max(1, |reference|) (after the warm start of R4 from random vectors pri_res is of the order 1e4)."""
    e = dict(x=0.0, y=0.0, pri=0.0, dua=0.0)
    for g, r in zip(got, calls):
        e["x"] = max(e["x"], distance(g["x"], r["x"]))
        e["y"] = max(e["y"], distance(g["y"], r["y"]))
        e["pri"] = max(e["pri"], abs(g["pri_res"] - r["pri_res"]) / max(1.0, r["pri_res"]))
        e["dua"] = max(e["dua"], abs(g["dua_res"] - r["dua_res"]) / max(1.0, r["dua_res"]))
    return e
