"""Host-side mirror of the reference's native API [REF src/interface.jl:18-773]
over the C ABI declared in include/osqp_amd.h.

The reference is Julia; Julia is not available in this image, so the host side
that is actually exercised is this Python mirror: same names (minus the ``!``
that Python identifiers cannot carry), same argument meaning, same error
behaviour.  ``julia/OSQPAMD.jl`` is the Julia statement of the same layer.

    model = Model()
    setup(model, P=P, q=q, A=A, l=l, u=u, eps_abs=1e-4, ...)
    results = solve(model)
    update(model, q=q_new); update_settings(model, rho=0.2); warm_start(model, x=x0, y=y0)
"""
import ctypes as C
import math

import numpy as np
import scipy.sparse as sp

from . import types as T
from .constants import (
    OSQP_INFTY,
    QDLDL_SOLVER,
    MKL_PARDISO_SOLVER,
    AMD_PCG_SOLVER,
    AMD_DIRECT_SOLVER,
    SOLUTION_PRESENT,
    UPDATABLE_SETTINGS,
    status_map,
)


class OSQPError(RuntimeError):
    """Counterpart of the ErrorException the Julia layer throws on a non-zero exit flag."""


class Info:
    """[REF src/types.jl:219-236]"""

    __slots__ = (
        "iter", "status", "status_val", "status_polish", "obj_val", "pri_res", "dua_res",
        "setup_time", "solve_time", "update_time", "polish_time", "run_time", "rho_updates", "rho_estimate",
    )

    def __init__(self):
        for k in self.__slots__:
            setattr(self, k, 0)
        self.status = "Unsolved"

    def copy_from(self, cinfo):
        """[REF src/types.jl:238-254]; an unknown status_val raises KeyError as in the reference."""
        self.iter = int(cinfo.iter)
        self.status = status_map[int(cinfo.status_val)]
        self.status_val = int(cinfo.status_val)
        self.status_polish = int(cinfo.status_polish)
        for k in ("obj_val", "pri_res", "dua_res", "setup_time", "solve_time", "update_time", "polish_time",
                  "run_time", "rho_estimate"):
            setattr(self, k, float(getattr(cinfo, k)))
        self.rho_updates = int(cinfo.rho_updates)
        return self

    def __repr__(self):
        return "Info(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__) + ")"


class Results:
    """[REF src/types.jl:256-272]"""

    def __init__(self):
        self.x = np.zeros(0)
        self.y = np.zeros(0)
        self.info = Info()
        self.prim_inf_cert = np.zeros(0)
        self.dual_inf_cert = np.zeros(0)

    def resize(self, n, m):
        if self.x.shape[0] != n:
            self.x = np.empty(n)
            self.dual_inf_cert = np.empty(n)
        if self.y.shape[0] != m:
            self.y = np.empty(m)
            self.prim_inf_cert = np.empty(m)
        return self


class Model:
    """[REF src/interface.jl:18-28]  Handle on a library workspace.

    ``lib`` is the dlopen'ed ABI library; the default is the product (HIP)
    library and it is an error if that is not built."""

    def __init__(self, lib=None):
        self.lib = lib if lib is not None else T.load_library()
        self.workspace = T.Workspace_p()  # NULL
        self.lcache = np.zeros(0)
        self.ucache = np.zeros(0)
        self.isempty = True

    def __del__(self):
        try:
            clean(self)
        except Exception:
            pass


def _as_f64(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64))


def _fptr(a):
    return a.ctypes.data_as(T.c_float_p)


def _iptr(a):
    return a.ctypes.data_as(T.c_int_p)


class ManagedCcsc:
    """[REF src/types.jl:21-47]  0-based CSC arrays with Cc_int indices, kept alive
    for the duration of the call; nz = -1 marks compressed-column form."""

    def __init__(self, M, canonical=True):
        M = sp.csc_matrix(M)
        if canonical and not M.has_canonical_format:
            # rows of a column ascending and unique, as a Julia SparseMatrixCSC always is (the library refuses anything else
            # with exit flag 1); on a copy: sp.csc_matrix(M) of a CSC input shares the caller's arrays
            M = M.copy()
            M.sum_duplicates()
        self.m, self.n = M.shape
        self.x = np.ascontiguousarray(M.data, dtype=np.float64)
        self.i = np.ascontiguousarray(M.indices, dtype=np.int64)
        self.p = np.ascontiguousarray(M.indptr, dtype=np.int64)
        self.ccsc = T.Ccsc(len(self.x), self.m, self.n, _iptr(self.p), _iptr(self.i), _fptr(self.x), -1)


def ccsc_to_scipy(c):
    """[REF src/types.jl:49-57]"""
    n, nzmax = int(c.n), int(c.nzmax)
    p = np.array([c.p[k] for k in range(n + 1)], dtype=np.int64)
    i = np.array([c.i[k] for k in range(nzmax)], dtype=np.int64)
    x = np.array([c.x[k] for k in range(nzmax)], dtype=np.float64)
    return sp.csc_matrix((x, i, p), shape=(int(c.m), n))


def default_settings(lib=None):
    """[REF src/types.jl:136-145]"""
    lib = lib if lib is not None else T.load_library()
    s = T.Settings()
    lib.osqp_set_default_settings(C.byref(s))
    return s


def linsys_solver_str_to_int(settings):
    """[REF src/interface.jl:749-773] (+ the two extension names)."""
    v = settings.get("linsys_solver")
    if v is None:
        return
    if not isinstance(v, str):
        raise OSQPError("linsys_solver is required to be a string")
    v = v.lower()
    table = {"qdldl": QDLDL_SOLVER, "mkl pardiso": MKL_PARDISO_SOLVER, "": QDLDL_SOLVER,
             "pcg": AMD_PCG_SOLVER, "direct": AMD_DIRECT_SOLVER}
    if v not in table:
        import warnings

        warnings.warn("Linear system solver not recognized. Using default QDLDL")
    settings["linsys_solver"] = table.get(v, QDLDL_SOLVER)


def make_settings(lib, settings):
    """[REF src/types.jl:147-171]  defaults from C, overridden by keyword, each
    converted to the field's C type; unknown keys are silently ignored."""
    s = default_settings(lib)
    settings = dict(settings)
    linsys_solver_str_to_int(settings)
    for name, ctype in T.Settings._fields_:
        if name in settings:
            v = settings[name]
            if ctype is T.c_float:
                v = float(v)
            else:
                if isinstance(v, float) and not float(v).is_integer():
                    raise OSQPError(f"setting {name} must be an integer")
                v = int(v)
            setattr(s, name, v)
    return s


def _istriu(P):
    """istriu(P) of [REF src/interface.jl:88-90] on a CSC matrix, without building its lower triangle."""
    if P.nnz == 0:
        return True
    first = P.indptr[:-1]
    nonempty = P.indptr[1:] > first
    if P.has_sorted_indices:  # the last stored row of every column decides
        last = P.indices[P.indptr[1:][nonempty] - 1]
        return not np.any(last > np.nonzero(nonempty)[0])
    cols = np.repeat(np.arange(P.shape[1], dtype=P.indices.dtype), np.diff(P.indptr))
    return not np.any(P.indices > cols)


def setup(model, P=None, q=None, A=None, l=None, u=None, comm=None, keep_A_order=False, **settings):
    """[REF src/interface.jl:35-162].  Extension: `comm` (sharded.HostComm / sharded.RcclComm) makes this rank keep
    its row block of one QP shared by all ranks of the communicator (osqp_amd_setup_sharded).  `keep_A_order` (tests): the
    CSC arrays of A go to the library as they are, rows of a column in the caller's order (a plain-C caller of libosqp may
    hand them over unsorted; Julia's SparseMatrixCSC never does)."""
    if P is None:
        if q is not None:
            n = len(q)
        elif A is not None:
            n = A.shape[1]
        else:
            raise OSQPError("The problem does not have any variables!")
    else:
        n = P.shape[0]
    m = 0 if A is None else A.shape[0]
    if (A is None and (l is not None or u is not None)) or (A is not None and l is None and u is None):
        raise OSQPError("A must be supplied together with l and u")
    if A is not None and l is None:
        l = -np.inf * np.ones(m)
    if A is not None and u is None:
        u = np.inf * np.ones(m)
    if P is None:
        P = sp.csc_matrix((n, n))
    if q is None:
        q = np.zeros(n)
    if A is None:
        A = sp.csc_matrix((m, n))
        l = np.zeros(m)
        u = np.zeros(m)
    q, l, u = _as_f64(q), _as_f64(l), _as_f64(u)
    if len(q) != n:
        raise OSQPError("Incorrect dimension of q")
    if len(l) != m:
        raise OSQPError("Incorrect dimensions of l")
    if len(u) != m:
        raise OSQPError("Incorrect dimensions of u")
    P = sp.csc_matrix(P)
    if not _istriu(P):
        P = sp.triu(P, format="csc")
    u = np.minimum(u, OSQP_INFTY)
    l = np.maximum(l, -OSQP_INFTY)
    model.lcache = np.empty(m)
    model.ucache = np.empty(m)
    managedP = ManagedCcsc(P)
    managedA = ManagedCcsc(sp.csc_matrix(A), canonical=False) if keep_A_order else ManagedCcsc(sp.csc_matrix(A))
    stgs = make_settings(model.lib, settings)
    data = T.Data(n, m, C.pointer(managedP.ccsc), C.pointer(managedA.ccsc), _fptr(q), _fptr(l), _fptr(u))
    workspace = T.Workspace_p()
    if comm is None:
        exitflag = model.lib.osqp_setup(C.byref(workspace), C.byref(data), C.byref(stgs))
    else:
        exitflag = model.lib.osqp_amd_setup_sharded(C.byref(workspace), C.byref(data), C.byref(stgs), comm.handle)
        model.comm = comm  # the communicator must outlive the workspace
    model.workspace = workspace
    if exitflag != 0:
        model.workspace = T.Workspace_p()
        raise OSQPError("Error in OSQP setup")
    model.isempty = False
    return model


def setup_generated(model, kind, n, per_row=0, seed=1, comm=None, **settings):
    """Extension: build one of the synthetic families directly where the library
    wants it (HBM for the product) and run setup on it (osqp_amd_setup_generated)."""
    stgs = make_settings(model.lib, settings)
    workspace = T.Workspace_p()
    if comm is None:
        exitflag = model.lib.osqp_amd_setup_generated(C.byref(workspace), kind, n, per_row, seed, C.byref(stgs))
    else:
        exitflag = model.lib.osqp_amd_setup_generated_sharded(C.byref(workspace), kind, n, per_row, seed, C.byref(stgs),
                                                              comm.handle)
        model.comm = comm
    if exitflag != 0:
        raise OSQPError("Error in OSQP setup")
    model.workspace = workspace
    (nn, m) = dimensions(model)
    model.lcache = np.empty(m)
    model.ucache = np.empty(m)
    model.isempty = False
    return model


def solve(model, results=None):
    """[REF src/interface.jl:164-217]"""
    if model.isempty:
        raise OSQPError("You are trying to solve an empty model. Please setup the model before calling solve!().")
    if results is None:
        results = Results()
    model.lib.osqp_solve(model.workspace)  # return value ignored, as in the reference
    workspace = model.workspace.contents
    info = results.info
    info.copy_from(workspace.info.contents)
    solution = workspace.solution.contents
    data = workspace.data.contents
    n, m = int(data.n), int(data.m)
    results.resize(n, m)
    if info.status in SOLUTION_PRESENT:
        C.memmove(results.x.ctypes.data, solution.x, 8 * n)
        C.memmove(results.y.ctypes.data, solution.y, 8 * m)
        results.prim_inf_cert.fill(np.nan)
        results.dual_inf_cert.fill(np.nan)
    else:
        results.x.fill(np.nan)
        results.y.fill(np.nan)
        if info.status in ("Primal_infeasible", "Primal_infeasible_inaccurate"):
            C.memmove(results.prim_inf_cert.ctypes.data, workspace.delta_y, 8 * m)
            results.dual_inf_cert.fill(np.nan)
        elif info.status in ("Dual_infeasible", "Dual_infeasible_inaccurate"):
            results.prim_inf_cert.fill(np.nan)
            C.memmove(results.dual_inf_cert.ctypes.data, workspace.delta_x, 8 * n)
        else:
            results.prim_inf_cert.fill(np.nan)
            results.dual_inf_cert.fill(np.nan)
    if info.status == "Non_convex":
        info.obj_val = math.nan
    return results


def version(lib=None):
    """[REF src/interface.jl:219-221]"""
    lib = lib if lib is not None else T.load_library()
    return lib.osqp_version().decode()


def clean(model):
    """[REF src/interface.jl:223-233]; the workspace pointer may be NULL."""
    ws, model.workspace = model.workspace, T.Workspace_p()
    model.isempty = True
    exitflag = model.lib.osqp_cleanup(ws)
    if exitflag != 0:
        raise OSQPError("Error in OSQP cleanup")


def dimensions(model):
    """[REF src/interface.jl:740-747]"""
    if not model.workspace:
        raise OSQPError("Workspace has not been setup yet")
    data = model.workspace.contents.data.contents
    return int(data.n), int(data.m)


def update_q(model, q):
    """[REF src/interface.jl:235-251]"""
    n, m = dimensions(model)
    q = _as_f64(q)
    if len(q) != n:
        raise OSQPError(f"q must have length n = {n}")
    if model.lib.osqp_update_lin_cost(model.workspace, _fptr(q)) != 0:
        raise OSQPError("Error updating q")


def update_l(model, l):
    """[REF src/interface.jl:253-269]"""
    n, m = dimensions(model)
    l = _as_f64(l)
    if len(l) != m:
        raise OSQPError(f"l must have length m = {m}")
    np.maximum(l, -OSQP_INFTY, out=model.lcache)
    if model.lib.osqp_update_lower_bound(model.workspace, _fptr(model.lcache)) != 0:
        raise OSQPError("Error updating l")


def update_u(model, u):
    """[REF src/interface.jl:271-287]"""
    n, m = dimensions(model)
    u = _as_f64(u)
    if len(u) != m:
        raise OSQPError(f"u must have length m = {m}")
    np.minimum(u, OSQP_INFTY, out=model.ucache)
    if model.lib.osqp_update_upper_bound(model.workspace, _fptr(model.ucache)) != 0:
        raise OSQPError("Error updating u")


def update_bounds(model, l, u):
    """[REF src/interface.jl:289-313]"""
    n, m = dimensions(model)
    l, u = _as_f64(l), _as_f64(u)
    if len(l) != m:
        raise OSQPError(f"l must have length m = {m}")
    if len(u) != m:
        raise OSQPError(f"u must have length m = {m}")
    np.maximum(l, -OSQP_INFTY, out=model.lcache)
    np.minimum(u, OSQP_INFTY, out=model.ucache)
    if model.lib.osqp_update_bounds(model.workspace, _fptr(model.lcache), _fptr(model.ucache)) != 0:
        raise OSQPError("Error updating bounds l and u")


def _prep_idx(idx, nvals, name):
    """[REF src/interface.jl:315-328]  Python callers pass 0-based positions already
    (numpy convention), so there is no in-place shift to undo."""
    if idx is None:
        return None, None
    idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int64))
    if len(idx) != nvals:
        raise OSQPError(f"{name} and {name}_idx must have the same length")
    return idx, _iptr(idx)


def update_P(model, Px, Px_idx=None):
    """[REF src/interface.jl:330-349]"""
    Px = _as_f64(Px)
    keep, ptr = _prep_idx(Px_idx, len(Px), "P")
    if model.lib.osqp_update_P(model.workspace, _fptr(Px), ptr, len(Px)) != 0:
        raise OSQPError("Error updating P")


def update_A(model, Ax, Ax_idx=None):
    """[REF src/interface.jl:351-370]"""
    Ax = _as_f64(Ax)
    keep, ptr = _prep_idx(Ax_idx, len(Ax), "A")
    if model.lib.osqp_update_A(model.workspace, _fptr(Ax), ptr, len(Ax)) != 0:
        raise OSQPError("Error updating A")


def update_P_A(model, Px, Px_idx, Ax, Ax_idx):
    """[REF src/interface.jl:372-406]"""
    Px, Ax = _as_f64(Px), _as_f64(Ax)
    keepP, pP = _prep_idx(Px_idx, len(Px), "P")
    keepA, pA = _prep_idx(Ax_idx, len(Ax), "A")
    if model.lib.osqp_update_P_A(model.workspace, _fptr(Px), pP, len(Px), _fptr(Ax), pA, len(Ax)) != 0:
        raise OSQPError("Error updating P and A")


def _is_device(a):
    """The rule of `batch._batch_array`: a device array is an object with `data_ptr()` and `shape` -- `batch.DeviceArray`, a
    torch CUDA tensor.  (A torch tensor that says it lives on the host is host data, converted like anything else.)"""
    return hasattr(a, "data_ptr") and hasattr(a, "shape") and getattr(a, "is_cuda", True) is not False


def _device_form(who, given):
    """Do the arrays of one call (name -> array, None left out) come in the device form?  One form per call: a mixture
    raises ValueError, before any library call."""
    dev = [k for k, v in given.items() if _is_device(v)]
    if dev and len(dev) != len(given):
        host = [k for k in given if k not in dev]
        raise ValueError(f"{who}: one form per call -- {', '.join(dev)} are device arrays, {', '.join(host)} are not")
    return bool(dev)


def _device_checked(name, a):
    """Element type and layout of a device array, before its shape is known."""
    dt = getattr(a, "dtype", None)
    if dt is not None and "float64" not in str(dt):
        raise ValueError(f"{name}: device arrays must be float64, got {dt}")
    if hasattr(a, "is_contiguous") and not a.is_contiguous():
        raise ValueError(f"{name}: device arrays must be contiguous")
    return tuple(int(k) for k in a.shape)


def _device_vector(name, a, cols):
    """Address of a device array of shape (cols,) -- or (1, cols), what `batch.DeviceArray` calls a vector --, or None when it
    has no entries (the library takes NULL: nothing to say)."""
    shape = _device_checked(name, a)
    if shape not in ((cols,), (1, cols)):
        raise ValueError(f"{name}: expected shape ({cols},), got {shape}")
    return a.data_ptr() if cols > 0 else None


_DERIVATIVES, _DEVICE_FORMS = "adjoint derivatives are", "the device-pointer forms are"


def _symbol(model, name, what):
    """The entry point, or OSQPError when the library does not have it (the CPU oracle has none of the extensions)."""
    fn = getattr(model.lib, name, None)
    if fn is None or fn.argtypes is None:
        raise OSQPError(f"this library does not export {name}: {what} an extension of libosqp_amd.so")
    return fn


def _data_cols(model, matrices=True):
    """Widths of the five data arrays: q [n], l, u [m], Px [nnz(triu P)], Ax [nnz(A)] -- the last two, a read of the library's
    counters, only with `matrices`."""
    n, m = dimensions(model)
    cols = dict(q=n, l=m, u=m)
    if matrices:
        st = stats(model, 4)
        cols.update(Px=int(st[3]), Ax=int(st[1]))
    return cols


def _update_device(model, given):
    """`update` with device arrays: osqp_amd_update_vectors_dev (q, l, u in one call), then osqp_amd_update_values_dev."""
    for name, a in given.items():
        _device_checked(name, a)
    cols = _data_cols(model, "Px" in given or "Ax" in given)
    ptr = {name: _device_vector(name, a, cols[name]) for name, a in given.items()}
    if any(ptr.get(k) is not None for k in ("q", "l", "u")):
        if _symbol(model, "osqp_amd_update_vectors_dev", _DEVICE_FORMS)(model.workspace, ptr.get("q"), ptr.get("l"), ptr.get("u")) != 0:
            raise OSQPError("Error updating q, l, u from device arrays: " + model.lib.osqp_amd_last_error().decode())
    if ptr.get("Px") is not None or ptr.get("Ax") is not None:
        if _symbol(model, "osqp_amd_update_values_dev", _DEVICE_FORMS)(model.workspace, ptr.get("Px"), ptr.get("Ax")) != 0:
            raise OSQPError("Error updating P and A from device arrays: " + model.lib.osqp_amd_last_error().decode())
    elif "Px" in given or "Ax" in given:
        # value arrays without entries only: no data to move, the host form's round (unscale, scale, refactorise) as it is
        update(model, **{k: np.zeros(0) for k in ("Px", "Ax") if k in given})


def update(model, q=None, l=None, u=None, Px=None, Px_idx=None, Ax=None, Ax_idx=None):
    """[REF src/interface.jl:408-440].  Extension: device arrays (`_is_device`: torch CUDA tensors, `batch.DeviceArray`) take
    the device-pointer forms of the library -- no host hop; one form per call, full value arrays only (no Px_idx / Ax_idx).
    The caller has finished producing them (the library runs on its own stream and blocks)."""
    given = {k: v for k, v in (("q", q), ("l", l), ("u", u), ("Px", Px), ("Ax", Ax)) if v is not None}
    if _device_form("update", given):
        if Px_idx is not None or Ax_idx is not None:
            raise ValueError("update: Px_idx / Ax_idx go with host values; the device form replaces the full value arrays")
        return _update_device(model, given)
    if q is not None:
        update_q(model, q)
    if l is not None and u is not None:
        update_bounds(model, l, u)
    elif l is not None:
        update_l(model, l)
    elif u is not None:
        update_u(model, u)
    if Px is not None and Ax is not None:
        update_P_A(model, Px, Px_idx, Ax, Ax_idx)
    elif Px is not None:
        update_P(model, Px, Px_idx)
    elif Ax is not None:
        update_A(model, Ax, Ax_idx)


_INT_SETTINGS = ("max_iter", "polish", "polish_refine_iter", "verbose", "check_termination", "warm_start")
_FLOAT_SETTINGS = ("eps_abs", "eps_rel", "eps_prim_inf", "eps_dual_inf", "rho", "alpha", "delta", "time_limit")


def update_settings(model, **kwargs):
    """[REF src/interface.jl:442-670]  One single-value C call per setting.  As in
    the reference, ``scaled_termination`` is not in UPDATABLE_SETTINGS and the
    branch that would call osqp_update_scaled_termination is unreachable from
    here [REF src/interface.jl:468, 617-628]; the C symbol itself is exported."""
    if not kwargs:
        return
    for key in kwargs:
        if key not in UPDATABLE_SETTINGS:
            raise OSQPError(f"{key} cannot be updated or is not recognized")
    for key in UPDATABLE_SETTINGS:  # fixed order, like the reference's sequence of ifs
        if key not in kwargs or kwargs[key] is None:
            continue
        fn = getattr(model.lib, "osqp_update_" + key)
        v = kwargs[key]
        v = int(v) if key in _INT_SETTINGS else float(v)
        if fn(model.workspace, v) != 0:
            raise OSQPError(f"Error updating {key}")


def warm_start_x(model, x):
    """[REF src/interface.jl:672-684]"""
    n, m = dimensions(model)
    x = _as_f64(x)
    if len(x) != n:
        raise OSQPError("Wrong dimension for variable x")
    if model.lib.osqp_warm_start_x(model.workspace, _fptr(x)) != 0:
        raise OSQPError("Error in warm starting x")


def warm_start_y(model, y):
    """[REF src/interface.jl:686-698]"""
    n, m = dimensions(model)
    y = _as_f64(y)
    if len(y) != m:
        raise OSQPError("Wrong dimension for variable y")
    if model.lib.osqp_warm_start_y(model.workspace, _fptr(y)) != 0:
        raise OSQPError("Error in warm starting y")


def warm_start_x_y(model, x, y):
    """[REF src/interface.jl:700-718]"""
    n, m = dimensions(model)
    x, y = _as_f64(x), _as_f64(y)
    if len(x) != n:
        raise OSQPError("Wrong dimension for variable x")
    if len(y) != m:
        raise OSQPError("Wrong dimension for variable y")
    if model.lib.osqp_warm_start(model.workspace, _fptr(x), _fptr(y)) != 0:
        raise OSQPError("Error in warm starting x and y")


def warm_start(model, x=None, y=None):
    """[REF src/interface.jl:720-732].  Extension: device arrays take osqp_amd_warm_start_dev (the rule of `update`); x alone
    zeroes the stored y and y alone the stored x, as the host forms do."""
    given = {k: v for k, v in (("x", x), ("y", y)) if v is not None}
    if _device_form("warm_start", given):
        for name, a in given.items():
            _device_checked(name, a)
        n, m = dimensions(model)
        ptr = {name: _device_vector(name, a, n if name == "x" else m) for name, a in given.items()}
        if _symbol(model, "osqp_amd_warm_start_dev", _DEVICE_FORMS)(model.workspace, ptr.get("x"), ptr.get("y")) != 0:
            raise OSQPError("Error in warm starting from device arrays: " + model.lib.osqp_amd_last_error().decode())
        return
    if x is not None and y is not None:
        warm_start_x_y(model, x, y)
    elif x is not None:
        warm_start_x(model, x)
    elif y is not None:
        warm_start_y(model, y)


def stats(model, count=27):
    """Extension: osqp_amd_get_stats as a list of floats."""
    out = np.zeros(count)
    k = model.lib.osqp_amd_get_stats(model.workspace, _fptr(out), count)
    return out[:k]


SPMV_LAYOUT_FIELDS = ("kernel", "G", "shift", "B", "Gp", "NG", "tiles", "slices", "padded", "nnz", "compact", "fused", "rshift",
                      "fused_launches")


def spmv_layout(model, which):
    """Extension (tests): osqp_amd_spmv_layout as a dict of ints -- which kernel the products of A (0), A' (1) or P (2)
    run on and the shape of its panel layout (include/osqp_amd.h)."""
    out = np.zeros(len(SPMV_LAYOUT_FIELDS))
    k = model.lib.osqp_amd_spmv_layout(model.workspace, which, _fptr(out), len(out))
    if k != len(out):
        raise OSQPError("osqp_amd_spmv_layout: bad argument")
    return {name: int(v) for name, v in zip(SPMV_LAYOUT_FIELDS, out)}


ADJOINT_GRADS = ("q", "l", "u", "Px", "Ax")
ADJOINT_STATS_FIELDS = ("builds", "solves", "n_low", "n_upp", "kept", "bytes")


_LEADING = dict(ncot="cotangents", ndir="directions")


def _leading(who, what, shapes, width):
    """The leading axis the input arrays of one `adjoint` (what = "ncot") or `jvp` ("ndir") call agree on, host or device form,
    from their shapes (name -> tuple; width: name -> columns): (count, had a leading axis?).  No array: (1, False)."""
    for nm, shp in shapes.items():
        if len(shp) not in (1, 2) or shp[-1] != width[nm] or (len(shp) == 2 and shp[0] < 1):
            raise ValueError(f"{nm}: expected shape ({width[nm]},) or ({what}, {width[nm]}) with {what} >= 1, got {shp}")
    if len({len(shp) for shp in shapes.values()}) > 1:
        raise ValueError(f"{who}: {' and '.join(shapes)} must all have a leading axis or all have none")
    many = any(len(shp) == 2 for shp in shapes.values())
    counts = {shp[0] if many else 1 for shp in shapes.values()}
    if len(counts) > 1:
        raise ValueError(f"{who}: {' and '.join(shapes)} differ in their leading axis, the number of {_LEADING[what]}: {sorted(counts)}")
    return (counts.pop() if counts else 1), many


def _host_inputs(who, what, given, width):
    """The host inputs of `adjoint` / `jvp` (name -> array-like) as float64 C-contiguous arrays [count x cols] (cols may be 0:
    m = 0), with (count, had a leading axis?).  Element types and shapes are checked here, before the library sees a pointer."""
    arrs = {nm: np.asarray(a) for nm, a in given.items()}
    for nm, arr in arrs.items():
        if arr.dtype.kind not in "fiu":
            raise ValueError(f"{nm}: expected a real numeric array, got dtype {arr.dtype}")
    count, many = _leading(who, what, {nm: arr.shape for nm, arr in arrs.items()}, width)
    return {nm: _as_f64(arr).reshape(count, width[nm]) for nm, arr in arrs.items()}, count, many


def _device_empty(model, like, shape):
    """An uninitialised fp64 device array of `shape` beside `like`: a torch tensor when `like` is one, else a
    `batch.DeviceArray` ([1 x cols] for a vector)."""
    import sys

    torch = sys.modules.get("torch")
    if torch is not None and torch.is_tensor(like):
        return torch.empty(shape, dtype=torch.float64, device=like.device)
    from .batch import DeviceArray

    return DeviceArray(model.lib, shape[0] if len(shape) == 2 else 1, shape[-1], getattr(like, "device", 0))


def _device_outputs(model, like, names, shape_of, out):
    """The device arrays a call writes: those of `out` (checked), fresh ones beside `like` for the rest."""
    res = {}
    for k in names:
        shape = shape_of(k)
        a = None if out is None else out.get(k)
        if a is None:
            a = _device_empty(model, like, shape)
        else:
            if not _is_device(a):
                raise ValueError(f"out[{k!r}]: expected a device array")
            got = _device_checked(f"out[{k!r}]", a)
            if got != shape and got != (1,) + shape:
                raise ValueError(f"out[{k!r}]: expected shape {shape}, got {got}")
        res[k] = a
    return res


def _adjoint_device(model, given, want, out):
    shapes = {nm: _device_checked(nm, a) for nm, a in given.items()}
    fn = _symbol(model, "osqp_amd_adjoint_dev", _DEVICE_FORMS)
    n, m = dimensions(model)
    ncot, many = _leading("adjoint", "ncot", shapes, dict(dx=n, dy=m))
    cols = _data_cols(model, "Px" in want or "Ax" in want)
    like = next(iter(given.values()))
    res = _device_outputs(model, like, want + ("act",), lambda k: (m,) if k == "act" else ((ncot, cols[k]) if many else (cols[k],)), out)
    addr = lambda a, width: a.data_ptr() if a is not None and width > 0 else None
    args = [addr(given.get("dx"), n), addr(given.get("dy"), m)] + [addr(res.get(k), cols.get(k, 0)) for k in ADJOINT_GRADS] + [addr(res["act"], m)]
    if any(p is not None for p in args[2:]):  # (m = 0 and only "l" / "u" wanted: nothing to compute)
        if fn(model.workspace, ncot, *args) != 0:
            raise OSQPError("Error in adjoint: " + model.lib.osqp_amd_last_error().decode())
    return res


def adjoint(model, dx=None, dy=None, want=ADJOINT_GRADS, out=None):
    """Extension: osqp_amd_adjoint (include/osqp_amd.h).  From dx = dloss/dx and dy = dloss/dy at the solution of the last
    `solve` (either may be None = 0) the gradients named in `want` -- "q", "l", "u", "Px" (upper triangle of P), "Ax", both
    in the nnz order `update` takes -- as a dict of numpy arrays, plus "act" [m] (-1 lower, 0 inactive, 1 upper).  Inputs
    [n] / [m] give outputs without a leading axis, inputs [ncot x n] / [ncot x m] outputs with one.  `want=()` with no
    cotangent returns "act" alone.  The first call after a solve factorises and keeps the factor (`adjoint_release`).
    Device arrays (the rule of `update`; one form per call) take osqp_amd_adjoint_dev: the gradients and "act" ([m], -1.0 /
    0.0 / 1.0 as the library keeps it) come back as device arrays -- torch tensors beside the inputs when those are tensors,
    `batch.DeviceArray` otherwise -- or are written into the arrays of the dict `out` (name -> device array; the others are
    allocated), as `ResidentBatch.adjoint` has it."""
    want = tuple(want)
    for k in want:
        if k not in ADJOINT_GRADS:
            raise ValueError(f"want: unknown gradient {k!r} (known: {', '.join(ADJOINT_GRADS)})")
    if len(set(want)) != len(want):
        raise ValueError("want: a gradient is named twice")
    if _device_form("adjoint", {nm: v for nm, v in (("dx", dx), ("dy", dy)) if v is not None}):
        return _adjoint_device(model, {nm: v for nm, v in (("dx", dx), ("dy", dy)) if v is not None}, want, out)
    if out is not None:
        raise ValueError("adjoint: out= goes with device arrays; host inputs return numpy arrays")
    fn = _symbol(model, "osqp_amd_adjoint", _DERIVATIVES)
    n, m = dimensions(model)
    got, ncot, many = _host_inputs("adjoint", "ncot", {nm: v for nm, v in (("dx", dx), ("dy", dy)) if v is not None}, dict(dx=n, dy=m))
    if want and not got:
        raise ValueError("adjoint: a gradient is wanted but dx and dy are both None")
    cols = _data_cols(model)
    out = {k: np.full((ncot, cols[k]), np.nan) for k in want}
    act = np.zeros(m)
    ptr = lambda a: None if a is None else _fptr(a)
    if fn(model.workspace, ncot, ptr(got.get("dx")), ptr(got.get("dy")), *(ptr(out.get(k)) for k in ADJOINT_GRADS), _fptr(act)) != 0:
        raise OSQPError("Error in adjoint: " + model.lib.osqp_amd_last_error().decode())
    res = {k: (v if many else v[0]) for k, v in out.items()}
    res["act"] = act.astype(int)
    return res


def _jvp_device(model, given, out):
    shapes = {nm: _device_checked(nm, a) for nm, a in given.items()}
    fn = _symbol(model, "osqp_amd_jvp_dev", _DEVICE_FORMS)
    cols = _data_cols(model, "Px" in given or "Ax" in given)
    n, m = cols["q"], cols["l"]
    ndir, many = _leading("jvp", "ndir", shapes, cols)
    like = next(iter(given.values()))
    width = dict(x=n, y=m, act=m)
    res = _device_outputs(model, like, ("x", "y", "act"), lambda k: (ndir, width[k]) if many and k != "act" else (width[k],), out)
    addr = lambda a, w: a.data_ptr() if a is not None and w > 0 else None
    tang = [addr(given.get(k), cols.get(k, 0)) for k in ADJOINT_GRADS]
    if all(p is None for p in tang):
        raise ValueError("jvp: every tangent given is an array without entries")
    if fn(model.workspace, ndir, *tang, addr(res["x"], n), addr(res["y"], m), addr(res["act"], m)) != 0:
        raise OSQPError("Error in jvp: " + model.lib.osqp_amd_last_error().decode())
    return res


def jvp(model, q=None, l=None, u=None, Px=None, Ax=None, out=None):
    """Extension: osqp_amd_jvp (include/osqp_amd.h).  The forward sensitivities of the solution of the last `solve` along a
    direction of the data: tangents q [n], l, u [m], Px [nnz(P upper)], Ax [nnz(A)] in the nnz order `update` takes (None =
    zero; not all).  Returns a dict "x" (tangent of x), "y" (of the multipliers; zero on inactive rows) and "act" [m].
    Inputs [cols] give outputs without a leading axis, inputs [ndir x cols] outputs with one; all tangents agree on this
    and on ndir.  On a row with l == u only `l` is read.  The factor is `adjoint`'s: whichever is called first after a
    solve builds it, the other reuses it (`adjoint_release`, `adjoint_stats`).  Device arrays (the rule of `update`; one form
    per call) take osqp_amd_jvp_dev and give device arrays, `out` as in `adjoint`."""
    given = [(nm, v) for nm, v in zip(ADJOINT_GRADS, (q, l, u, Px, Ax)) if v is not None]
    if _device_form("jvp", dict(given)):
        return _jvp_device(model, dict(given), out)
    if out is not None:
        raise ValueError("jvp: out= goes with device arrays; host inputs return numpy arrays")
    fn = _symbol(model, "osqp_amd_jvp", _DERIVATIVES)
    if not given:
        raise ValueError("jvp: q, l, u, Px and Ax are all None: at least one tangent is needed")
    cols = _data_cols(model, Px is not None or Ax is not None)
    n, m = cols["q"], cols["l"]
    got, ndir, many = _host_inputs("jvp", "ndir", dict(given), cols)
    tx, ty, act = np.full((ndir, n), np.nan), np.full((ndir, m), np.nan), np.zeros(m)
    ptr = lambda a: None if a is None else _fptr(a)
    if fn(model.workspace, ndir, *(ptr(got.get(k)) for k in ADJOINT_GRADS), _fptr(tx), _fptr(ty), _fptr(act)) != 0:
        raise OSQPError("Error in jvp: " + model.lib.osqp_amd_last_error().decode())
    return dict(x=tx if many else tx[0], y=ty if many else ty[0], act=act.astype(int))


def _any_compact(model):
    """Whether one of A, A', P of the workspace has released its CSR arrays (`spmv_layout`: "compact")."""
    out = np.zeros(len(SPMV_LAYOUT_FIELDS))
    at = SPMV_LAYOUT_FIELDS.index("compact")
    fn = getattr(model.lib, "osqp_amd_spmv_layout", None)
    return fn is not None and any(fn(model.workspace, which, _fptr(out), len(out)) == len(out) and out[at] != 0 for which in (0, 1, 2))


JACOBIAN_OF = ("x", "y")
JACOBIAN_BUDGET = 256 << 20  # bytes: the unit vectors and the largest output of one call of `jacobian` (default chunk)


def jacobian(model, of=("x",), wrt=("q", "l", "u"), mode="auto", out_rows=None, chunk=None):
    """Jacobians of the solution of the last `solve` with respect to the data (`ResidentBatch.jacobian` for a single model):
    a dict {(o, w): [cols(o) x cols(w)]} for o in `of` (a subset of "x", "y") and w in `wrt` (a subset of "q", "l", "u",
    "Px", "Ax"), entry [a, b] the derivative of component a of o with respect to entry b of w, plus "act".  out_rows: a dict
    {"x": indices, "y": indices} that restricts the outputs to these components, in the order given.
    mode="reverse": unit cotangents through `adjoint`, one solve per requested output component; mode="forward": unit
    directions through `jvp`, one solve per column of the `wrt` arrays; "auto": the one with fewer solves (reverse on a tie).
    On a row with l == u the derivative with respect to moving both bounds is in "l" and "u" is zero; an inactive bound has
    a zero column.  chunk: the most unit vectors per call; the chunks are independent calls on the kept factor whose
    results are placed side by side, so the result does not depend on it.  Default: as many as keep the unit vectors and
    the largest output array of one call under 256 MiB together, at least 1.  Nothing is computed on the results."""
    for name in ("osqp_amd_adjoint", "osqp_amd_jvp"):
        _symbol(model, name, _DERIVATIVES)
    of, wrt = tuple(of), tuple(wrt)
    if not of or len(set(of)) != len(of) or any(o not in JACOBIAN_OF for o in of):
        raise ValueError(f"of: expected a non-empty subset of {JACOBIAN_OF} without repeats, got {of!r}")
    if not wrt or len(set(wrt)) != len(wrt) or any(w not in ADJOINT_GRADS for w in wrt):
        raise ValueError(f"wrt: expected a non-empty subset of {ADJOINT_GRADS} without repeats, got {wrt!r}")
    if mode not in ("auto", "reverse", "forward"):
        raise ValueError(f"mode: expected 'auto', 'reverse' or 'forward', got {mode!r}")
    if chunk is not None and (not isinstance(chunk, (int, np.integer)) or isinstance(chunk, bool) or chunk < 1):
        raise ValueError(f"chunk: expected a positive integer, got {chunk!r}")
    wcols = _data_cols(model)
    ocols = dict(x=wcols["q"], y=wcols["l"])
    out_rows = {} if out_rows is None else dict(out_rows)
    idx = {}
    for o in out_rows:
        if o not in of:
            raise ValueError(f"out_rows: {o!r} is not in `of` {of!r}")
    for o in of:
        if o in out_rows:
            a = np.asarray(out_rows[o])
            if a.ndim != 1 or a.dtype.kind not in "iu":
                raise ValueError(f"out_rows[{o!r}]: expected a one-dimensional integer array, got shape {a.shape}, dtype {a.dtype}")
            if a.size and (a.min() < 0 or a.max() >= ocols[o]):
                raise ValueError(f"out_rows[{o!r}]: components must be in [0, {ocols[o]})")
            idx[o] = a.astype(np.int64)
        else:
            idx[o] = np.arange(ocols[o], dtype=np.int64)
    n_rev, n_fwd = sum(len(idx[o]) for o in of), sum(wcols[w] for w in wrt)
    if n_rev == 0 or n_fwd == 0:
        raise ValueError("jacobian: no output component or no data column is asked for")
    if mode == "auto":
        mode = "reverse" if n_rev <= n_fwd else "forward"
        # a compact workspace serves dPx / dAx (reverse) but not the matrix tangents (forward)
        if mode == "forward" and ("Px" in wrt or "Ax" in wrt) and _any_compact(model):
            mode = "reverse"
    reverse = mode == "reverse"
    total = n_rev if reverse else n_fwd
    if chunk is None:
        unit = sum(ocols[o] for o in of) if reverse else n_fwd
        largest = max(wcols[w] for w in wrt) if reverse else max(ocols[o] for o in of)
        chunk = max(1, JACOBIAN_BUDGET // (8 * (unit + largest)))
    chunk = int(min(chunk, total))
    # the solves of the call in order: segment (name, first solve, number) -- the components of each o (reverse), the columns
    # of each w (forward)
    segs, at = [], 0
    for name, width in ([(o, len(idx[o])) for o in of] if reverse else [(w, wcols[w]) for w in wrt]):
        segs.append((name, at, width))
        at += width
    J = {(o, w): np.zeros((len(idx[o]), wcols[w])) for o in of for w in wrt}
    res = {}
    for c0 in range(0, total, chunk):
        c1 = min(c0 + chunk, total)
        nc = c1 - c0
        parts = [(name, max(s0, c0) - c0, min(s0 + w, c1) - c0, max(s0, c0) - s0) for name, s0, w in segs if max(s0, c0) < min(s0 + w, c1)]
        if reverse:
            cot = {o: np.zeros((nc, ocols[o])) for o in of if ocols[o] > 0}
            for o, a, b, p0 in parts:
                cot[o][np.arange(a, b), idx[o][p0:p0 + b - a]] = 1.0
            want = tuple(w for w in wrt if wcols[w] > 0)
            res = adjoint(model, dx=cot.get("x"), dy=cot.get("y"), want=want)
            for o, a, b, p0 in parts:
                for w in want:
                    J[(o, w)][p0:p0 + b - a, :] = res[w][a:b]
        else:
            tan = {w: np.zeros((nc, wcols[w])) for w in wrt if wcols[w] > 0}
            for w, a, b, p0 in parts:
                tan[w][np.arange(a, b), np.arange(p0, p0 + b - a)] = 1.0
            res = jvp(model, **tan)
            for w, a, b, p0 in parts:
                for o in of:
                    if ocols[o] > 0:
                        J[(o, w)][:, p0:p0 + b - a] = res[o][a:b][:, idx[o]].T
    J["act"] = res["act"]
    return J


DEVICE_FORM_FIELDS = ("update_vectors", "update_values", "warm_start", "solution", "adjoint", "jvp")


def solution(model, x=None, y=None, device=0):
    """Extension: osqp_amd_solution_dev -- the solution of the last `solve` read into device arrays: x [n] and y [m] are
    filled where given (device arrays, the rule of `update`), allocated where not (`batch.DeviceArray` [1 x n] / [1 x m] on
    `device`, or torch tensors beside the one that was given).  Returns (x, y); NaN where the solve ended without a solution."""
    given = {k: v for k, v in (("x", x), ("y", y)) if v is not None}
    for name, a in given.items():
        if not _is_device(a):
            raise ValueError(f"solution: {name} must be a device array (a torch CUDA tensor or a batch.DeviceArray)")
        _device_checked(name, a)
    fn = _symbol(model, "osqp_amd_solution_dev", _DEVICE_FORMS)
    n, m = dimensions(model)
    like = next(iter(given.values()), None)
    if like is None:
        from .batch import DeviceArray

        like = DeviceArray(model.lib, 1, n, device)
        given["x"] = like
    res = _device_outputs(model, like, ("x", "y"), lambda k: (n,) if k == "x" else (m,), given)
    if fn(model.workspace, res["x"].data_ptr(), res["y"].data_ptr() if m > 0 else None) != 0:
        raise OSQPError("Error in solution: " + model.lib.osqp_amd_last_error().decode())
    return res["x"], res["y"]


def device_form_calls(model):
    """Extension: osqp_amd_device_form_calls as a dict of ints -- the device-form calls this model has served so far."""
    fn = _symbol(model, "osqp_amd_device_form_calls", _DEVICE_FORMS)
    out = np.zeros(len(DEVICE_FORM_FIELDS))
    if fn(model.workspace, _fptr(out), len(out)) != len(out):
        raise OSQPError("osqp_amd_device_form_calls: bad argument")
    return {name: int(v) for name, v in zip(DEVICE_FORM_FIELDS, out)}


def adjoint_release(model):
    """Extension: drop the factor `adjoint` keeps (it is as large as a polish's)."""
    if _symbol(model, "osqp_amd_adjoint_release", _DERIVATIVES)(model.workspace) != 0:
        raise OSQPError("Error in adjoint_release: " + model.lib.osqp_amd_last_error().decode())


def adjoint_stats(model):
    """Extension: osqp_amd_adjoint_stats as a dict of ints -- factor builds and KKT solves so far, n_low / n_upp of the kept
    factor, whether one is kept, and the device bytes it holds."""
    fn = _symbol(model, "osqp_amd_adjoint_stats", _DERIVATIVES)
    out = np.zeros(len(ADJOINT_STATS_FIELDS))
    if fn(model.workspace, _fptr(out), len(out)) != len(out):
        raise OSQPError("osqp_amd_adjoint_stats: bad argument")
    return {name: int(v) for name, v in zip(ADJOINT_STATS_FIELDS, out)}


ADJOINT_RETAIN_STATS_FIELDS = ("mode", "checks", "reused", "refactorised", "rebuilt_active_set", "rebuilt_failed", "last_rows_changed", "stale")


def adjoint_retain(model, on=True):
    """Extension: osqp_amd_adjoint_retain -- with on=True the factor `adjoint` / `jvp` keep outlives its solution: updates,
    warm starts and solves mark it stale instead of dropping it, and the first derivative call on the next solution checks
    on the device whether any row changed its side.  None did: the factor is reused (after a numeric refactorisation where
    P or A changed); otherwise it is rebuilt as by default.  Settings updates, `derivative_method` and `adjoint_release`
    still drop it.  on=False (the default of every model) drops a stale factor at once.  The results have the bits of the
    default life cycle."""
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError(f"on: expected a bool, got {on!r}")
    fn = _symbol(model, "osqp_amd_adjoint_retain", _DERIVATIVES)
    if fn(model.workspace, 1 if on else 0) != 0:
        raise OSQPError("Error in adjoint_retain: " + model.lib.osqp_amd_last_error().decode())


def adjoint_retain_stats(model):
    """Extension: osqp_amd_adjoint_retain_stats as a dict of ints -- the mode, the checks of a stale factor made so far and
    what became of them (reused, refactorised, rebuilt_active_set, rebuilt_failed), the rows that had changed side at the
    last check, and whether the kept factor is stale now."""
    fn = _symbol(model, "osqp_amd_adjoint_retain_stats", _DERIVATIVES)
    out = np.zeros(len(ADJOINT_RETAIN_STATS_FIELDS))
    if fn(model.workspace, _fptr(out), len(out)) != len(out):
        raise OSQPError("osqp_amd_adjoint_retain_stats: bad argument")
    return {name: int(v) for name, v in zip(ADJOINT_RETAIN_STATS_FIELDS, out)}


DERIVATIVE_METHODS = ("direct", "auto", "iterative")
DERIVATIVE_ITER_STATS_FIELDS = ("builds", "outer_steps", "cg_iters", "last_outer_steps", "last_drop", "kept", "bytes")


def derivative_method(model, method="direct", max_outer=None, rel_drop=None):
    """Extension: osqp_amd_derivative_method -- which KKT solve `adjoint`, `jvp`, `jacobian` and `qp_layer.QPLayer` use on
    this model.  "direct" (the default): the kept factor; a compact workspace and a factor that does not fit are refused.
    "auto": the factor where "direct" builds one, the iterative solve on the operator of the indirect back-end on a compact
    workspace and where the factor does not fit.  "iterative": always the iterative solve (needs `linsys_solver="pcg"` on one
    device).  max_outer (default 40) caps its outer steps, rel_drop (default 1e-10) is the drop of the residual of the
    unregularised system they run to; a solve that misses it makes the derivative call raise.  Drops the derivative state
    the current solution keeps."""
    if method not in DERIVATIVE_METHODS:
        raise ValueError(f"method: expected one of {DERIVATIVE_METHODS}, got {method!r}")
    if max_outer is not None and (not isinstance(max_outer, (int, np.integer)) or isinstance(max_outer, bool) or max_outer < 1):
        raise ValueError(f"max_outer: expected a positive integer or None, got {max_outer!r}")
    if rel_drop is not None and not (isinstance(rel_drop, (float, np.floating)) and 0.0 < rel_drop < 1.0):
        raise ValueError(f"rel_drop: expected a float in (0, 1) or None, got {rel_drop!r}")
    fn = _symbol(model, "osqp_amd_derivative_method", _DERIVATIVES)
    if fn(model.workspace, DERIVATIVE_METHODS.index(method), 0 if max_outer is None else int(max_outer), 0.0 if rel_drop is None else float(rel_drop)) != 0:
        raise OSQPError("Error in derivative_method: " + model.lib.osqp_amd_last_error().decode())


def derivative_iter_stats(model):
    """Extension: osqp_amd_derivative_iter_stats as a dict -- iterative states built, outer steps and CG iterations of the
    derivatives so far, outer steps and reached residual drop ("last_drop", a float) of the last pass, whether the kept
    state is the iterative one, and the device bytes it holds."""
    fn = _symbol(model, "osqp_amd_derivative_iter_stats", _DERIVATIVES)
    out = np.zeros(len(DERIVATIVE_ITER_STATS_FIELDS))
    if fn(model.workspace, _fptr(out), len(out)) != len(out):
        raise OSQPError("osqp_amd_derivative_iter_stats: bad argument")
    return {name: (float(v) if name == "last_drop" else int(v)) for name, v in zip(DERIVATIVE_ITER_STATS_FIELDS, out)}


DUALITY_FIELDS = ("prim_obj", "dual_obj", "gap", "eps_gap", "rule", "gap_refusals")
_DUALITY = "the dual objective and the duality gap are"


def duality_gap_check(model, on=True):
    """Extension: osqp_amd_duality_gap_check -- with on=True every later `solve` also needs the duality gap
    |x'Px + q'x + SC(y)| < eps_abs + eps_rel max(|x'Px|, |q'x|, |SC|) to hold before it ends Solved (10 eps for Solved
    inaccurate), besides the two residual tests (OSQP 1.0's check_dualgap).  Off by default.  The call
    does not move the iterate, rho, the factor or a kept derivative factor."""
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError(f"on: expected a bool, got {on!r}")
    fn = _symbol(model, "osqp_amd_duality_gap_check", _DUALITY)
    if fn(model.workspace, 1 if on else 0) != 0:
        raise OSQPError("Error in duality_gap_check: " + model.lib.osqp_amd_last_error().decode())


def duality(model):
    """Extension: osqp_amd_duality as a dict -- "prim_obj", "dual_obj" and "gap" = prim_obj - dual_obj of the (x, y) the
    model holds (what the last `solve` returned, or the current iterate after `iterate`; NaN dual_obj and gap where the
    status carries no solution), "eps_gap" of the last termination check the rule took part in (NaN: none), "rule" (bool)
    and "gap_refusals": the checks at which both residual tests held and the gap alone refused.  Changes nothing."""
    fn = _symbol(model, "osqp_amd_duality", _DUALITY)
    out = np.zeros(len(DUALITY_FIELDS))
    if fn(model.workspace, _fptr(out), len(out)) != 0:
        raise OSQPError("Error in duality: " + model.lib.osqp_amd_last_error().decode())
    res = {name: float(v) for name, v in zip(DUALITY_FIELDS, out)}
    res["rule"] = bool(out[4])
    res["gap_refusals"] = int(out[5])
    return res
