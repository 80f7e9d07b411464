"""Batched small-QP path and its multi-GPU sharding.

`count` independent QPs that share one sparsity pattern are solved one per
workgroup on the device (csrc/batch.hip).  Across GPUs the instance range is cut
into contiguous equal blocks, one per rank (one process per GPU); there is no
communication during the solve.  The only collective is the final gather of
the packed per-rank results [x | y | info]: an in-place all-gather on the
library's own communicator (`sharded.RcclComm`: ncclAllGather over xGMI issued by
libosqp_amd.so itself; `sharded.HostComm`: pinned-host staging + a caller callback)
-- `MpcBatch` below, which needs no torch at all: its packed result array is a `DeviceArray` allocated through the library.
"""
import ctypes as C

import numpy as np

from . import types as T
from .interface import _as_f64, _fptr, _iptr, make_settings, OSQPError
from .constants import UPDATABLE_SETTINGS, status_map

MPC_N, MPC_M = 100, 200
INFO_COLS = 4  # iter, status_val, pri_res, dua_res


class _large_switch:
    """osqp_amd_batch_large set to `on` for the length of one call, then put back to what it was."""

    def __init__(self, lib, on):
        self.lib, self.on = lib, 1 if on else 0

    def __enter__(self):
        self.before = self.lib.osqp_amd_batch_large(self.on)

    def __exit__(self, *exc):
        self.lib.osqp_amd_batch_large(self.before)
        return False


def large_plan(lib, P, A):
    """What the kernel of the opt-in path for 128 < n <= 256 needs for the pattern of P (upper triangle) and A
    (osqp_amd_batch_large_plan; host only, no device is touched): a dict with `lds_bytes` per workgroup, `scratch_bytes` per
    instance (8 n^2: the inverse that every iteration reads) and `tiles_per_wave` of the inversion.  A pattern the kernel
    does not take raises OSQPError with the library's reason."""
    import scipy.sparse as sp

    P = sp.csc_matrix(sp.triu(P)); P.sort_indices()
    A = sp.csc_matrix(A); A.sort_indices()
    n, m = A.shape[1], A.shape[0]
    ndiag = int(np.count_nonzero(P.tocoo().row == P.tocoo().col))
    out = np.zeros(3, dtype=np.int64)
    if lib.osqp_amd_batch_large_plan(n, m, A.nnz, 2 * P.nnz - ndiag, out.ctypes.data) != 0:
        raise OSQPError("Error in batched plan: " + lib.osqp_amd_last_error().decode())
    return {"lds_bytes": int(out[0]), "scratch_bytes": int(out[1]), "tiles_per_wave": int(out[2])}


def large_factor_plan(lib, P, A):
    """What polish, adjoint and JVP need for the pattern of P (upper triangle) and A on a handle with 128 < n <= 256 and
    `large_factor` on (osqp_amd_batch_large_factor_plan; host only): a dict with `lds_bytes` per workgroup, `scratch_bytes`
    per launched instance (8 n^2: the factor) and `nb`, the columns per panel of the blocked factorisation.  A pattern they do
    not take raises OSQPError with the library's reason."""
    import scipy.sparse as sp

    P = sp.csc_matrix(sp.triu(P)); P.sort_indices()
    A = sp.csc_matrix(A); A.sort_indices()
    n, m = A.shape[1], A.shape[0]
    ndiag = int(np.count_nonzero(P.tocoo().row == P.tocoo().col))
    out = np.zeros(3, dtype=np.int64)
    if lib.osqp_amd_batch_large_factor_plan(n, m, A.nnz, 2 * P.nnz - ndiag, out.ctypes.data) != 0:
        raise OSQPError("Error in batched plan: " + lib.osqp_amd_last_error().decode())
    return {"lds_bytes": int(out[0]), "scratch_bytes": int(out[1]), "nb": int(out[2])}


def solve_batch(lib, P, A, Px_all, Ax_all, q_all, l_all, u_all, device=0, large=False, **settings):
    """Host-pointer entry point (osqp_amd_batch_solve).  P (upper triangle) and A are
    scipy CSC matrices giving the shared pattern; the *_all arrays are [count x .].
    large: accept 128 < n <= 256 for this call (osqp_amd_batch_large: the inverse of the reduced KKT matrix read from global
    memory every iteration, slower per iteration than the register kernels); n <= 128 runs as without it."""
    import scipy.sparse as sp

    P = sp.csc_matrix(sp.triu(P)); P.sort_indices()
    A = sp.csc_matrix(A); A.sort_indices()
    n, m = A.shape[1], A.shape[0]
    Px_all, Ax_all = _as_f64(Px_all), _as_f64(Ax_all)
    q_all, l_all, u_all = _as_f64(q_all), _as_f64(l_all), _as_f64(u_all)
    count = q_all.shape[0]
    assert Px_all.shape == (count, P.nnz) and Ax_all.shape == (count, A.nnz)
    assert l_all.shape == (count, m) and u_all.shape == (count, m)
    Pp, Pi = np.ascontiguousarray(P.indptr, dtype=np.int64), np.ascontiguousarray(P.indices, dtype=np.int64)
    Ap, Ai = np.ascontiguousarray(A.indptr, dtype=np.int64), np.ascontiguousarray(A.indices, dtype=np.int64)
    stgs = make_settings(lib, settings)
    x = np.empty((count, n)); y = np.empty((count, m))
    infos = (T.CInfo * count)()
    with _large_switch(lib, large):
        rc = lib.osqp_amd_batch_solve(count, n, m, _iptr(Pp), _iptr(Pi), _fptr(Px_all), _iptr(Ap), _iptr(Ai), _fptr(Ax_all),
                                      _fptr(q_all), _fptr(l_all), _fptr(u_all), C.byref(stgs), _fptr(x), _fptr(y), infos, device)
    if rc != 0:
        raise OSQPError("Error in batched solve: " + lib.osqp_amd_last_error().decode())
    info = np.array([[i.iter, i.status_val, i.pri_res, i.dua_res, i.obj_val, i.rho_updates] for i in infos])
    return x, y, info


SCHEDULE_FIELDS = ("entry", "p1_top", "p1_bot", "bw", "ns", "kew0", "kew1", "kew2", "kew3", "lds_bytes", "instances")


def last_schedule(lib):
    """The schedule of the last batched launch of this process (osqp_amd_batch_last_schedule) as a dict: `entry` (-1 the
    512-thread kernel, -2 the kernel for 128 < n <= 256 -- or, with `lds_bytes` 0, none yet), `p1_top`, `p1_bot`, `bw`, `ns`, `kew` (the four wavefronts' longest rows), `lds_bytes`,
    `instances`."""
    out = np.zeros(len(SCHEDULE_FIELDS), dtype=np.int64)
    got = lib.osqp_amd_batch_last_schedule(out.ctypes.data, len(out))
    if got != len(out):
        raise OSQPError(f"osqp_amd_batch_last_schedule wrote {got} of {len(out)} entries")
    d = {k: int(v) for k, v in zip(SCHEDULE_FIELDS, out)}
    d["kew"] = [d.pop("kew%d" % i) for i in range(4)]
    return d


def shard_range(count, rank, world):
    """Contiguous equal blocks: instance i -> rank floor(i / (count / world))."""
    if count % world != 0:
        raise ValueError("instance count must be divisible by the number of ranks")
    per = count // world
    return rank * per, per


def device_mpc_solver(lib, device, **settings):
    """Returns solve(first, count, seed) -> packed torch tensor [count x (n + m + 4)] on `device`,
    generated and solved in HBM by osqp_amd_batch_solve_generated."""
    import torch

    stgs = make_settings(lib, settings)

    def solve(first, count, seed):
        packed = torch.empty((count, MPC_N + MPC_M + INFO_COLS), dtype=torch.float64, device=f"cuda:{device}")
        x = torch.empty((count, MPC_N), dtype=torch.float64, device=f"cuda:{device}")
        y = torch.empty((count, MPC_M), dtype=torch.float64, device=f"cuda:{device}")
        info = torch.empty((count, INFO_COLS), dtype=torch.float64, device=f"cuda:{device}")
        rc = lib.osqp_amd_batch_solve_generated(first, count, seed, C.byref(stgs), x.data_ptr(), y.data_ptr(), info.data_ptr(), device)
        if rc != 0:
            raise OSQPError("Error in batched solve: " + lib.osqp_amd_last_error().decode())
        packed[:, :MPC_N] = x
        packed[:, MPC_N:MPC_N + MPC_M] = y
        packed[:, MPC_N + MPC_M:] = info
        return packed

    return solve


def split_packed(full):
    """(x, y, info) views of a packed [count x (n + m + 4)] array."""
    return full[:, :MPC_N], full[:, MPC_N:MPC_N + MPC_M], full[:, MPC_N + MPC_M:]


def solve_mpc_sharded(solver, count, seed, rank=0, world=1, gather=None):
    """The host logic of the sharded batch with the two device steps passed in: each rank solves its block with
    `solver(first, count, seed)` -> packed [per x 304]; `gather(full, rank, per)` fills the other ranks' rows of
    `full` in place (one collective).  Returns (x, y, info) views of the whole batch.  `MpcBatch` is the product form
    of the same steps (both inside libosqp_amd.so); the CPU tests drive this one with the oracle and gloo."""
    first, per = shard_range(count, rank, world)
    mine = solver(first, per, seed)
    if world > 1:
        full = mine.new_empty((count, mine.shape[1]))
        full[first:first + per] = mine
        gather(full, rank, per)
    else:
        full = mine
    return split_packed(full)


class DeviceArray:
    """A [rows x cols] fp64 array in HBM allocated through the library (osqp_amd_device_alloc): what `MpcBatch.solve` writes
    into.  `numpy()` downloads it; `clone()` copies it on the device."""

    def __init__(self, lib, rows, cols, device=0):
        self.lib, self.shape, self.device = lib, (int(rows), int(cols)), int(device)
        self.nbytes = 8 * self.shape[0] * self.shape[1]
        self.ptr = lib.osqp_amd_device_alloc(self.nbytes, self.device)
        if not self.ptr:
            raise OSQPError("device allocation failed: " + lib.osqp_amd_last_error().decode())

    def data_ptr(self):
        return self.ptr

    def numpy(self):
        out = np.empty(self.shape)
        if self.lib.osqp_amd_device_copy(out.ctypes.data_as(C.c_void_p), self.ptr, self.nbytes, 0, self.device) != 0:
            raise OSQPError("device copy failed: " + self.lib.osqp_amd_last_error().decode())
        return out

    def upload(self, host):
        """Fill the array from a host array of the same shape; returns self."""
        host = _as_f64(host)
        if host.shape != self.shape:
            raise ValueError(f"expected shape {self.shape}, got {host.shape}")
        if self.lib.osqp_amd_device_copy(self.ptr, host.ctypes.data_as(C.c_void_p), self.nbytes, 1, self.device) != 0:
            raise OSQPError("device copy failed: " + self.lib.osqp_amd_last_error().decode())
        return self

    def clone(self):
        other = DeviceArray(self.lib, self.shape[0], self.shape[1], self.device)
        if self.lib.osqp_amd_device_copy(other.ptr, self.ptr, self.nbytes, 2, self.device) != 0:
            raise OSQPError("device copy failed: " + self.lib.osqp_amd_last_error().decode())
        return other

    def free(self):
        if self.ptr:
            self.lib.osqp_amd_device_free(self.ptr, self.device)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MpcBatch:
    """`total` MPC instances cut over the ranks of `comm` (None: one rank), resident in HBM; `solve()` = rows K11 + K12
    in one library call (osqp_amd_batch_mpc_solve): this rank's block, one workgroup per instance, written in place into
    the packed device array, then one in-place all-gather on the library's communicator."""

    def __init__(self, lib, total, seed=1, device=0, comm=None, **settings):
        self.lib, self.total, self.device, self.comm = lib, int(total), int(device), comm
        self.world = comm.world if comm is not None else 1
        self.rank = comm.rank if comm is not None else 0
        self.first, self.per = shard_range(self.total, self.rank, self.world)
        stgs = make_settings(lib, settings)
        self.handle = C.c_void_p()
        rc = lib.osqp_amd_batch_mpc_create(C.byref(self.handle), self.total, seed, C.byref(stgs),
                                           comm.handle if comm is not None else None, self.device)
        if rc != 0:
            raise OSQPError("Error in batched setup: " + lib.osqp_amd_last_error().decode())

    def alloc(self):
        return DeviceArray(self.lib, self.total, MPC_N + MPC_M + INFO_COLS, self.device)

    def solve(self, out=None):
        packed = self.alloc() if out is None else out
        rc = self.lib.osqp_amd_batch_mpc_solve(self.handle, packed.data_ptr())
        if rc != 0:
            raise OSQPError("Error in batched solve: " + self.lib.osqp_amd_last_error().decode())
        return packed

    def close(self):
        if self.handle:
            self.lib.osqp_amd_batch_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _batch_array(name, a, shape):
    """(address, device form?) of an array argument of `ResidentBatch`: a numpy array (host form; anything array-like is
    converted) or an object with `data_ptr()` and `shape` -- `DeviceArray`, a torch tensor on the handle's device -- (device
    form).  Shape and element type are checked here, before the library sees the pointer."""
    if hasattr(a, "data_ptr"):
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(a.shape)}")
        dt = getattr(a, "dtype", None)
        if dt is not None and "float64" not in str(dt):
            raise ValueError(f"{name}: device arrays must be float64, got {dt}")
        if hasattr(a, "is_contiguous") and not a.is_contiguous():
            raise ValueError(f"{name}: device arrays must be contiguous")
        if getattr(a, "is_cuda", True) is False:
            raise ValueError(f"{name}: a tensor with data_ptr() must live on the device; pass host data as a numpy array")
        return a, a.data_ptr(), 1
    arr = np.asarray(a)
    if arr.dtype.kind not in "fiu":
        raise ValueError(f"{name}: expected a real numeric array, got dtype {arr.dtype}")
    if arr.shape != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {arr.shape}")
    arr = _as_f64(arr)
    return arr, arr.ctypes.data, 0


def selection(rows, count):
    """The instance numbers of a `rows=` argument of `ResidentBatch` as a contiguous int64 array [k], in the order given: an
    integer sequence or array (distinct entries in [0, count)), or a boolean mask of length `count` (the numbers of its True
    entries, ascending).  Checked here, before the library is called: dtype, dimension, range, duplicates, an empty
    selection, more than `count` entries -- each a ValueError."""
    count = int(count)
    arr = np.asarray(rows)
    if arr.ndim == 1 and arr.size == 0:
        raise ValueError("rows: the selection is empty")
    if arr.dtype == object or arr.dtype.kind not in "biu":
        raise ValueError(f"rows: expected integers or a boolean mask, got dtype {arr.dtype}")
    if arr.ndim != 1:
        raise ValueError(f"rows: expected a one-dimensional selection, got shape {arr.shape}")
    if arr.dtype.kind == "b":
        if arr.shape[0] != count:
            raise ValueError(f"rows: a boolean mask must have length {count}, got {arr.shape[0]}")
        arr = np.flatnonzero(arr)
    if arr.size == 0:
        raise ValueError("rows: the selection is empty")
    if arr.size > count:
        raise ValueError(f"rows: {arr.size} entries for a batch of {count} instances")
    if arr.dtype.kind == "u" and arr.max() > np.iinfo(np.int64).max:
        raise ValueError(f"rows: instance {int(arr.max())} is out of range [0, {count})")
    arr = np.ascontiguousarray(arr, dtype=np.int64)
    out_of_range = (arr < 0) | (arr >= count)
    if out_of_range.any():
        raise ValueError(f"rows: instance {int(arr[out_of_range][0])} is out of range [0, {count})")
    seen = np.zeros(count, dtype=bool)
    for i in arr:
        if seen[i]:
            raise ValueError(f"rows: instance {int(i)} is repeated")
        seen[i] = True
    return arr


# The calls of a resident handle that exist for every instance and for a selection, by base name: the symbols are spelled
# out so that a search for one finds its caller (`ResidentBatch._entry`).
_CALL_FORMS = {
    "update_lin_cost": ("osqp_amd_batch_update_lin_cost", "osqp_amd_batch_update_lin_cost_rows"),
    "update_bounds": ("osqp_amd_batch_update_bounds", "osqp_amd_batch_update_bounds_rows"),
    "update_matrices": ("osqp_amd_batch_update_matrices", "osqp_amd_batch_update_matrices_rows"),
    "warm_start": ("osqp_amd_batch_warm_start", "osqp_amd_batch_warm_start_rows"),
    "resolve": ("osqp_amd_batch_resolve", "osqp_amd_batch_resolve_rows"),
    "polish_status": ("osqp_amd_batch_polish_status", "osqp_amd_batch_polish_status_rows"),
    "certificates": ("osqp_amd_batch_certificates", "osqp_amd_batch_certificates_rows"),
    "duality": ("osqp_amd_batch_duality", "osqp_amd_batch_duality_rows"),
    "gap_refusals": ("osqp_amd_batch_gap_refusals", "osqp_amd_batch_gap_refusals_rows"),
    "adjoint": ("osqp_amd_batch_adjoint", "osqp_amd_batch_adjoint_rows"),
    "adjoint_multi": ("osqp_amd_batch_adjoint_multi", "osqp_amd_batch_adjoint_multi_rows"),
    "jvp": ("osqp_amd_batch_jvp", "osqp_amd_batch_jvp_rows"),
}


class ResidentBatch:
    """`count` QPs of the caller's own that share one sparsity pattern, resident in HBM (osqp_amd_batch_setup): the life
    cycle of a single model -- setup, `update`, `warm_start`, `solve`, again and again -- instance by instance.  Scaling is
    computed once from the setup data; every solve starts from the iterate and the rho the last one ended on (with
    `warm_start=False` in the settings: from zero).  P (upper triangle) and A are scipy matrices giving the pattern; the
    *_all arrays are [count x .] as for `solve_batch`.  Array arguments of `update` / `warm_start` and the `out` of `solve`
    may be numpy arrays (host form) or device arrays (`DeviceArray`, torch tensors: no host hop).
    `update`, `warm_start`, `solve`, `adjoint`, `jvp`, `certificates`, `polish_status`, `duality` and `gap_refusals`
    take `rows=`: a selection of the instances (`selection` above: integers in any order, or a boolean mask; always
    host data). Their arrays are then compact, [k x .], row j for instance rows[j]; a selected instance gets the
    bits of the whole-batch call, every other instance is left exactly as it was -- data, record, certificates,
    polish status (include/osqp_amd.h, "*_rows")."""

    def __init__(self, lib, P, A, Px_all, Ax_all, q_all, l_all, u_all, device=0, large=False, large_factor=False, **settings):
        """large: accept 128 < n <= 256 (osqp_amd_batch_large, set for the setup call only: the handle remembers its path).
        By default polish, `adjoint` and `jvp` raise the library's capacity refusal on such a handle ("instance too large to
        polish ..."); large_factor=True (or `large_factor()` later) switches on the forms of those kernels that keep their factor
        in global scratch.  With it, `polish=True` is set up in the order the library asks for: setup
        with polish = 0, the switch, then `update_polish(True)`."""
        import scipy.sparse as sp

        P = sp.csc_matrix(sp.triu(P)); P.sort_indices()
        A = sp.csc_matrix(A); A.sort_indices()
        self.n, self.m, self.nnzP, self.nnzA = A.shape[1], A.shape[0], P.nnz, A.nnz
        if P.shape != (self.n, self.n):
            raise ValueError(f"P: expected shape {(self.n, self.n)}, got {P.shape}")
        q0 = np.asarray(q_all)
        if q0.ndim != 2:
            raise ValueError(f"q_all: expected a [count x {self.n}] array, got shape {q0.shape}")
        self.count = count = q0.shape[0]
        if count == 0:
            raise ValueError("q_all: the batch is empty")
        arrays = []
        for name, a, k in (("Px_all", Px_all, self.nnzP), ("Ax_all", Ax_all, self.nnzA), ("q_all", q_all, self.n),
                           ("l_all", l_all, self.m), ("u_all", u_all, self.m)):
            if hasattr(a, "data_ptr"):
                raise ValueError(f"{name}: the setup data are host arrays (numpy); device arrays are for update / warm_start / solve")
            arrays.append(_batch_array(name, a, (count, k))[0])
        Px, Ax, q, l, u = arrays
        self.lib, self.device, self.handle = lib, int(device), C.c_void_p()
        Pp, Pi = np.ascontiguousarray(P.indptr, dtype=np.int64), np.ascontiguousarray(P.indices, dtype=np.int64)
        Ap, Ai = np.ascontiguousarray(A.indptr, dtype=np.int64), np.ascontiguousarray(A.indices, dtype=np.int64)
        polish_after = bool(large_factor and self.n > 128 and settings.get("polish"))
        if polish_after:
            settings = dict(settings, polish=False)
        stgs = make_settings(lib, settings)
        self.polish_refine_iter = int(stgs.polish_refine_iter)
        with _large_switch(lib, large):
            rc = lib.osqp_amd_batch_setup(C.byref(self.handle), count, self.n, self.m, _iptr(Pp), _iptr(Pi), _fptr(Px), _iptr(Ap), _iptr(Ai),
                                          _fptr(Ax), _fptr(q), _fptr(l), _fptr(u), C.byref(stgs), self.device)
        if rc != 0:
            self.handle = C.c_void_p()
            raise OSQPError("Error in batched setup: " + lib.osqp_amd_last_error().decode())
        if large_factor and self.n > 128:
            try:
                self.large_factor(True)
                if polish_after:
                    self.update_polish(True)
            except Exception:
                self.close()
                raise

    def large_factor(self, on=True):
        """Polish, `adjoint`, `jvp` and `jacobian` on a handle with 128 < n <= 256 (osqp_amd_batch_large_factor, DESIGN.md section
        13.2): off after setup; returns the previous value.  While it is on those kernels keep the factor of M in the
        instance's block of global scratch instead of in LDS; a shape whose other LDS needs exceed the limit is refused where
        polish is asked for and at every derivative call.  Launches nothing.  Switching off puts the refusals back and sets
        polish off.  A handle with n <= 128 raises."""
        before = self.lib.osqp_amd_batch_large_factor(self.handle, 1 if on else 0)
        if before < 0:
            raise OSQPError("Error in batched large_factor: " + self.lib.osqp_amd_last_error().decode())
        return bool(before)

    def _call(self, what, rc):
        if rc != 0:
            raise OSQPError(f"Error in batched {what}: " + self.lib.osqp_amd_last_error().decode())

    def _served(self, rows):
        """(sel, k) of a `rows=` argument: the checked selection and its length, or (None, count) for every instance."""
        if rows is None:
            return None, self.count
        sel = selection(rows, self.count)
        return sel, len(sel)

    def _entry(self, what, name, sel, *args):
        """One call of the library on the handle (`name`: a key of _CALL_FORMS): osqp_amd_batch_<name>(handle, *args) for every
        instance (sel None), or osqp_amd_batch_<name>_rows(handle, rows, k, *args) for the selection; a refusal raises as
        "Error in batched <what>"."""
        whole, subset = _CALL_FORMS[name]
        if sel is None:
            self._call(what, getattr(self.lib, whole)(self.handle, *args))
        else:
            self._call(what, getattr(self.lib, subset)(self.handle, _iptr(sel), len(sel), *args))

    def _one_output(self, what, name, sel, out, shape, device_shape=None):
        """The one output of the entry `name`: out=None -> a new numpy array of `shape`; out = a device array of `device_shape`
        (None: `shape`) -> filled in place.  Returns the array."""
        if out is None:
            res = np.empty(shape)
            self._entry(what, name, sel, res.ctypes.data, 0)
            return res
        if not hasattr(out, "data_ptr"):
            raise ValueError("out: expected a device array (DeviceArray, torch tensor); omit `out` for a numpy result")
        self._entry(what, name, sel, _batch_array("out", out, shape if device_shape is None else device_shape)[1], 1)
        return out

    def _pair(self, names, values, cols, rows=None):
        """The two optional arrays of one library call: both in the same form (host or device); None stays NULL.  `rows`:
        the number of rows they must have (None: count)."""
        rows = self.count if rows is None else rows
        got = [None if v is None else _batch_array(nm, v, (rows, k)) for nm, v, k in zip(names, values, cols)]
        forms = {g[2] for g in got if g is not None}
        if len(forms) > 1:
            raise ValueError(f"{names[0]} and {names[1]} must both be host arrays or both device arrays")
        return got, [None if g is None else g[1] for g in got], (forms.pop() if forms else 0)

    def update(self, q=None, l=None, u=None, Px=None, Ax=None, rows=None):
        """New q / bounds / matrix values for every instance, in the order of `osqp.update!`: q, then the bounds (scaled with
        the stored factors), then the matrices (which re-equilibrate, with the q, l, u just given).  Nothing is changed by a
        call whose arguments fail the checks; `l > u` in any instance raises and leaves the bounds as they were.
        rows: a selection (`selection`); the arrays are then [k x .] and only those instances change and re-equilibrate."""
        sel, k = self._served(rows)
        qa = None if q is None else _batch_array("q", q, (k, self.n))
        keep_b, bounds, where_b = self._pair(("l", "u"), (l, u), (self.m, self.m), k)
        keep_m, mats, where_m = self._pair(("Px", "Ax"), (Px, Ax), (self.nnzP, self.nnzA), k)
        if keep_b[0] is not None and keep_b[1] is not None and not where_b and np.any(keep_b[0][0] > keep_b[1][0]):
            raise OSQPError("Error in batched update: lower bound greater than upper bound")
        if qa is not None:
            self._entry("update", "update_lin_cost", sel, qa[1], qa[2])
        if bounds[0] is not None or bounds[1] is not None:
            self._entry("update", "update_bounds", sel, bounds[0], bounds[1], where_b)
        if mats[0] is not None or mats[1] is not None:
            self._entry("update", "update_matrices", sel, mats[0], mats[1], where_m)

    def warm_start(self, x=None, y=None, rows=None):
        """Start the next solve from x and / or y (caller's units, [count x n] / [count x m]); a missing one is zero.
        rows: a selection (`selection`); x / y are then [k x .] and only the iterates of those instances change."""
        sel, k = self._served(rows)
        keep, ptrs, where = self._pair(("x", "y"), (x, y), (self.n, self.m), k)
        if ptrs[0] is not None or ptrs[1] is not None:
            self._entry("warm start", "warm_start", sel, ptrs[0], ptrs[1], where)

    def solve(self, out=None, rows=None):
        """Solve every instance -> (x [count x n], y [count x m], info [count x 6]: iter, status_val, pri_res, dua_res,
        obj_val, rho_updates).  out=None: numpy arrays; out=(x, y, info) of device arrays: written in place and returned.
        rows: a selection (`selection`): only those instances are launched, the results are [k x .] (`alloc(k)`), and every
        other instance keeps its iterate, rho, certificates, polish status and info row."""
        sel, k = self._served(rows)
        if out is None:
            x, y, info = np.empty((k, self.n)), np.empty((k, self.m)), np.empty((k, 6))
            self._entry("solve", "resolve", sel, x.ctypes.data, y.ctypes.data, info.ctypes.data, 0)
            return x, y, info
        if len(out) != 3:
            raise ValueError("out: expected (x, y, info)")
        ptrs = []
        for name, a, cols in (("out[0]", out[0], self.n), ("out[1]", out[1], self.m), ("out[2]", out[2], 6)):
            if a is None and cols == 0:
                ptrs.append(None)
                continue
            if not hasattr(a, "data_ptr"):
                raise ValueError(f"{name}: expected a device array (DeviceArray, torch tensor); omit `out` for numpy results")
            ptrs.append(_batch_array(name, a, (k, cols))[1])
        self._entry("solve", "resolve", sel, ptrs[0], ptrs[1], ptrs[2], 1)
        return out

    def polish_status(self, out=None, rows=None):
        """status_polish of every instance from its own last `solve()` (whole or `rows=`): 1 accepted, -1 refused, 0 not polished (the instance was
        not Solved, or `polish` is off).  out=None: a numpy int array [count]; out = a device array [count x 1] of float64:
        filled in place and returned.  rows: a selection (`selection`); the result is [k] ([k x 1]), entry j for instance
        rows[j], gathered on the device."""
        sel, k = self._served(rows)
        st = self._one_output("polish status", "polish_status", sel, out, (k,), (k, 1))
        return st.astype(np.int64) if out is None else st

    def update_polish(self, polish, polish_refine_iter=None):
        """Switch polishing of the following solves on (1 / True) or off (0 / False), as `update_settings(polish=...)` does
        for a single model; `polish_refine_iter` (>= 0) is kept when None.  Anything else raises and changes nothing."""
        if isinstance(polish, (bool, np.bool_)):
            polish = int(polish)
        if not isinstance(polish, (int, np.integer)) or polish not in (0, 1):
            raise ValueError(f"polish: expected 0 or 1, got {polish!r}")
        if polish_refine_iter is None:
            polish_refine_iter = getattr(self, "polish_refine_iter", 3)
        if not isinstance(polish_refine_iter, (int, np.integer)) or isinstance(polish_refine_iter, bool) or polish_refine_iter < 0:
            raise ValueError(f"polish_refine_iter: expected a nonnegative integer, got {polish_refine_iter!r}")
        self._call("update", self.lib.osqp_amd_batch_update_polish(self.handle, int(polish), int(polish_refine_iter)))
        self.polish_refine_iter = int(polish_refine_iter)

    # what `update_settings` takes: the list of a single model, and scaled_termination, for which the C ABI has a symbol too
    SETTINGS = tuple(UPDATABLE_SETTINGS) + ("scaled_termination",)

    def update_settings(self, **kw):
        """New values for settings of the following solves, as `update_settings` does for a single model: the names of
        `constants.UPDATABLE_SETTINGS` and `scaled_termination`, each checked by the rule of the single-model function
        (osqp_amd_batch_update_setting).  Any other name raises before the library is called; values of None are skipped.
        `rho` also replaces the rho of every instance, adapted or not; the iterate stays.  The calls are issued in the order
        of the list; one that is refused raises and leaves its setting (and those after it) unchanged."""
        for key in kw:
            if key not in self.SETTINGS:
                raise OSQPError(f"{key} cannot be updated or is not recognized")
        for key in self.SETTINGS:
            value = kw.get(key)
            if value is None:
                continue
            self._call("settings update", self.lib.osqp_amd_batch_update_setting(self.handle, key.encode(), float(value)))
            if key == "polish_refine_iter":
                self.polish_refine_iter = int(value)

    def certificates(self, out=None, rows=None):
        """(prim_inf_cert [count x m], dual_inf_cert [count x n]) of every instance's own last `solve()` (whole or `rows=`): row i of the first is the direction
        that proves instance i primal infeasible (status -3 or 3), of the second dual infeasible (-4 or 4), each with
        largest entry +-1 as a single model's results carry them; every other row is NaN, and all rows before the first
        solve.  out=None: numpy arrays; out=(p, d) of device arrays, either may be None: filled in place and returned.
        With m = 0 the first element is None.  rows: a selection (`selection`); the arrays are [k x .], row j for instance
        rows[j], gathered on the device."""
        sel, k = self._served(rows)
        if out is None:
            p = np.empty((k, self.m)) if self.m else None
            d = np.empty((k, self.n))
            self._entry("certificates", "certificates", sel, None if p is None else p.ctypes.data, d.ctypes.data, 0)
            return p, d
        if len(out) != 2:
            raise ValueError("out: expected (prim_inf_cert, dual_inf_cert)")
        ptrs = []
        for name, a, cols in (("out[0]", out[0], self.m), ("out[1]", out[1], self.n)):
            if a is None:
                ptrs.append(None)
                continue
            if not hasattr(a, "data_ptr"):
                raise ValueError(f"{name}: expected a device array (DeviceArray, torch tensor); omit `out` for numpy results")
            ptrs.append(_batch_array(name, a, (k, cols))[1])
        if ptrs[1] is None and (ptrs[0] is None or self.m == 0):
            raise ValueError("out: no certificate was asked for")
        self._entry("certificates", "certificates", sel, ptrs[0], ptrs[1], 1)
        return (None if self.m == 0 else out[0]), out[1]

    def duality(self, out=None, rows=None):
        """[count x 3]: prim_obj, dual_obj and gap = prim_obj - dual_obj of the pair (x, y) every instance's last `solve()`
        returned, in the caller's units (osqp_amd_batch_duality); a NaN row where that solve left no
        solution.  Every instance served must be current (solved after its last update or warm start).  out=None: a numpy
        array; out = a device array [count x 3] of float64: filled in place and returned.  rows: a selection (`selection`);
        the result is [k x 3], row j for instance rows[j], and only these must be current.  Only reads the handle."""
        sel, k = self._served(rows)
        return self._one_output("duality", "duality", sel, out, (k, 3))

    def duality_gap_check(self, on=True):
        """The duality gap as a third termination test of every later `solve()`, whole or `rows=`
        (osqp_amd_batch_duality_gap_check): |gap| < eps_abs + eps_rel max(|x'Px|, |q'x|, |SC|), evaluated
        inside the solve kernels at the checks where both residual tests hold.  An instance whose gap holds there stops where
        it stopped before, with the same bits; the others iterate on.  Off by default.  Drops nothing of the handle (iterate,
        rho, which instances are current, certificates, polish status); the refusal counts start from zero."""
        self._call("duality_gap_check", self.lib.osqp_amd_batch_duality_gap_check(self.handle, 1 if on else 0))

    def gap_refusals(self, out=None, rows=None):
        """[count]: how many checks of every instance's own last `solve()` the gap test alone refused
        (osqp_amd_batch_gap_refusals); zeros while the rule is off.  out=None: a numpy array of float64; out = a device array
        [count] of float64: filled in place and returned.  rows: a selection (`selection`); the result is [k], entry j for
        instance rows[j].  Only reads the handle."""
        sel, k = self._served(rows)
        return self._one_output("gap_refusals", "gap_refusals", sel, out, (k,))

    ADJOINT_WANT = ("q", "l", "u", "Px", "Ax")

    def _adjoint_cols(self):
        return dict(q=self.n, l=self.m, u=self.m, Px=self.nnzP, Ax=self.nnzA, act=self.m, status=1)

    def adjoint(self, dx=None, dy=None, want=ADJOINT_WANT, out=None, rows=None):
        """Gradients of a scalar loss with respect to the data, through the solutions of the last `solve()`
        (osqp_amd_batch_adjoint): dx [count x n], dy [count x m] are the loss's gradients with respect to x and y (None: zero;
        not both).  Returns a dict with the entries of `want` -- "q" [count x n], "l", "u" [count x m], "Px" [count x nnz(P
        upper)], "Ax" [count x nnz(A)] -- plus "act" [count x m] (-1 lower, 1 upper, 0 inactive) and "status" (1
        differentiated, 0 no solution, -1 factorisation failed; rows with status != 1 are zeros).  Entries of width 0 (m = 0)
        are left out.  Host form: numpy dx / dy, out=None, numpy results ("act" and "status" [count] as integers).  Device
        form: dx / dy device arrays and `out` a dict of float64 device arrays for the entries of `want` and, optionally,
        "act" and "status" ([count x 1]); they are filled in place and `out` is returned.  The handle must hold the solution
        of its current data, for EVERY instance: a `solve()` that served it since its last `update` / `warm_start` (`rows=` calls
        count per instance; the refusal names the first stale one).  Where the active constraints of an instance
        are dependent the derivative does not exist and the regularised answer is returned (see include/osqp_amd.h).
        rows: a selection (`selection`): a launch of k workgroups; dx, dy and every result are [k x .], row j for instance
        rows[j] with the bits of row rows[j] of the whole call, and only the SELECTED instances must hold a current solution
        (the refusal names the first stale one in the order of `rows`).
        Several cotangents at once: dx / dy with a leading axis, [ncot x count x .] ([ncot x k x .] with `rows`), both with the
        same number of dimensions and the same ncot (osqp_amd_batch_adjoint_multi) -- one launch, one factorisation per
        instance, one solve per cotangent, and cotangent c has the bits of a call with that pair alone.  The gradients are then
        shaped like the cotangents, [ncot x count x .]; "act" [count x m] and "status" [count] stay per instance."""
        sel, cnt = self._served(rows)
        cols = self._adjoint_cols()
        want = tuple(want)
        for w in want:
            if w not in self.ADJOINT_WANT:
                raise ValueError(f"want: unknown gradient {w!r}; expected a subset of {self.ADJOINT_WANT}")
        if dx is None and dy is None:
            raise ValueError("dx and dy: at least one incoming gradient is needed")
        dims = {k: len(tuple(v.shape)) if hasattr(v, "data_ptr") else np.asarray(v).ndim for k, v in (("dx", dx), ("dy", dy)) if v is not None}
        if len(set(dims.values())) > 1 or next(iter(dims.values())) not in (2, 3):
            raise ValueError(f"dx and dy: expected both [count x cols] or both [ncot x count x cols], got dimensions {dims}")
        many = next(iter(dims.values())) == 3
        if many:
            ncots = {k: int((v.shape if hasattr(v, "data_ptr") else np.asarray(v).shape)[0]) for k, v in (("dx", dx), ("dy", dy)) if v is not None}
            if len(set(ncots.values())) > 1:
                raise ValueError(f"dx and dy: they must carry the same number of cotangents, got {ncots}")
            ncot = next(iter(ncots.values()))
            if ncot < 1:
                raise ValueError("dx and dy: ncot must be at least 1")
        lead = (ncot, cnt) if many else (cnt,)
        got = [None if v is None else _batch_array(nm, v, lead + (k,)) for nm, v, k in (("dx", dx, self.n), ("dy", dy, self.m))]
        forms = {g[2] for g in got if g is not None}
        if len(forms) > 1:
            raise ValueError("dx and dy must both be host arrays or both device arrays")
        ptrs, where = [None if g is None else g[1] for g in got], forms.pop()
        oshape = {k: ((cnt, cols[k]) if k in ("act", "status") else lead + (cols[k],)) for k in cols}
        names = [k for k in self.ADJOINT_WANT + ("act", "status") if cols[k] > 0]
        if not where:
            if out is not None:
                raise ValueError("out: host gradients (numpy dx / dy) return numpy arrays; pass device arrays for dx / dy to fill `out`")
            res = {k: np.empty(oshape[k]) for k in names if k in want or k in ("act", "status")}
            addr = {k: v.ctypes.data for k, v in res.items()}
        else:
            if not isinstance(out, dict):
                raise ValueError("out: device gradients need a dict of device arrays to fill, one per entry of `want`")
            for k in out:
                if k not in cols:
                    raise ValueError(f"out: unknown entry {k!r}")
            addr = {}
            for k in names:
                if k in out and (k in want or k in ("act", "status")):
                    if not hasattr(out[k], "data_ptr"):
                        raise ValueError(f"out[{k!r}]: expected a device array (DeviceArray, torch tensor)")
                    addr[k] = _batch_array(f"out[{k!r}]", out[k], oshape[k])[1]
                elif k in want:
                    raise ValueError(f"out: no array for the wanted gradient {k!r}")
            res = out
        tail = [ptrs[0], ptrs[1]] + [addr.get(k) for k in self.ADJOINT_WANT] + [addr.get("act"), addr.get("status"), where]
        if many:
            self._entry("adjoint", "adjoint_multi", sel, ncot, *tail)
        else:
            self._entry("adjoint", "adjoint", sel, *tail)
        if not where:
            if "act" in res:
                res["act"] = res["act"].astype(np.int64)
            res["status"] = res["status"].ravel().astype(np.int64)
        return res

    JVP_TANGENTS = ("q", "l", "u", "Px", "Ax")

    def jvp(self, q=None, l=None, u=None, Px=None, Ax=None, out=None, rows=None):
        """Forward sensitivities of the solutions of the last `solve()` along directions of the data (osqp_amd_batch_jvp): the
        tangents q [count x n], l, u [count x m], Px [count x nnz(P upper)], Ax [count x nnz(A)] (None: zero; not all), or
        each with a leading axis [ndir x count x .] for several directions at once -- one launch, one factorisation per
        instance, one solve per direction, and direction d has the bits of a call with that direction alone.  All tangents
        have the same number of dimensions and the same ndir.  Returns a dict: "x" (tangent of the solution), "y" (of the
        multipliers; zero on inactive rows), shaped like the tangents, "act" [count x m] (-1 lower, 1 upper, 0 inactive) and
        "status" (1 differentiated, 0 no solution, -1 factorisation failed; rows with status != 1 are zeros).  "y" and "act"
        are left out when m = 0.  On a row with l == u only the tangent `l` is read; a tangent of an inactive bound has no
        effect.  Host form: numpy tangents, out=None, numpy results ("act" and "status" [count] as integers).  Device form:
        device arrays and `out` a dict of float64 device arrays -- "x" and (m > 0) "y", optionally "act" [count x m] and
        "status" [count x 1] -- filled in place and returned.  The handle must hold the solution of its current data for
        EVERY instance, as for `adjoint`.  rows: a selection (`selection`): a launch of k workgroups; the tangents and the
        results are [k x .] / [ndir x k x .], "act" [k x m], "status" [k], row j for instance rows[j] with the bits of row rows[j]
        of the whole call, and only the SELECTED instances must hold a current solution."""
        sel, cnt = self._served(rows)
        cols = dict(q=self.n, l=self.m, u=self.m, Px=self.nnzP, Ax=self.nnzA)
        given = {k: v for k, v in zip(self.JVP_TANGENTS, (q, l, u, Px, Ax)) if v is not None}
        if not given:
            raise ValueError("q, l, u, Px, Ax: at least one tangent is needed")
        dims = {k: len(tuple(v.shape)) if hasattr(v, "data_ptr") else np.asarray(v).ndim for k, v in given.items()}
        if len(set(dims.values())) > 1 or next(iter(dims.values())) not in (2, 3):
            raise ValueError(f"tangents: expected all [count x cols] or all [ndir x count x cols], got dimensions {dims}")
        many = next(iter(dims.values())) == 3
        first = next(iter(given.values()))
        ndir = int((first.shape if hasattr(first, "data_ptr") else np.asarray(first).shape)[0]) if many else 1
        if ndir < 1:
            raise ValueError("tangents: ndir must be at least 1")
        lead = (ndir, cnt) if many else (cnt,)
        got = {k: _batch_array(k, v, lead + (cols[k],)) for k, v in given.items()}
        forms = {g[2] for g in got.values()}
        if len(forms) > 1:
            raise ValueError("tangents: they must all be host arrays or all device arrays")
        where = forms.pop()
        ocols = dict(x=self.n, y=self.m, act=self.m, status=1)
        oshape = dict(x=lead + (self.n,), y=lead + (self.m,), act=(cnt, self.m), status=(cnt, 1))
        names = [k for k in ("x", "y", "act", "status") if ocols[k] > 0]
        if not where:
            if out is not None:
                raise ValueError("out: host tangents (numpy) return numpy arrays; pass device arrays for the tangents to fill `out`")
            res = {k: np.empty(oshape[k]) for k in names}
            addr = {k: v.ctypes.data for k, v in res.items()}
        else:
            if not isinstance(out, dict):
                raise ValueError("out: device tangents need a dict of device arrays to fill: x, y")
            for k in out:
                if k not in ocols:
                    raise ValueError(f"out: unknown entry {k!r}")
            addr = {}
            for k in names:
                if k in out:
                    if not hasattr(out[k], "data_ptr"):
                        raise ValueError(f"out[{k!r}]: expected a device array (DeviceArray, torch tensor)")
                    addr[k] = _batch_array(f"out[{k!r}]", out[k], oshape[k])[1]
                elif k in ("x", "y"):
                    raise ValueError(f"out: no array for {k!r}")
            res = out
        tail = [ndir] + [got[k][1] if k in got else None for k in self.JVP_TANGENTS]
        tail += [addr.get("x"), addr.get("y"), addr.get("act"), addr.get("status"), where]
        self._entry("jvp", "jvp", sel, *tail)
        if not where:
            if "act" in res:
                res["act"] = res["act"].astype(np.int64)
            res["status"] = res["status"].ravel().astype(np.int64)
        return res

    JACOBIAN_OF = ("x", "y")
    JACOBIAN_BUDGET = 256 << 20  # bytes: the unit vectors and the largest output of one launch of `jacobian` (default chunk)

    def jacobian(self, of=("x",), wrt=("q", "l", "u"), mode="auto", rows=None, out_rows=None, chunk=None, device=False):
        """Jacobians of the solutions of the last `solve()` with respect to the data, instance by instance: a dict
        {(o, w): [count x cols(o) x cols(w)]} for o in `of` (a subset of "x", "y") and w in `wrt` (a subset of "q", "l", "u",
        "Px", "Ax"; the matrices in the setup's pattern order), entry [i, a, b] the derivative of component a of o with respect to
        entry b of w of instance i, plus "act" and "status" as `adjoint` / `jvp` return them (an instance with status != 1 has
        zeros).  out_rows: a dict {"x": indices, "y": indices} that restricts the outputs of `of` to these components (cols(o)
        is then their number, in the order given) -- for an MPC instance the indices of the first input.
        mode="reverse": unit cotangents through `adjoint` with a leading axis, one solve per requested output component;
        mode="forward": unit directions through `jvp`, one solve per column of the `wrt` arrays; "auto": the one with fewer
        solves (reverse on a tie).  Each is the plain derivative of the active-set solution: on a row with l == u the
        derivative with respect to moving both bounds is in "l" and "u" is zero; an inactive bound has a zero column.
        chunk: the most cotangents / directions per launch; the chunks of a call are independent launches whose results are
        concatenated, so the result does not depend on it.  Default: as many as keep the unit vectors (every cotangent or
        tangent array of the launch) and the largest output array of one launch under 256 MiB together, at least 1.
        rows: a selection (`selection`): the arrays are [k x . x .], entry j for instance rows[j].  device=False: numpy
        results; device=True: the unit vectors are made and the results returned as torch tensors on the handle's device
        (no host hop).  Nothing is computed on the results: they are transposed and placed."""
        sel, cnt = self._served(rows)
        of, wrt = tuple(of), tuple(wrt)
        wcols = dict(q=self.n, l=self.m, u=self.m, Px=self.nnzP, Ax=self.nnzA)
        ocols = dict(x=self.n, y=self.m)
        if not of or len(set(of)) != len(of) or any(o not in self.JACOBIAN_OF for o in of):
            raise ValueError(f"of: expected a non-empty subset of {self.JACOBIAN_OF} without repeats, got {of!r}")
        if not wrt or len(set(wrt)) != len(wrt) or any(w not in self.ADJOINT_WANT for w in wrt):
            raise ValueError(f"wrt: expected a non-empty subset of {self.ADJOINT_WANT} without repeats, got {wrt!r}")
        if mode not in ("auto", "reverse", "forward"):
            raise ValueError(f"mode: expected 'auto', 'reverse' or 'forward', got {mode!r}")
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
        if chunk is not None and (not isinstance(chunk, (int, np.integer)) or isinstance(chunk, bool) or chunk < 1):
            raise ValueError(f"chunk: expected a positive integer, got {chunk!r}")
        n_rev, n_fwd = sum(len(idx[o]) for o in of), sum(wcols[w] for w in wrt)
        if n_rev == 0 or n_fwd == 0:
            raise ValueError("jacobian: no output component or no data column is asked for")
        if mode == "auto":
            mode = "reverse" if n_rev <= n_fwd else "forward"
        reverse = mode == "reverse"
        total = n_rev if reverse else n_fwd
        if chunk is None:
            unit = sum(ocols[o] for o in of) if reverse else n_fwd
            largest = max(wcols[w] for w in wrt) if reverse else max(ocols[o] for o in of)
            chunk = max(1, self.JACOBIAN_BUDGET // (8 * cnt * (unit + largest)))
        chunk = int(min(chunk, total))

        if device:
            import torch

            dev = torch.device("cuda", self.device)

            def zeros(*shape):
                return torch.zeros(shape, dtype=torch.float64, device=dev)

            def empty(*shape):
                return torch.empty(shape, dtype=torch.float64, device=dev)

            def index(a):
                return torch.as_tensor(a, device=dev)

            def moved(a, perm):
                return a.permute(*perm)

            def ready():
                torch.cuda.current_stream(dev).synchronize()
        else:
            zeros, empty, index, ready = (lambda *shape: np.zeros(shape)), (lambda *shape: np.empty(shape)), (lambda a: a), (lambda: None)

            def moved(a, perm):
                return np.transpose(a, perm)

        # the solves of the call in order: segment (name, first solve, number) -- the components of each o (reverse), the
        # columns of each w (forward)
        segs, at = [], 0
        for name, width in ([(o, len(idx[o])) for o in of] if reverse else [(w, wcols[w]) for w in wrt]):
            segs.append((name, at, width))
            at += width
        J = {(o, w): zeros(cnt, len(idx[o]), wcols[w]) for o in of for w in wrt}
        res = {}
        for c0 in range(0, total, chunk):
            c1 = min(c0 + chunk, total)
            nc = c1 - c0
            # the part [a, b) of each segment that falls into this chunk, as positions of the chunk and of the segment
            parts = [(name, max(s0, c0) - c0, min(s0 + w, c1) - c0, max(s0, c0) - s0) for name, s0, w in segs if max(s0, c0) < min(s0 + w, c1)]
            if reverse:
                cot = {o: zeros(nc, cnt, ocols[o]) for o in of if ocols[o] > 0}
                for o, a, b, p0 in parts:
                    cot[o][index(np.arange(a, b)), :, index(idx[o][p0:p0 + b - a])] = 1.0
                want = tuple(w for w in wrt if wcols[w] > 0)
                out = None
                if device:
                    out = {w: empty(nc, cnt, wcols[w]) for w in want}
                    out.update(act=empty(cnt, self.m), status=empty(cnt, 1))
                    if self.m == 0:
                        del out["act"]
                ready()
                res = self.adjoint(dx=cot.get("x"), dy=cot.get("y"), want=want, out=out, rows=sel)
                for o, a, b, p0 in parts:
                    for w in want:
                        J[(o, w)][:, p0:p0 + b - a, :] = moved(res[w][a:b], (1, 0, 2))
            else:
                tan = {w: zeros(nc, cnt, wcols[w]) for w in wrt if wcols[w] > 0}
                for w, a, b, p0 in parts:
                    tan[w][index(np.arange(a, b)), :, index(np.arange(p0, p0 + b - a))] = 1.0
                out = None
                if device:
                    out = dict(x=empty(nc, cnt, self.n), y=empty(nc, cnt, self.m), act=empty(cnt, self.m), status=empty(cnt, 1))
                    if self.m == 0:
                        del out["y"], out["act"]
                ready()
                res = self.jvp(**tan, out=out, rows=sel)
                for w, a, b, p0 in parts:
                    for o in of:
                        if ocols[o] > 0:
                            J[(o, w)][:, :, p0:p0 + b - a] = moved(res[o][a:b][:, :, index(idx[o])], (1, 2, 0))
        if "act" in res:
            J["act"] = res["act"]
        J["status"] = res["status"]
        return J

    def alloc(self, k=None):
        """Device arrays (x, y, info) for `solve(out=...)`; y is None for a batch without constraints.  k: the number of
        rows, for a solve of a selection of k instances (None: count)."""
        k = self.count if k is None else int(k)
        if not 1 <= k <= self.count:
            raise ValueError(f"k: expected 1 <= k <= {self.count}, got {k}")
        return (DeviceArray(self.lib, k, self.n, self.device),
                DeviceArray(self.lib, k, self.m, self.device) if self.m else None,
                DeviceArray(self.lib, k, 6, self.device))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.osqp_amd_batch_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pattern_sizes(P, A):
    import scipy.sparse as sp

    P = sp.csc_matrix(sp.triu(P)); P.sort_indices()
    A = sp.csc_matrix(A); A.sort_indices()
    ndiag = int(np.count_nonzero(P.tocoo().row == P.tocoo().col))
    return P, A, A.shape[1], A.shape[0], 2 * P.nnz - ndiag


def shared_plan(lib, P, A):
    """What a shared batch needs for the pattern of P (upper triangle) and A (osqp_amd_shared_batch_plan; host only, no device
    is touched): a dict with `T`, the instances per workgroup -- chosen from the shape alone, never from the number of
    instances --, `lds_bytes` per workgroup, `model_bytes` (scaling, scaled values and the padded inverse, once per handle) and
    `instance_bytes` of device state per instance.  A shape it does not take raises OSQPError with the library's reason."""
    P, A, n, m, nnzF = _pattern_sizes(P, A)
    out = np.zeros(4, dtype=np.int64)
    if lib.osqp_amd_shared_batch_plan(n, m, A.nnz, nnzF, out.ctypes.data) != 0:
        raise OSQPError("Error in batched plan: " + lib.osqp_amd_last_error().decode())
    return {"T": int(out[0]), "lds_bytes": int(out[1]), "model_bytes": int(out[2]), "instance_bytes": int(out[3])}


def shared_launches(lib):
    """Launches of the shared solve kernel by this process so far (osqp_amd_shared_batch_launches): one per `SharedBatch.solve`."""
    return int(lib.osqp_amd_shared_batch_launches())


def shared_adjoint_launches(lib):
    """Accepted `SharedBatch.adjoint` calls of this process so far (osqp_amd_shared_batch_adjoint_launches): one per call, whatever
    the number of cotangents; a refused call does not count."""
    return int(lib.osqp_amd_shared_batch_adjoint_launches())


def shared_jvp_launches(lib):
    """Accepted `SharedBatch.jvp` calls of this process so far (osqp_amd_shared_batch_jvp_launches): one per call, whatever the
    number of directions; a refused call does not count."""
    return int(lib.osqp_amd_shared_batch_jvp_launches())


class SharedBatch:
    """ONE model and `count` right-hand sides on a shared KKT inverse (osqp_amd_shared_batch_setup).
    Instance i is `setup(P, q0, A, l0, u0)`, `update(q=q[i], l=l[i], u=u[i])`, `solve()` on a fresh model: scaling comes from the
    base data, rho is fixed (`adaptive_rho` is set to 0 here unless the caller passes it; anything else is refused by the
    library) and every row of every instance must keep the kind -- loose, equality, inequality -- it has under (l0, u0).
    After setup every instance holds (q0, l0, u0).  Arrays of `update` / `warm_start` and the `out` of `solve` are numpy arrays
    or device arrays (`DeviceArray`, torch tensors), as for `ResidentBatch`.  `adjoint` differentiates the solutions of the last
    `solve()`, per instance and -- for the shared values of P and A -- summed over the instances; `jvp` moves them along
    directions of the data, with ONE tangent of the shared values of P and A for the whole batch; `jacobian` builds Jacobians
    from either.  There is no `rows=`, polish, certificate or duality call here, and the matrices cannot be updated: a new
    model is a new handle."""

    SETTINGS = ("max_iter", "eps_abs", "eps_rel", "eps_prim_inf", "eps_dual_inf", "alpha", "check_termination",
                "scaled_termination", "rho")

    def __init__(self, lib, P, A, q0, l0, u0, count, device=0, **settings):
        P, A, self.n, self.m, _ = _pattern_sizes(P, A)
        if P.shape != (self.n, self.n):
            raise ValueError(f"P: expected shape {(self.n, self.n)}, got {P.shape}")
        self.count = int(count)
        if self.count <= 0:
            raise ValueError("count: the batch is empty")
        q0 = _batch_array("q0", q0, (self.n,))[0]
        l0 = _batch_array("l0", l0, (self.m,))[0]
        u0 = _batch_array("u0", u0, (self.m,))[0]
        settings.setdefault("adaptive_rho", 0)
        stgs = make_settings(lib, settings)
        self.lib, self.device, self.handle = lib, int(device), C.c_void_p()
        Pp, Pi = np.ascontiguousarray(P.indptr, dtype=np.int64), np.ascontiguousarray(P.indices, dtype=np.int64)
        Ap, Ai = np.ascontiguousarray(A.indptr, dtype=np.int64), np.ascontiguousarray(A.indices, dtype=np.int64)
        Px, Ax = _as_f64(P.data), _as_f64(A.data)
        self.nnzP, self.nnzA = P.nnz, A.nnz
        self.Px, self.Ax = Px.copy(), Ax.copy()  # the shared values, in the order of the gradients "Px_sum" / "Ax_sum"
        rc = lib.osqp_amd_shared_batch_setup(C.byref(self.handle), self.count, self.n, self.m, _iptr(Pp), _iptr(Pi), _fptr(Px), _iptr(Ap),
                                             _iptr(Ai), _fptr(Ax), _fptr(q0), _fptr(l0), _fptr(u0), C.byref(stgs), self.device)
        if rc != 0:
            self.handle = C.c_void_p()
            raise OSQPError("Error in shared batch setup: " + lib.osqp_amd_last_error().decode())

    def _call(self, what, rc):
        if rc != 0:
            raise OSQPError(f"Error in shared batch {what}: " + self.lib.osqp_amd_last_error().decode())

    def update(self, q=None, l=None, u=None):
        """New q [count x n] and / or bounds l, u [count x m] (both, in one form).  Bounds with l > u, or that change the kind
        of a row of an instance, raise -- naming the first offending instance and row -- and leave the handle as it was."""
        qa = None if q is None else _batch_array("q", q, (self.count, self.n))
        if (l is None) != (u is None):
            raise ValueError("l and u: a shared batch updates both bounds in one call")
        ba = None
        if l is not None:
            ba = (_batch_array("l", l, (self.count, self.m)), _batch_array("u", u, (self.count, self.m)))
            if ba[0][2] != ba[1][2]:
                raise ValueError("l and u must both be host arrays or both device arrays")
        if qa is not None:
            self._call("update", self.lib.osqp_amd_shared_batch_update_lin_cost(self.handle, qa[1], qa[2]))
        if ba is not None:
            self._call("update", self.lib.osqp_amd_shared_batch_update_bounds(self.handle, ba[0][1], ba[1][1], ba[0][2]))

    def warm_start(self, x=None, y=None):
        """Start the next solve from x [count x n] and / or y [count x m] (caller's units); a missing one is zero."""
        got = [None if v is None else _batch_array(nm, v, (self.count, k)) for nm, v, k in (("x", x, self.n), ("y", y, self.m))]
        forms = {g[2] for g in got if g is not None}
        if len(forms) > 1:
            raise ValueError("x and y must both be host arrays or both device arrays")
        if forms:
            self._call("warm start", self.lib.osqp_amd_shared_batch_warm_start(self.handle, None if got[0] is None else got[0][1],
                                                                               None if got[1] is None else got[1][1], forms.pop()))

    def solve(self, out=None):
        """Solve every instance in one launch -> (x [count x n], y [count x m], info [count x 6]: iter, status_val, pri_res,
        dua_res, obj_val, 0).  out=None: numpy arrays; out=(x, y, info) of device arrays: written in place and returned."""
        k = self.count
        if out is None:
            x, y, info = np.empty((k, self.n)), np.empty((k, self.m)), np.empty((k, 6))
            self._call("solve", self.lib.osqp_amd_shared_batch_resolve(self.handle, x.ctypes.data, y.ctypes.data, info.ctypes.data, 0))
            return x, y, info
        if len(out) != 3:
            raise ValueError("out: expected (x, y, info)")
        ptrs = []
        for name, a, cols in (("out[0]", out[0], self.n), ("out[1]", out[1], self.m), ("out[2]", out[2], 6)):
            if a is None and cols == 0:
                ptrs.append(None)
                continue
            if not hasattr(a, "data_ptr"):
                raise ValueError(f"{name}: expected a device array (DeviceArray, torch tensor); omit `out` for numpy results")
            ptrs.append(_batch_array(name, a, (k, cols))[1])
        self._call("solve", self.lib.osqp_amd_shared_batch_resolve(self.handle, ptrs[0], ptrs[1], ptrs[2], 1))
        return out

    def update_settings(self, **kw):
        """New values for settings of the following solves (osqp_amd_shared_batch_update_setting): the names of `SETTINGS`.
        `rho` re-factorises the shared matrix once; the carried iterates stay.  Any other name raises, here or in the library."""
        for key, value in kw.items():
            if value is None:
                continue
            self._call("settings update", self.lib.osqp_amd_shared_batch_update_setting(self.handle, key.encode(), float(value)))

    ADJOINT_WANT = ("q", "l", "u", "Px", "Ax")
    ADJOINT_SUMS = ("Px", "Ax")

    def adjoint(self, dx=None, dy=None, want=ADJOINT_WANT, sums=(), out=None):
        """Gradients of a scalar loss with respect to the data, through the solutions of the last `solve()`
        (osqp_amd_shared_batch_adjoint): dx [count x n], dy [count x m] are the loss's gradients with respect to x and y (None:
        zero; not both), or both with a leading axis [ncot x count x .] for several cotangents in one call.  Returns a dict with
        the entries of `want` -- "q", "l", "u", "Px", "Ax", per instance, shaped like the cotangents -- the entries of `sums`
        (a subset of ("Px", "Ax")) under "Px_sum" [nnz(P upper)] and "Ax_sum" [nnz(A)] ([ncot x .] with a leading axis): the
        gradients of the SHARED values, summed over the instances on the device in blocks of 16 (include/osqp_amd.h has the
        order; the bits do not depend on `want`) -- plus "act" [count x m] and "status" [count] (1 differentiated, 0 no
        solution, -1 factorisation failed; such rows are zeros).  Entries of width 0 are left out.  Host form: numpy dx / dy,
        out=None, numpy results.  Device form: dx / dy device arrays and `out` a dict of float64 device arrays for the wanted
        entries (the sums as [1 x cols] or [cols] without a leading axis) and, optionally, "act" and "status" ([count x 1]).  The handle
        must hold the solutions of its current data: a `solve()` since the last `update`, `warm_start` or rho update."""
        cnt = self.count
        cols = dict(q=self.n, l=self.m, u=self.m, Px=self.nnzP, Ax=self.nnzA, Px_sum=self.nnzP, Ax_sum=self.nnzA, act=self.m, status=1)
        want, sums = tuple(want), tuple(sums)
        for w in want:
            if w not in self.ADJOINT_WANT:
                raise ValueError(f"want: unknown gradient {w!r}; expected a subset of {self.ADJOINT_WANT}")
        for w in sums:
            if w not in self.ADJOINT_SUMS:
                raise ValueError(f"sums: unknown sum {w!r}; expected a subset of {self.ADJOINT_SUMS}")
        if dx is None and dy is None:
            raise ValueError("dx and dy: at least one incoming gradient is needed")
        shapes = {k: tuple(v.shape) if hasattr(v, "data_ptr") else np.asarray(v).shape for k, v in (("dx", dx), ("dy", dy)) if v is not None}
        dims = {k: len(s) for k, s in shapes.items()}
        if len(set(dims.values())) > 1 or next(iter(dims.values())) not in (2, 3):
            raise ValueError(f"dx and dy: expected both [count x cols] or both [ncot x count x cols], got dimensions {dims}")
        many = next(iter(dims.values())) == 3
        ncot = 1
        if many:
            ncots = {k: int(s[0]) for k, s in shapes.items()}
            if len(set(ncots.values())) > 1:
                raise ValueError(f"dx and dy: they must carry the same number of cotangents, got {ncots}")
            ncot = next(iter(ncots.values()))
            if ncot < 1:
                raise ValueError("dx and dy: ncot must be at least 1")
        lead = (ncot, cnt) if many else (cnt,)
        got = [None if v is None else _batch_array(nm, v, lead + (k,)) for nm, v, k in (("dx", dx, self.n), ("dy", dy, self.m))]
        forms = {g[2] for g in got if g is not None}
        if len(forms) > 1:
            raise ValueError("dx and dy must both be host arrays or both device arrays")
        ptrs, where = [None if g is None else g[1] for g in got], forms.pop()
        wanted = want + tuple(w + "_sum" for w in sums)
        oshape = {k: (cnt, cols[k]) if k in ("act", "status") else
                  ((ncot if many else 1, cols[k]) if k.endswith("_sum") else lead + (cols[k],)) for k in cols}
        order = self.ADJOINT_WANT + ("Px_sum", "Ax_sum", "act", "status")
        names = [k for k in order if cols[k] > 0]
        if not where:
            if out is not None:
                raise ValueError("out: host gradients (numpy dx / dy) return numpy arrays; pass device arrays for dx / dy to fill `out`")
            res = {k: np.empty(oshape[k]) for k in names if k in wanted or k in ("act", "status")}
            addr = {k: v.ctypes.data for k, v in res.items()}
        else:
            if not isinstance(out, dict):
                raise ValueError("out: device gradients need a dict of device arrays to fill, one per entry of `want` and `sums`")
            for k in out:
                if k not in cols:
                    raise ValueError(f"out: unknown entry {k!r}")
            addr = {}
            for k in names:
                if k in out and (k in wanted or k in ("act", "status")):
                    if not hasattr(out[k], "data_ptr"):
                        raise ValueError(f"out[{k!r}]: expected a device array (DeviceArray, torch tensor)")
                    flat = k.endswith("_sum") and not many and len(tuple(out[k].shape)) == 1  # a torch vector [cols]
                    addr[k] = _batch_array(f"out[{k!r}]", out[k], (cols[k],) if flat else oshape[k])[1]
                elif k in wanted:
                    raise ValueError(f"out: no array for the wanted gradient {k!r}")
            res = out
        self._call("adjoint", self.lib.osqp_amd_shared_batch_adjoint(self.handle, ncot, ptrs[0], ptrs[1], *[addr.get(k) for k in order], where))
        if not where:
            for k in ("Px_sum", "Ax_sum"):
                if k in res and not many:
                    res[k] = res[k][0]
            if "act" in res:
                res["act"] = res["act"].astype(np.int64)
            res["status"] = res["status"].ravel().astype(np.int64)
        return res

    JVP_TANGENTS = ("q", "l", "u", "Px", "Ax")
    JVP_SHARED = ("Px", "Ax")

    def jvp(self, q=None, l=None, u=None, Px=None, Ax=None, out=None):
        """Forward sensitivities of the solutions of the last `solve()` along directions of the data (osqp_amd_shared_batch_jvp,
        DESIGN.md section 13.5).  The tangents q [count x n], l, u [count x m] are PER INSTANCE; Px [nnz(P upper)] and Ax [nnz(A)]
        are ONE tangent of the SHARED values for the whole batch, in the index spaces of "Px_sum" / "Ax_sum" (None: zero; not
        all).  Or all of them with a leading axis, [ndir x count x .] and [ndir x nnz], for several directions in one call: one
        factorisation per instance, one solve per direction, and direction d has the bits of a call with that direction alone.
        Mixed ranks raise.  Returns a dict: "x" (tangent of the solutions) and "y" (of the multipliers; zero on inactive rows),
        [count x .] or [ndir x count x .], "act" [count x m] (-1 lower, 1 upper, 0 inactive) and "status" (1 differentiated, 0 no
        solution, -1 factorisation failed; such rows are zeros), as `adjoint` returns them.  Entries of width 0 are left out,
        and a tangent of width 0 is ignored.  On a row with l == u only the tangent `l` is read.  Host form: numpy tangents,
        out=None, numpy results.  Device form: device arrays and `out` a dict of float64 device arrays -- "x" and / or "y",
        optionally "act" [count x m] and "status" [count x 1] -- filled in place and returned.  The handle must hold the
        solutions of its current data, as for `adjoint`."""
        cnt = self.count
        cols = dict(q=self.n, l=self.m, u=self.m, Px=self.nnzP, Ax=self.nnzA)
        given = {k: v for k, v in zip(self.JVP_TANGENTS, (q, l, u, Px, Ax)) if v is not None}
        if not given:
            raise ValueError("q, l, u, Px, Ax: at least one tangent is needed")
        shapes = {k: tuple(v.shape) if hasattr(v, "data_ptr") else np.asarray(v).shape for k, v in given.items()}
        # the rank of a direction-less call: 2 for the per-instance tangents, 1 for the shared ones
        extra = {k: len(s) - (1 if k in self.JVP_SHARED else 2) for k, s in shapes.items()}
        if len(set(extra.values())) > 1 or next(iter(extra.values())) not in (0, 1):
            raise ValueError("tangents: expected q, l, u [count x cols] with Px, Ax [nnz], or all with a leading axis [ndir x ...], got shapes "
                             f"{shapes}")
        many = next(iter(extra.values())) == 1
        ndir = 1
        if many:
            ndirs = {k: int(s[0]) for k, s in shapes.items()}
            if len(set(ndirs.values())) > 1:
                raise ValueError(f"tangents: they must carry the same number of directions, got {ndirs}")
            ndir = next(iter(ndirs.values()))
            if ndir < 1:
                raise ValueError("tangents: ndir must be at least 1")
        lead = (ndir,) if many else ()
        got = {k: _batch_array(k, v, lead + (() if k in self.JVP_SHARED else (cnt,)) + (cols[k],)) for k, v in given.items()}
        forms = {g[2] for g in got.values()}
        if len(forms) > 1:
            raise ValueError("tangents: they must all be host arrays or all device arrays")
        where = forms.pop()
        got = {k: g for k, g in got.items() if cols[k] > 0}
        if not got:
            raise ValueError("q, l, u, Px, Ax: every tangent given has width 0")
        ocols = dict(x=self.n, y=self.m, act=self.m, status=1)
        oshape = dict(x=lead + (cnt, self.n), y=lead + (cnt, self.m), act=(cnt, self.m), status=(cnt, 1))
        names = [k for k in ("x", "y", "act", "status") if ocols[k] > 0]
        if not where:
            if out is not None:
                raise ValueError("out: host tangents (numpy) return numpy arrays; pass device arrays for the tangents to fill `out`")
            res = {k: np.empty(oshape[k]) for k in names}
            addr = {k: v.ctypes.data for k, v in res.items()}
        else:
            if not isinstance(out, dict):
                raise ValueError("out: device tangents need a dict of device arrays to fill: x, y")
            for k in out:
                if k not in ocols:
                    raise ValueError(f"out: unknown entry {k!r}")
            addr = {}
            for k in names:
                if k in out:
                    if not hasattr(out[k], "data_ptr"):
                        raise ValueError(f"out[{k!r}]: expected a device array (DeviceArray, torch tensor)")
                    addr[k] = _batch_array(f"out[{k!r}]", out[k], oshape[k])[1]
            if "x" not in addr and "y" not in addr:
                raise ValueError("out: no array for 'x' or 'y'")
            res = out
        tail = [got[k][1] if k in got else None for k in self.JVP_TANGENTS]
        tail += [addr.get("x"), addr.get("y"), addr.get("act"), addr.get("status"), where]
        self._call("jvp", self.lib.osqp_amd_shared_batch_jvp(self.handle, ndir, *tail))
        if not where:
            if "act" in res:
                res["act"] = res["act"].astype(np.int64)
            res["status"] = res["status"].ravel().astype(np.int64)
        return res

    JACOBIAN_OF = ("x", "y")
    JACOBIAN_BUDGET = 256 << 20  # bytes: the unit vectors and the largest output of one call of `jacobian` (default chunk)

    def jacobian(self, of=("x",), wrt=("q",), mode="auto", chunk=None):
        """Jacobians of the solutions of the last `solve()` with respect to the data: a dict {(o, w): array} for o in `of` (a
        subset of "x", "y") and w in `wrt` (a subset of "q", "l", "u", "Px", "Ax"), plus "act" and "status" as `adjoint` / `jvp`
        return them (an instance with status != 1 has zeros).  w in q, l, u: [count x cols(o) x cols(w)], entry [i, a, b] the
        derivative of component a of o of instance i with respect to entry b of ITS OWN w.  w in Px, Ax: [count x cols(o) x nnz],
        the derivative with respect to entry b of the SHARED values.  mode="forward": unit directions through `jvp`, one solve
        per column of the `wrt` arrays -- one unit direction is applied to every instance at once; mode="reverse": unit
        cotangents through `adjoint` with the per-instance rows, one solve per output component; "auto": the one with fewer
        solves per instance (reverse on a tie).  chunk: the most directions / cotangents per call; the chunks are independent
        calls whose results are concatenated.  Default: as many as keep the unit vectors and the largest output of one call
        under 256 MiB together, at least 1.  Host arrays only.  Nothing is computed on the results: they are transposed and
        placed."""
        of, wrt = tuple(of), tuple(wrt)
        cnt = self.count
        wcols = dict(q=self.n, l=self.m, u=self.m, Px=self.nnzP, Ax=self.nnzA)
        ocols = dict(x=self.n, y=self.m)
        if not of or len(set(of)) != len(of) or any(o not in self.JACOBIAN_OF for o in of):
            raise ValueError(f"of: expected a non-empty subset of {self.JACOBIAN_OF} without repeats, got {of!r}")
        if not wrt or len(set(wrt)) != len(wrt) or any(w not in self.ADJOINT_WANT for w in wrt):
            raise ValueError(f"wrt: expected a non-empty subset of {self.ADJOINT_WANT} without repeats, got {wrt!r}")
        if mode not in ("auto", "reverse", "forward"):
            raise ValueError(f"mode: expected 'auto', 'reverse' or 'forward', got {mode!r}")
        n_rev, n_fwd = sum(ocols[o] for o in of), sum(wcols[w] for w in wrt)
        if n_rev == 0 or n_fwd == 0:
            raise ValueError("jacobian: no output component or no data column is asked for")
        if mode == "auto":
            mode = "reverse" if n_rev <= n_fwd else "forward"
        total = n_rev if mode == "reverse" else n_fwd
        if chunk is not None and (not isinstance(chunk, (int, np.integer)) or isinstance(chunk, bool) or chunk < 1):
            raise ValueError(f"chunk: expected a positive integer, got {chunk!r}")
        reverse = mode == "reverse"
        if chunk is None:
            unit = sum(ocols[o] for o in of) if reverse else sum(wcols[w] for w in wrt if w not in self.JVP_SHARED)
            largest = max(wcols[w] for w in wrt) if reverse else max(ocols[o] for o in of)
            chunk = max(1, self.JACOBIAN_BUDGET // (8 * cnt * (unit + largest)))
        chunk = int(min(chunk, total))
        # the solves of the call in order: segment (name, first solve, number) -- the components of each o (reverse), the
        # columns of each w (forward)
        segs, at = [], 0
        for name, width in ([(o, ocols[o]) for o in of] if reverse else [(w, wcols[w]) for w in wrt]):
            segs.append((name, at, width))
            at += width
        J = {(o, w): np.zeros((cnt, ocols[o], wcols[w])) for o in of for w in wrt}
        res = {}
        for c0 in range(0, total, chunk):
            c1 = min(c0 + chunk, total)
            nc = c1 - c0
            # the part [a, b) of each segment that falls into this chunk, as positions of the chunk and of the segment
            parts = [(name, max(s0, c0) - c0, min(s0 + w, c1) - c0, max(s0, c0) - s0) for name, s0, w in segs if max(s0, c0) < min(s0 + w, c1)]
            if reverse:
                cot = {o: np.zeros((nc, cnt, ocols[o])) for o in of if ocols[o] > 0}
                for o, a, b, p0 in parts:
                    cot[o][np.arange(a, b), :, np.arange(p0, p0 + b - a)] = 1.0
                want = tuple(w for w in wrt if wcols[w] > 0)
                res = self.adjoint(dx=cot.get("x"), dy=cot.get("y"), want=want)
                for o, a, b, p0 in parts:
                    for w in want:
                        J[(o, w)][:, p0:p0 + b - a, :] = np.transpose(res[w][a:b], (1, 0, 2))
            else:
                tan = {w: np.zeros((nc, wcols[w]) if w in self.JVP_SHARED else (nc, cnt, wcols[w])) for w in wrt if wcols[w] > 0}
                for w, a, b, p0 in parts:
                    if w in self.JVP_SHARED:
                        tan[w][np.arange(a, b), np.arange(p0, p0 + b - a)] = 1.0
                    else:
                        tan[w][np.arange(a, b), :, np.arange(p0, p0 + b - a)] = 1.0
                res = self.jvp(**tan)
                for w, a, b, p0 in parts:
                    for o in of:
                        if ocols[o] > 0:
                            J[(o, w)][:, :, p0:p0 + b - a] = np.transpose(res[o][a:b], (1, 2, 0))
        if "act" in res:
            J["act"] = res["act"]
        J["status"] = res["status"]
        return J

    def device_bytes(self):
        return int(self.lib.osqp_amd_shared_batch_device_bytes(self.handle))

    def alloc(self):
        """Device arrays (x, y, info) for `solve(out=...)`; y is None for a batch without constraints."""
        return (DeviceArray(self.lib, self.count, self.n, self.device),
                DeviceArray(self.lib, self.count, self.m, self.device) if self.m else None,
                DeviceArray(self.lib, self.count, 6, self.device))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.osqp_amd_shared_batch_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def status_names(info):
    return [status_map[int(v)] for v in info[:, 1]]
