"""A resident batch as a differentiable torch layer: `BatchQPFunction` solves `count` QPs in its forward
(`ResidentBatch.update` + `solve`, device pointers, no host hop) and differentiates their solutions in its backward
(`ResidentBatch.adjoint`: one launch of k_batch_adjoint, also for a BATCH of cotangents -- below); under forward-mode differentiation (`torch.autograd.forward_ad`,
`torch.func.jvp`) its `jvp` pushes the tangents of the inputs forward to the solutions (`ResidentBatch.jvp`: one launch of
k_batch_jvp).  torch is plumbing only: tensors are passed to the library by address and nothing is computed in torch.

    rb = batch.ResidentBatch(lib, P, A, Px, Ax, q, l, u, polish=True)
    layer = BatchQPLayer(rb)
    x, y = layer(q=q_t, l=l_t, u=u_t)          # float64 CUDA tensors [count x .]; None keeps the handle's data
    loss(x, y).backward()                       # q_t.grad, l_t.grad, u_t.grad
    with forward_ad.dual_level():               # forward mode: the tangents of x, y along a tangent of q
        x, y = layer(q=forward_ad.make_dual(q_t, tq_t))
        tx = forward_ad.unpack_dual(x).tangent

    x, y = layer(q=q_t[sel], rows=sel)         # a selection (`batch.selection`): tensors [k x .], the others untouched

    xs, vjp_fn = torch.func.vjp(lambda q: layer(q=q)[0], q_t)
    (dq,) = torch.func.vmap(vjp_fn)(G)          # G [ncot x count x n]: ONE adjoint launch for all cotangents
    J = torch.func.jacrev(lambda q: layer(q=q)[0])(q_t)   # [count x n x count x n], one launch as well
    J = layer.jacobian(of=("x",), wrt=("q",))   # the per-instance blocks [count x n x n] (`ResidentBatch.jacobian`)

Batched reverse mode: `BatchQPFunction` is a new-style Function (`forward` without ctx, `setup_context`) whose backward calls
a second Function, `BatchQPAdjoint`; its `vmap` rule moves the batch axis of the cotangents to the front (a cotangent that
arrives unbatched -- `jacrev` of x alone hands over gy as unbatched zeros -- is expanded) and calls `ResidentBatch.adjoint`
with [ncot x k x .] arrays: one factorisation per instance, one solve per cotangent.  Out of scope: `torch.autograd.grad(...,
is_grads_batched=True)`, which uses torch's legacy vmap -- that ignores the `vmap` rule and hands the backward batched
tensors without addresses; and `torch.func.jacfwd`, that is `vmap` over the forward-mode rule.

Three rules.  The library runs on its own stream and blocks, so torch's current stream is synchronised before every library
call.  The handle holds ONE solution per instance: every forward stamps the instances it served (all of them without
`rows`), and a backward raises RuntimeError when one of ITS instances has been served by a later forward -- two forwards on
disjoint selections can both run their backward (the forward-mode rule runs with its forward and needs no stamp).  Instances whose adjoint status is not 1 (no solution, failed factorisation) get zero gradients; where
an instance's active constraints are dependent the derivative does not exist and the regularised answer is returned
(include/osqp_amd.h, osqp_amd_batch_adjoint); the same holds for the tangents (osqp_amd_batch_jvp).

A shared batch (`batch.SharedBatch`: ONE model, many right-hand sides) as a layer: `SharedBatchQPFunction` /
`SharedBatchQPLayer(sb)`, after the two classes above.  q, l, u [count x .] update the handle and get per-instance gradients;
Px [nnzP] and Ax [nnzA] are the shared values -- they must be the handle's own and get the gradients SUMMED over the instances
(`SharedBatch.adjoint(sums=...)`: one launch of k_shared_adjoint plus the fixed-order reduction, no host hop).

    sb = batch.SharedBatch(lib, P, A, q0, l0, u0, count)
    layer = SharedBatchQPLayer(sb)
    Px = torch.nn.Parameter(layer.Px.clone())
    x, y = layer(q=q_t, l=l_t, u=u_t, Px=Px)    # Px.grad [nnzP]: the sum over the instances

A single model (`interface.Model`: one large sparse QP, any n) as a layer: `QPFunction` / `QPLayer(model)`, at the end of this
file.  The forward is `update` + `solve`, the backward one `interface.adjoint` call on the kept factor, and under
`torch.autograd.forward_ad` the tangents of (x, y) come from one `interface.jvp` call on the same factor.  Two routes, by
where the tensors live.  CUDA tensors (all of them, on the model's device) take the device-pointer forms of the library
(include/osqp_amd.h: osqp_amd_update_vectors_dev ... osqp_amd_jvp_dev): the data are read from HBM, x, y and the gradients
are torch-allocated CUDA tensors the library writes into, nothing goes through the host; torch's current stream is
synchronised before every library call, as for the batch.  CPU tensors take the host forms.  The two routes give the same
bits (the device forms are the host forms with the copy removed); a mixture of CPU and CUDA tensors raises ValueError.

    layer = QPLayer(model)
    x, y = layer(q=q_t, l=l_t, u=u_t)           # float64 tensors [n] / [m]; None keeps the model's data
    loss(x, y).backward()                        # q_t.grad, l_t.grad, u_t.grad through osqp_amd_adjoint"""
import numpy as np
import torch

from . import interface as _iface
from .batch import selection

NAMES = ("q", "l", "u", "Px", "Ax")


def _sync(t):
    torch.cuda.current_stream(t.device).synchronize()


def stamp_forward(rb, sel):
    """A forward has served the instances `sel` of `rb` (None: all of them): they carry its stamp, which is returned."""
    stamps = getattr(rb, "_qp_layer_stamps", None)
    if stamps is None:
        stamps = rb._qp_layer_stamps = np.zeros(rb.count, dtype=np.int64)
    rb._qp_layer_stamp = getattr(rb, "_qp_layer_stamp", 0) + 1
    stamps[slice(None) if sel is None else sel] = rb._qp_layer_stamp
    return rb._qp_layer_stamp


def stamp_holds(rb, stamp, sel):
    """Do the instances `sel` of `rb` (None: all of them) still hold the solution of the forward that got `stamp`?"""
    stamps = getattr(rb, "_qp_layer_stamps", None)
    return stamps is not None and bool(np.all(stamps[slice(None) if sel is None else sel] == stamp))


def _check_inputs(given):
    for name, t in given.items():
        if t is not None and (not t.is_cuda or t.dtype != torch.float64):
            raise ValueError(f"{name}: expected a float64 CUDA tensor")


class BatchQPAdjoint(torch.autograd.Function):
    """The pull-back of `BatchQPFunction` as a Function of its own, so that it can carry a `vmap` rule: (gx, gy) -> the
    gradients `want` of the instances `sel` of `rb`, through `ResidentBatch.adjoint`.  Under `torch.func.vmap` the cotangents
    arrive with a batch axis and go to the library as ONE launch with a leading axis [ncot x k x .]."""

    @staticmethod
    def forward(rb, sel, stamp, want, gx, gy):
        return BatchQPAdjoint._pull(rb, sel, stamp, want, gx, gy, ())

    @staticmethod
    def setup_context(ctx, inputs, output):
        pass

    @staticmethod
    def backward(ctx, *grads):
        raise RuntimeError("BatchQPAdjoint: the adjoint of the batch is not differentiable a second time")

    @staticmethod
    def vmap(info, in_dims, rb, sel, stamp, want, gx, gy):
        ncot = info.batch_size

        def front(g, dim):  # the batch axis to the front; a cotangent that arrives unbatched is the same for every one
            if g is None:
                return None
            return g.unsqueeze(0).expand((ncot,) + tuple(g.shape)) if dim is None else g.movedim(dim, 0)

        out = BatchQPAdjoint._pull(rb, sel, stamp, want, front(gx, in_dims[4]), front(gy, in_dims[5]), (ncot,))
        return out, tuple(0 for _ in out)

    @staticmethod
    def _pull(rb, sel, stamp, want, gx, gy, lead):
        if not stamp_holds(rb, stamp, sel):
            raise RuntimeError("BatchQPFunction: the batch has been solved again since this forward; its handle holds one "
                               "solution, so backward must run before the next forward")
        k = rb.count if sel is None else len(sel)
        cols = dict(q=rb.n, l=rb.m, u=rb.m, Px=rb.nnzP, Ax=rb.nnzA)
        ref = gx if gx is not None else gy
        out = {w: torch.empty(lead + (k, cols[w]), dtype=torch.float64, device=ref.device) for w in want}
        _sync(ref)
        rb.adjoint(dx=None if gx is None else gx.contiguous(), dy=None if gy is None or rb.m == 0 else gy.contiguous(), want=want, out=out,
                   rows=sel)
        return tuple(out[w] for w in want)


class BatchQPFunction(torch.autograd.Function):
    @staticmethod
    def forward(rb, q, l, u, Px, Ax, rows=None):
        given = dict(zip(NAMES, (q, l, u, Px, Ax)))
        tensors = [t for t in given.values() if t is not None]
        if not tensors:
            raise ValueError("BatchQPFunction: at least one of q, l, u, Px, Ax must be a tensor")
        _check_inputs(given)
        sel = None if rows is None else selection(rows.cpu().numpy() if torch.is_tensor(rows) else rows, rb.count)
        k = rb.count if sel is None else len(sel)
        ref = tensors[0]
        _sync(ref)
        rb.update(**{name: t.detach().contiguous() for name, t in given.items() if t is not None}, rows=sel)
        x = torch.empty((k, rb.n), dtype=torch.float64, device=ref.device)
        y = torch.empty((k, rb.m), dtype=torch.float64, device=ref.device)
        info = torch.empty((k, 6), dtype=torch.float64, device=ref.device)
        rb.solve(out=(x, y if rb.m else None, info), rows=sel)
        rb._qp_layer_info = info
        rb._qp_layer_served = (sel, k, stamp_forward(rb, sel))  # for setup_context, which runs next
        return x, y

    @staticmethod
    def setup_context(ctx, inputs, output):
        rb = inputs[0]
        ctx.rb = rb
        ctx.sel, ctx.k, ctx.stamp = rb._qp_layer_served
        ctx.given = tuple(name for name, t in zip(NAMES, inputs[1:6]) if t is not None)  # for jvp: the inputs that have a tangent

    @staticmethod
    def jvp(ctx, t_rb, tq, tl, tu, tPx, tAx, *t_rows):
        """Forward mode: the tangents of (x, y) along the tangents of the tensor inputs (an input without a tangent arrives
        as zeros, a None input as None)."""
        rb = ctx.rb
        cols = dict(q=rb.n, l=rb.m, u=rb.m, Px=rb.nnzP, Ax=rb.nnzA)
        tang = {k: t.contiguous() for k, t in zip(NAMES, (tq, tl, tu, tPx, tAx)) if k in ctx.given and t is not None and cols[k] > 0}
        ref = next(iter(tang.values()))
        tx = torch.empty((ctx.k, rb.n), dtype=torch.float64, device=ref.device)
        ty = torch.empty((ctx.k, rb.m), dtype=torch.float64, device=ref.device)
        _sync(ref)
        rb.jvp(**tang, out=dict(x=tx, y=ty) if rb.m else dict(x=tx), rows=ctx.sel)
        return tx, ty

    @staticmethod
    def backward(ctx, gx, gy):
        rb = ctx.rb
        if not stamp_holds(rb, ctx.stamp, ctx.sel):
            raise RuntimeError("BatchQPFunction: the batch has been solved again since this forward; its handle holds one "
                               "solution, so backward must run before the next forward")
        nargs = len(ctx.needs_input_grad)  # 6, or 7 with rows
        need = dict(zip(NAMES, ctx.needs_input_grad[1:6]))
        cols = dict(q=rb.n, l=rb.m, u=rb.m, Px=rb.nnzP, Ax=rb.nnzA)
        want = tuple(k for k in NAMES if need[k] and cols[k] > 0)
        if gx is None and gy is None:
            return (None,) * nargs
        ref = gx if gx is not None else gy
        out = dict(zip(want, BatchQPAdjoint.apply(rb, ctx.sel, ctx.stamp, want, gx, gy))) if want else {}
        # a wanted gradient of width zero: zeros shaped like the others (`ref` carries the batch axis of a vmapped pull-back)
        grads = {k: (out[k] if k in out else (ref.new_zeros((ctx.k, 0)) if need[k] else None)) for k in NAMES}
        return (None,) + tuple(grads[k] for k in NAMES) + (None,) * (nargs - 6)


class BatchQPLayer(torch.nn.Module):
    """`layer(q=None, l=None, u=None, Px=None, Ax=None, rows=None) -> (x, y)` on the resident batch `rb`; `layer.info` is the
    info array [count x 6] of the last forward.  rows: a selection of the instances (`batch.selection`); the tensors, x, y
    and `layer.info` are then [k x .], row j for instance rows[j], and every other instance is left as it was.
    duality_gap_check=True calls `rb.duality_gap_check()` once here: every forward then also needs the duality gap below its
    bound before an instance ends Solved, and the backward differentiates at that point.
    large=True states that `rb` was built with `ResidentBatch(..., large=True)` for 128 < n <= 256 (it is also set when rb.n >
    128): by default such a layer is forward only -- the adjoint and JVP kernels keep M in LDS, and `backward` / `jacobian`
    raise the library's refusal ("instance too large to polish ...").  large_factor=True calls `rb.large_factor()` once here:
    backward and forward mode then run the forms of those kernels that keep the factor in global scratch (DESIGN.md section
    13.2)."""

    def __init__(self, rb, duality_gap_check=False, large=False, large_factor=False):
        super().__init__()
        self.rb, self.info = rb, None
        self.large = bool(large) or rb.n > 128
        if large_factor:
            rb.large_factor(True)
        if duality_gap_check:
            rb.duality_gap_check(True)

    def forward(self, q=None, l=None, u=None, Px=None, Ax=None, rows=None):
        if rows is None:
            x, y = BatchQPFunction.apply(self.rb, q, l, u, Px, Ax)
        else:
            x, y = BatchQPFunction.apply(self.rb, q, l, u, Px, Ax, rows)
        self.info, self._served = self.rb._qp_layer_info, self.rb._qp_layer_served
        return x, y

    def jacobian(self, of=("x",), wrt=("q", "l", "u"), mode="auto", out_rows=None, chunk=None):
        """`ResidentBatch.jacobian` of the instances of the last forward, as tensors on the handle's device: a dict
        {(o, w): [k x cols(o) x cols(w)]} plus "act" and "status".  Raises RuntimeError when one of these instances has been
        served by a later forward on the same handle (the stamp rule)."""
        served = getattr(self, "_served", None)
        if served is None:
            raise RuntimeError("BatchQPLayer.jacobian: no forward has run yet")
        sel, _, stamp = served
        if not stamp_holds(self.rb, stamp, sel):
            raise RuntimeError("BatchQPLayer.jacobian: the batch has been solved again since the last forward of this layer")
        return self.rb.jacobian(of=of, wrt=wrt, mode=mode, rows=sel, out_rows=out_rows, chunk=chunk, device=True)


def shared_values(sb, device):
    """The values of P (upper triangle) and A of the shared batch `sb` as tensors on `device`, uploaded once per handle: what
    a Px / Ax input of `SharedBatchQPFunction` is compared with."""
    own = getattr(sb, "_qp_layer_values", None)
    if own is None or own["Px"].device != device:
        own = sb._qp_layer_values = dict(Px=torch.tensor(sb.Px, device=device), Ax=torch.tensor(sb.Ax, device=device))
    return own


class SharedBatchQPAdjoint(torch.autograd.Function):
    """The pull-back of `SharedBatchQPFunction` as a Function of its own with a `vmap` rule, after `BatchQPAdjoint`: (gx, gy) ->
    the gradients `want` (per instance) and `sums` (of the shared values) through ONE `SharedBatch.adjoint` call; under
    `torch.func.vmap` the cotangents go to the library with a leading axis [ncot x count x .]."""

    @staticmethod
    def forward(sb, stamp, want, sums, gx, gy):
        return SharedBatchQPAdjoint._pull(sb, stamp, want, sums, gx, gy, ())

    @staticmethod
    def setup_context(ctx, inputs, output):
        pass

    @staticmethod
    def backward(ctx, *grads):
        raise RuntimeError("SharedBatchQPAdjoint: the adjoint of the batch is not differentiable a second time")

    @staticmethod
    def vmap(info, in_dims, sb, stamp, want, sums, gx, gy):
        ncot = info.batch_size

        def front(g, dim):  # the batch axis to the front; a cotangent that arrives unbatched is the same for every one
            if g is None:
                return None
            return g.unsqueeze(0).expand((ncot,) + tuple(g.shape)) if dim is None else g.movedim(dim, 0)

        out = SharedBatchQPAdjoint._pull(sb, stamp, want, sums, front(gx, in_dims[4]), front(gy, in_dims[5]), (ncot,))
        return out, tuple(0 for _ in out)

    @staticmethod
    def _pull(sb, stamp, want, sums, gx, gy, lead):
        if not stamp_holds(sb, stamp, None):
            raise RuntimeError("SharedBatchQPFunction: the batch has been solved again since this forward; its handle holds one "
                               "solution, so backward must run before the next forward")
        cols = dict(q=sb.n, l=sb.m, u=sb.m, Px=sb.nnzP, Ax=sb.nnzA)
        ref = gx if gx is not None else gy
        out = {w: torch.empty(lead + (sb.count, cols[w]), dtype=torch.float64, device=ref.device) for w in want}
        out.update({w + "_sum": torch.empty(lead + (cols[w],), dtype=torch.float64, device=ref.device) for w in sums})
        _sync(ref)
        sb.adjoint(dx=None if gx is None else gx.contiguous(), dy=None if gy is None or sb.m == 0 else gy.contiguous(), want=want, sums=sums,
                   out=out)
        return tuple(out[w] for w in want) + tuple(out[w + "_sum"] for w in sums)


class SharedBatchQPFunction(torch.autograd.Function):
    """(x, y) of every instance of a shared batch as a function of q, l, u [count x .] -- which update the handle and receive
    per-instance gradients -- and of the SHARED values Px [nnzP], Ax [nnzA], which must be the handle's own (they are not
    updated: a new model is a new handle) and receive the gradients summed over the instances."""

    @staticmethod
    def forward(sb, q, l, u, Px, Ax):
        given = dict(zip(NAMES, (q, l, u, Px, Ax)))
        tensors = [t for t in given.values() if t is not None]
        if not tensors:
            raise ValueError("SharedBatchQPFunction: at least one of q, l, u, Px, Ax must be a tensor")
        _check_inputs(given)
        if (l is None) != (u is None):
            raise ValueError("l and u: a shared batch updates both bounds in one call")
        ref = tensors[0]
        for name in ("Px", "Ax"):  # compared on the device: no host hop
            t, own = given[name], shared_values(sb, ref.device)[name]
            if t is not None and (tuple(t.shape) != tuple(own.shape) or not torch.equal(t.detach(), own)):
                raise ValueError(f"{name}: the values differ from those of the handle; a shared batch cannot update its matrices "
                                 "(a new model is a new handle)")
        _sync(ref)
        sb.update(**{name: given[name].detach().contiguous() for name in ("q", "l", "u") if given[name] is not None})
        x = torch.empty((sb.count, sb.n), dtype=torch.float64, device=ref.device)
        y = torch.empty((sb.count, sb.m), dtype=torch.float64, device=ref.device)
        info = torch.empty((sb.count, 6), dtype=torch.float64, device=ref.device)
        sb.solve(out=(x, y if sb.m else None, info))
        sb._qp_layer_info = info
        sb._qp_layer_served = stamp_forward(sb, None)  # for setup_context, which runs next
        return x, y

    @staticmethod
    def setup_context(ctx, inputs, output):
        ctx.sb = inputs[0]
        ctx.stamp = ctx.sb._qp_layer_served
        ctx.given = tuple(name for name, t in zip(NAMES, inputs[1:6]) if t is not None)  # for jvp: the inputs that have a tangent

    @staticmethod
    def jvp(ctx, t_sb, tq, tl, tu, tPx, tAx):
        """Forward mode: the tangents of (x, y) of every instance along the tangents of the tensor inputs (an input without a
        tangent arrives as zeros, a None input as None) through ONE `SharedBatch.jvp` call on the device.  The tangents of Px /
        Ax are the shared [nnz] vectors: one direction of the model's values moves every instance.  The stamp rule of
        `backward` holds."""
        sb = ctx.sb
        if not stamp_holds(sb, ctx.stamp, None):
            raise RuntimeError("SharedBatchQPFunction: the batch has been solved again since this forward; its handle holds one "
                               "solution, so jvp must run before the next forward")
        cols = dict(q=sb.n, l=sb.m, u=sb.m, Px=sb.nnzP, Ax=sb.nnzA)
        tang = {k: t.contiguous() for k, t in zip(NAMES, (tq, tl, tu, tPx, tAx)) if k in ctx.given and t is not None and cols[k] > 0}
        ref = next(iter(tang.values()))
        tx = torch.empty((sb.count, sb.n), dtype=torch.float64, device=ref.device)
        ty = torch.empty((sb.count, sb.m), dtype=torch.float64, device=ref.device)
        _sync(ref)
        sb.jvp(**tang, out=dict(x=tx, y=ty) if sb.m else dict(x=tx))
        return tx, ty

    @staticmethod
    def backward(ctx, gx, gy):
        sb = ctx.sb
        if not stamp_holds(sb, ctx.stamp, None):
            raise RuntimeError("SharedBatchQPFunction: the batch has been solved again since this forward; its handle holds one "
                               "solution, so backward must run before the next forward")
        need = dict(zip(NAMES, ctx.needs_input_grad[1:6]))
        cols = dict(q=sb.n, l=sb.m, u=sb.m, Px=sb.nnzP, Ax=sb.nnzA)
        want = tuple(k for k in ("q", "l", "u") if need[k] and cols[k] > 0)
        sums = tuple(k for k in ("Px", "Ax") if need[k] and cols[k] > 0)
        if gx is None and gy is None:
            return (None,) * 6
        ref = gx if gx is not None else gy
        out = dict(zip(want + sums, SharedBatchQPAdjoint.apply(sb, ctx.stamp, want, sums, gx, gy))) if want or sums else {}
        # a wanted gradient of width zero: zeros (`ref` carries the batch axis of a vmapped pull-back)
        lead = tuple(ref.shape[:-2])
        zeros = {k: ref.new_zeros(lead + ((sb.count, 0) if k in ("q", "l", "u") else (0,))) for k in NAMES}
        grads = {k: (out[k] if k in out else (zeros[k] if need[k] else None)) for k in NAMES}
        return (None,) + tuple(grads[k] for k in NAMES)


class SharedBatchQPLayer(torch.nn.Module):
    """`layer(q=None, l=None, u=None, Px=None, Ax=None) -> (x, y)` on the shared batch `sb` (`batch.SharedBatch`: one model, many
    right-hand sides); `layer.info` is the info array [count x 6] of the last forward.  q, l, u: float64 CUDA tensors
    [count x .] (None keeps the handle's data; l and u come together); they update the handle and get per-instance gradients
    from `SharedBatch.adjoint`.  Px [nnz(P upper)], Ax [nnz(A)]: the SHARED values as float64 CUDA tensors -- they must equal
    the handle's values bit for bit (ValueError otherwise: a new model is a new handle) and get the gradients summed over the
    instances, "Px_sum" / "Ax_sum" of the same adjoint call.  `layer.Px` / `layer.Ax` are the handle's values on its device,
    ready to be cloned into parameters.  The stamp rule of `BatchQPLayer` holds: backward after a later forward raises.
    `torch.func.vmap` / `jacrev` over the pull-back is one adjoint call with a leading axis.  Forward mode (`torch.autograd.forward_ad`, `torch.func.jvp`) is one
    `SharedBatch.jvp` call: the tangents of q, l, u are per instance, those of Px / Ax are the shared [nnz] vectors."""

    def __init__(self, sb):
        super().__init__()
        self.sb, self.info = sb, None
        own = shared_values(sb, torch.device("cuda", sb.device))
        self.Px, self.Ax = own["Px"], own["Ax"]

    def forward(self, q=None, l=None, u=None, Px=None, Ax=None):
        x, y = SharedBatchQPFunction.apply(self.sb, q, l, u, Px, Ax)
        self.info = self.sb._qp_layer_info
        return x, y


def stamp_model_forward(model):
    """A forward has solved `model`: it carries that forward's stamp, which is returned (the single-model form of
    `stamp_forward`: a model holds ONE solution)."""
    model._qp_layer_stamp = getattr(model, "_qp_layer_stamp", 0) + 1
    return model._qp_layer_stamp


def _route(who, tensors):
    """True: the device route (every tensor a CUDA tensor), False: the host route (every tensor a CPU tensor, or none given);
    a mixture raises ValueError."""
    cuda = [t.is_cuda for t in tensors]
    if any(cuda) and not all(cuda):
        raise ValueError(f"{who}: CPU and CUDA tensors are mixed; give all of them on one side")
    return bool(cuda) and all(cuda)


class QPFunction(torch.autograd.Function):
    """(x, y) of a single model as a function of the data given: each tensor goes through `interface.update`, then `solve`,
    which must end Solved.  backward: ONE `interface.adjoint` call that asks only for the gradients of the inputs that
    require grad; it raises when a later forward has solved the model again (the stamp), and the library itself refuses a
    model that was updated or warm-started by hand since (OSQPError: no current solution).  CUDA tensors: the device forms
    throughout (x, y and the gradients are CUDA tensors the library writes into); CPU tensors: the host forms."""

    @staticmethod
    def forward(ctx, model, q, l, u, Px, Ax):
        given = dict(zip(NAMES, (q, l, u, Px, Ax)))
        for name, t in given.items():
            if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float64 or t.dim() != 1):
                raise ValueError(f"{name}: expected a one-dimensional float64 tensor")
        tensors = {name: t for name, t in given.items() if t is not None}
        on_device = _route("QPFunction", tensors.values())
        if on_device:
            ref = next(iter(tensors.values()))
            data = {name: t.detach().contiguous() for name, t in tensors.items()}
            _sync(ref)  # (after the copies `contiguous` may have queued)
            _iface.update(model, **data)
        elif tensors:
            _iface.update(model, **{name: t.detach().cpu().contiguous().numpy() for name, t in tensors.items()})
        res = _iface.solve(model)
        ctx.model, ctx.stamp = model, stamp_model_forward(model)
        ctx.given = tuple(tensors)  # for jvp: the inputs that can carry a tangent
        model._qp_layer_info = res.info
        if res.info.status != "Solved":
            raise RuntimeError(f"QPFunction: the solve ended with status {res.info.status}; there is no solution to differentiate")
        if on_device:
            n, m = _iface.dimensions(model)
            x = torch.empty(n, dtype=torch.float64, device=ref.device)
            y = torch.empty(m, dtype=torch.float64, device=ref.device)
            _sync(ref)
            _iface.solution(model, x=x, y=y)
            return x, y
        return torch.from_numpy(res.x.copy()), torch.from_numpy(res.y.copy())

    @staticmethod
    def jvp(ctx, t_model, tq, tl, tu, tPx, tAx):
        """Forward mode (`torch.autograd.forward_ad`): ONE `interface.jvp` call with the tangents of the inputs that carry
        one, on the factor `backward` uses; the same stamp rule."""
        model = ctx.model
        if getattr(model, "_qp_layer_stamp", None) != ctx.stamp:
            raise RuntimeError("QPFunction: the model has been solved again since this forward; it holds one solution, so "
                               "jvp must run before the next forward")
        tang = {k: t for k, t in zip(NAMES, (tq, tl, tu, tPx, tAx)) if k in ctx.given and t is not None and t.numel() > 0}
        if not tang:
            return None, None
        ref = next(iter(tang.values()))
        if _route("QPFunction.jvp", tang.values()):
            n, m = _iface.dimensions(model)
            tx = torch.empty(n, dtype=torch.float64, device=ref.device)
            ty = torch.empty(m, dtype=torch.float64, device=ref.device)
            data = {k: t.detach().contiguous() for k, t in tang.items()}
            _sync(ref)
            _iface.jvp(model, **data, out=dict(x=tx, y=ty))
            return tx, ty
        out = _iface.jvp(model, **{k: t.detach().cpu().contiguous().numpy() for k, t in tang.items()})
        return torch.from_numpy(out["x"]), torch.from_numpy(out["y"])

    @staticmethod
    def backward(ctx, gx, gy):
        model = ctx.model
        if getattr(model, "_qp_layer_stamp", None) != ctx.stamp:
            raise RuntimeError("QPFunction: the model has been solved again since this forward; it holds one solution, so "
                               "backward must run before the next forward")
        need = dict(zip(NAMES, ctx.needs_input_grad[1:6]))
        want = tuple(k for k in NAMES if need[k])
        if not want or (gx is None and gy is None):
            return (None,) * 6
        ref = gx if gx is not None else gy
        n, m = _iface.dimensions(model)
        if m == 0:
            gy = None
        if gx is None and gy is None:  # (m = 0 and only gy came: nothing reaches the data)
            return (None,) * 6
        if _route("QPFunction.backward", [g for g in (gx, gy) if g is not None]):
            gx, gy = (None if g is None else g.detach().contiguous() for g in (gx, gy))
            _sync(ref)
            out = _iface.adjoint(model, dx=gx, dy=gy, want=want)
            return (None,) + tuple(out[k] if need[k] else None for k in NAMES)
        out = _iface.adjoint(model, dx=None if gx is None else gx.detach().numpy(), dy=None if gy is None else gy.detach().numpy(), want=want)
        return (None,) + tuple(torch.from_numpy(out[k]) if need[k] else None for k in NAMES)


class QPLayer(torch.nn.Module):
    """`layer(q=None, l=None, u=None, Px=None, Ax=None) -> (x, y)` on the single model `model` (set up, direct back-end, not
    compact); `layer.info` is the `Info` of the last forward.  Px / Ax: full value arrays in the nnz order of `update`.
    Tensors on the model's device stay there (device-pointer forms, no host hop; x, y and the gradients come back as CUDA
    tensors); CPU tensors go the host way and give CPU tensors; both at once is a ValueError.
    derivative_method: "direct" (the kept factor, the default), "auto" or "iterative" -- `interface.derivative_method`,
    called once here; the last two serve a model on the indirect back-end, compact ones included.
    retain_factor: True calls `interface.adjoint_retain(model)` once here -- the factor of one backward serves the next
    step while the active set holds (a training loop); the default leaves the model's life cycle as it is."""

    def __init__(self, model, derivative_method="direct", retain_factor=False):
        super().__init__()
        self.model, self.info = model, None
        if derivative_method != "direct":
            _iface.derivative_method(model, derivative_method)
        if retain_factor:
            _iface.adjoint_retain(model, True)

    def forward(self, q=None, l=None, u=None, Px=None, Ax=None):
        try:
            return QPFunction.apply(self.model, q, l, u, Px, Ax)
        finally:
            self.info = getattr(self.model, "_qp_layer_info", None)
