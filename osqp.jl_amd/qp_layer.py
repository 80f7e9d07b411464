"""A resident batch as a differentiable torch layer: `BatchQPFunction` solves `count` QPs in its forward
(`ResidentBatch.update` + `solve`, device pointers, no host hop) and differentiates their solutions in its backward
(`ResidentBatch.adjoint`: one launch of k_batch_adjoint); under forward-mode differentiation (`torch.autograd.forward_ad`,
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

Three rules.  The library runs on its own stream and blocks, so torch's current stream is synchronised before every library
call.  The handle holds ONE solution per instance: every forward stamps the instances it served (all of them without
`rows`), and a backward raises RuntimeError when one of ITS instances has been served by a later forward -- two forwards on
disjoint selections can both run their backward (the forward-mode rule runs with its forward and needs no stamp).  Instances whose adjoint status is not 1 (no solution, failed factorisation) get zero gradients; where
an instance's active constraints are dependent the derivative does not exist and the regularised answer is returned
(include/osqp_amd.h, osqp_amd_batch_adjoint); the same holds for the tangents (osqp_amd_batch_jvp)."""
import numpy as np
import torch

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


class BatchQPFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rb, q, l, u, Px, Ax, rows=None):
        given = dict(zip(NAMES, (q, l, u, Px, Ax)))
        tensors = [t for t in given.values() if t is not None]
        if not tensors:
            raise ValueError("BatchQPFunction: at least one of q, l, u, Px, Ax must be a tensor")
        for name, t in given.items():
            if t is not None and (not t.is_cuda or t.dtype != torch.float64):
                raise ValueError(f"{name}: expected a float64 CUDA tensor")
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
        ctx.rb, ctx.sel, ctx.k, ctx.stamp = rb, sel, k, stamp_forward(rb, sel)
        ctx.given = tuple(name for name, t in given.items() if t is not None)  # for jvp: the inputs that have a tangent
        return x, y

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
        dev = gx.device if gx is not None else gy.device
        out = {k: torch.empty((ctx.k, cols[k]), dtype=torch.float64, device=dev) for k in want}
        _sync(gx if gx is not None else gy)
        rb.adjoint(dx=None if gx is None else gx.contiguous(), dy=None if gy is None or rb.m == 0 else gy.contiguous(), want=want, out=out,
                   rows=ctx.sel)
        grads = {k: (out[k] if k in out else (torch.zeros((ctx.k, 0), dtype=torch.float64, device=dev) if need[k] else None)) for k in NAMES}
        return (None,) + tuple(grads[k] for k in NAMES) + (None,) * (nargs - 6)


class BatchQPLayer(torch.nn.Module):
    """`layer(q=None, l=None, u=None, Px=None, Ax=None, rows=None) -> (x, y)` on the resident batch `rb`; `layer.info` is the
    info array [count x 6] of the last forward.  rows: a selection of the instances (`batch.selection`); the tensors, x, y
    and `layer.info` are then [k x .], row j for instance rows[j], and every other instance is left as it was."""

    def __init__(self, rb):
        super().__init__()
        self.rb, self.info = rb, None

    def forward(self, q=None, l=None, u=None, Px=None, Ax=None, rows=None):
        if rows is None:
            x, y = BatchQPFunction.apply(self.rb, q, l, u, Px, Ax)
        else:
            x, y = BatchQPFunction.apply(self.rb, q, l, u, Px, Ax, rows)
        self.info = self.rb._qp_layer_info
        return x, y
