"""`qp_layer.QPLayer` on CUDA tensors: the device route (osqp_amd_*_dev, no host hop) against the same layer on CPU tensors
and a twin model.  The two routes run the same kernels on the same operands, so every comparison is bitwise."""
import numpy as np
import pytest

import osqp_jl_amd as oq
import model_adjoint_ref as mar
from batch_resident_ref import OPTS

pytestmark = pytest.mark.gpu

NO_CALLS = dict(update_vectors=0, update_values=0, warm_start=0, solution=0, adjoint=0, jvp=0)


def _model(product_lib, p):
    mdl = oq.Model(product_lib)
    oq.setup(mdl, **mar.setup_args(p), **dict(OPTS, polish=True))
    return mdl


def _inputs(p, device):
    import torch

    A = p["A_given"] if "A_given" in p else p["A"]
    data = dict(q=p["q"], l=p["l"], u=p["u"], Ax=np.array(A.data, dtype=np.float64))
    return {k: torch.tensor(v, dtype=torch.float64, device=device, requires_grad=True) for k, v in data.items()}


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("case", ["control6_unsorted", "tiny"])
def test_cuda_tensors_take_the_device_route(product_lib, oracle_lib, case):
    import torch
    from torch.autograd import forward_ad

    from osqp_jl_amd.qp_layer import QPLayer

    p = mar.problems(oracle_lib, case)[0]
    n, m = len(p["q"]), len(p["l"])
    w, v = (g[0] for g in mar.incoming(case, 0, n, m))
    runs = {}
    for device in ("cuda:0", "cpu"):
        mdl = _model(product_lib, p)
        layer = QPLayer(mdl)
        t = _inputs(p, device)
        x, y = layer(**t)
        assert layer.info.status == "Solved"
        assert x.device.type == y.device.type == torch.device(device).type
        ((torch.tensor(w, device=device) * x).sum() + (torch.tensor(v, device=device) * y).sum()).backward()
        assert all(t[k].grad.device.type == torch.device(device).type for k in t)
        calls = oq.device_form_calls(mdl)
        assert calls == (dict(NO_CALLS, update_vectors=1, update_values=1, solution=1, adjoint=1) if device != "cpu" else NO_CALLS)
        # forward mode along q
        tq = torch.tensor(w, device=device)
        with forward_ad.dual_level():
            xd, yd = layer(q=forward_ad.make_dual(t["q"].detach(), tq))
            tx, ty = forward_ad.unpack_dual(xd).tangent, forward_ad.unpack_dual(yd).tangent
        assert tx.device.type == torch.device(device).type
        calls = oq.device_form_calls(mdl)
        assert calls == (dict(NO_CALLS, update_vectors=2, update_values=1, solution=2, adjoint=1, jvp=1) if device != "cpu" else NO_CALLS)
        runs[device] = dict(x=x, y=y, tx=tx, ty=ty, **{"d" + k: t[k].grad for k in t})
        oq.clean(mdl)
    for k, on_device in runs["cuda:0"].items():
        assert _same(on_device.detach().cpu().numpy(), runs["cpu"][k].detach().numpy()), k


def test_mixed_inputs_and_the_stamp_rule(product_lib, oracle_lib):
    import torch

    from osqp_jl_amd.qp_layer import QPLayer

    p = mar.problems(oracle_lib, "control6_unsorted")[0]
    mdl = _model(product_lib, p)
    layer = QPLayer(mdl)
    with pytest.raises(ValueError, match="mixed"):
        layer(q=torch.tensor(p["q"], device="cuda:0"), l=torch.tensor(p["l"]))
    assert oq.device_form_calls(mdl) == NO_CALLS
    # the model holds one solution: a backward after a later forward raises on the device route as on the host route
    q1 = torch.tensor(p["q"], device="cuda:0", requires_grad=True)
    x1, _ = layer(q=q1)
    layer(q=q1.detach())
    with pytest.raises(RuntimeError, match="solved again"):
        x1.sum().backward()
    # ... and the library refuses a model that was updated by hand since
    q2 = torch.tensor(p["q"], device="cuda:0", requires_grad=True)
    x2, _ = layer(q=q2)
    oq.update(mdl, q=torch.tensor(p["q"] * 1.5, device="cuda:0"))
    with pytest.raises(oq.OSQPError, match="osqp_solve"):
        x2.sum().backward()
    oq.clean(mdl)
