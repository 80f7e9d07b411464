"""`qp_layer.QPLayer(model, derivative_method="iterative")`: the torch layer of a single model on the iterative KKT solve
(osqp_amd_derivative_method).  tiny (8 instances): the gradients of backward() against those of a layer
on the kept factor ("direct") over the same data, within the sum of the two bounds of tests/test_model_adjoint_iter_gpu.py
(each method against `exact`), with CPU tensors (host form) and CUDA tensors (device form)."""
import numpy as np
import pytest

import osqp_jl_amd as oq
import model_adjoint_ref as mar
from batch_resident_ref import OPTS
from test_model_adjoint_host import MEASURED
from test_model_adjoint_iter_host import MEASURED_ITER

pytestmark = pytest.mark.gpu

EPS = 2.2e-16


def _grads(product_lib, p, method, device, w, v):
    import torch

    from osqp_jl_amd.qp_layer import QPLayer

    mdl = oq.Model(product_lib)
    oq.setup(mdl, **mar.setup_args(p), **dict(OPTS, polish=True, linsys_solver="pcg"))
    layer = QPLayer(mdl, derivative_method=method)
    t = {k: torch.tensor(p[k], dtype=torch.float64, device=device, requires_grad=True) for k in ("q", "l", "u")}
    x, y = layer(**t)
    assert layer.info.status == "Solved" and x.device.type == device.split(":")[0]
    ((torch.tensor(w, device=device) * x).sum() + (torch.tensor(v, device=device) * y).sum()).backward()
    it, st = oq.derivative_iter_stats(mdl), oq.adjoint_stats(mdl)
    act = oq.adjoint(mdl, want=())["act"]
    oq.clean(mdl)
    assert it["kept"] == (1 if method == "iterative" else 0) and st["kept"] == 1
    return {k: t[k].grad.cpu().numpy() for k in t}, act


@pytest.mark.parametrize("device", ["cpu", "cuda:0"])
def test_iterative_layer_against_direct_layer(product_lib, oracle_lib, device):
    case = "tiny"
    for k, p in enumerate(mar.problems(oracle_lib, case)):
        n, m = len(p["q"]), len(p["l"])
        w, v = (g[0] for g in mar.incoming(case, k, n, m))
        gi, act = _grads(product_lib, p, "iterative", device, w, v)
        gd, act_d = _grads(product_lib, p, "direct", device, w, v)
        assert np.array_equal(act, act_d)
        cond = np.linalg.cond(mar.dense_K(p["P"], p["A"], act))
        bound = max(1000 * MEASURED_ITER[case], 1000 * cond * EPS) + max(1000 * MEASURED[case], 1000 * cond * EPS)
        worst = max(float(np.max(np.abs(gi[name] - gd[name]))) / max(1.0, float(np.max(np.abs(gd[name])))) for name in gi)
        print(f"tiny[{k}] {device}: iterative layer against direct layer {worst:.2e} / {bound:.2e}")
        assert worst <= bound
