"""The probe of the dense top block's explicit inverse (csrc/direct.hip: LdlFactor, dense_probe_tol).
qp_zoo.lasso_data(n=30, m=300): variables without a cost term (pivots of sigma / delta) under a dense top block of 390 of the
720 pivots.  The inverse by unpivoted Gauss-Jordan sweeps is useless there -- before the probe the direct back-end ended at
Max_iter_reached with pri_res 1.2e2 and a polish on the reduced factor was rejected; the triangular solves of the same pivots
serve.  With the probe the factor is rebuilt without the block: the solve ends Solved, the polish is accepted, the solution is
the oracle's.  Tolerance: the one of the smoke run, 2e-4 relative at eps = 1e-5 (both sides polished).
A problem whose block passes the probe keeps it (equality_qp: a dense P)."""
import numpy as np
import pytest

import osqp_jl_amd as oq
import qp_zoo
from batch_resident_ref import OPTS

pytestmark = pytest.mark.gpu


def test_a_block_that_fails_the_probe_is_given_up(product_lib, oracle_lib):
    p = qp_zoo.lasso_data(n=30, m=300)
    res = {}
    for name, lib in (("gpu", product_lib), ("oracle", oracle_lib)):
        mdl = oq.Model(lib)
        oq.setup(mdl, **p, **dict(OPTS, polish=True))
        res[name] = oq.solve(mdl)
        if name == "gpu":
            st = oq.stats(mdl)
            assert st[0] == 0.0  # the direct back-end
            assert st[25] == 0.0  # ... without the block by now
        oq.clean(mdl)
    g, o = res["gpu"], res["oracle"]
    print(f"iterations gpu / oracle {g.info.iter} / {o.info.iter}  polish {g.info.status_polish} / {o.info.status_polish}  "
          f"max |dx| {np.max(np.abs(g.x - o.x)):.2e}")
    assert g.info.status == o.info.status == "Solved" and g.info.status_polish == 1
    assert np.max(np.abs(g.x - o.x)) <= 2e-4 * max(1.0, float(np.max(np.abs(o.x))))
    assert np.max(np.abs(g.y - o.y)) <= 2e-4 * max(1.0, float(np.max(np.abs(o.y))))


def test_a_block_that_passes_the_probe_is_kept(product_lib):
    p = qp_zoo.equality_qp(n=300)
    mdl = oq.Model(product_lib)
    oq.setup(mdl, **p, **OPTS)
    r = oq.solve(mdl)
    st = oq.stats(mdl)
    oq.clean(mdl)
    assert r.info.status == "Solved" and st[0] == 0.0 and st[25] > 0.0
