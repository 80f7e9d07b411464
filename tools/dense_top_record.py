#!/usr/bin/env python3
"""One record of the direct back-end on problems whose factor takes a dense top block (tests/qp_zoo.py: equality_qp -- a dense P --,
portfolio, svm) and on the one whose block fails the probe (lasso_data(30, 300)): status, iterations, setup and solve time,
numeric factorisations, pivots of the block after the solve, and a hash of the solution's bits.  The library is the one
`OSQP_AMD_LIB` names (default: this tree's), so that two builds can be alternated and compared line by line.  A report, not a
gate.
usage: python tools/dense_top_record.py"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import osqp_jl_amd as oq  # noqa: E402
import qp_zoo  # noqa: E402

lib = oq.load_library()
OPTS = dict(verbose=False, eps_abs=1e-5, eps_rel=1e-5, adaptive_rho_interval=50, max_iter=4000, polish=True)
PROBLEMS = (("equality_qp", qp_zoo.equality_qp()), ("equality_qp300", qp_zoo.equality_qp(n=300)), ("portfolio", qp_zoo.portfolio()),
            ("svm", qp_zoo.svm()), ("lasso_data_30_300", qp_zoo.lasso_data(n=30, m=300)))
for name, prob in PROBLEMS:
    model = oq.Model(lib)
    oq.setup(model, **prob, **OPTS)
    r = oq.solve(model)
    st = oq.stats(model)
    digest = hashlib.sha256(np.ascontiguousarray(r.x).tobytes() + np.ascontiguousarray(r.y).tobytes()).hexdigest()[:16]
    print(json.dumps(dict(problem=name, status=r.info.status, iters=r.info.iter, polish=r.info.status_polish, setup_ms=r.info.setup_time * 1e3,
                          solve_ms=r.info.solve_time * 1e3, polish_ms=r.info.polish_time * 1e3, factorizations=int(st[8]), backend=int(st[0]),
                          dense_block=int(st[25]), xy_sha16=digest)), flush=True)
    oq.clean(model)
