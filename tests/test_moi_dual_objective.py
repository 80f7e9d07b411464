"""MOI.DualObjectiveValue on the HIP engine (`Optimizer.dual_objective_value`): the attribute the
reference's conformance run excludes [REF test/MOI_wrapper.jl:36-37].  Every case of tests/moi_conformance.py runs with
`expect_optimal` wrapped: wherever a case expects an optimum with objective `obj`, the dual objective must equal it too, to
the atol / rtol of the reference's own MOI.Test.Config (1e-4 each) [REF test/MOI_wrapper.jl:28-39]."""
import pytest

import moi_conformance

pytestmark = pytest.mark.gpu

ATOL = RTOL = 1e-4


@pytest.mark.parametrize("case", moi_conformance.ALL, ids=lambda f: f.__name__)
def test_dual_objective_equals_the_expected_optimum(product_lib, monkeypatch, case):
    plain = moi_conformance.expect_optimal
    seen = []

    def expect_optimal(opt, idx, obj, *args, **kwargs):
        plain(opt, idx, obj, *args, **kwargs)
        dual = opt.dual_objective_value()
        seen.append((obj, dual))
        print(f"{case.__name__}: objective {opt.objective_value():.9g} dual objective {dual:.9g} expected {obj:.9g}")
        assert abs(dual - obj) <= max(ATOL, RTOL * max(abs(dual), abs(obj))), (case.__name__, dual, obj)

    monkeypatch.setattr(moi_conformance, "expect_optimal", expect_optimal)
    case(product_lib)
