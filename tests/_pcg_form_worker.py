"""One form of the CG iteration in a process of its own (started by test_pcg_reference_gpu.py; not a test module): the forms
whose switches pcg.hip reads once per process (`static const`), so the environment must be set before the library's first solve.

usage: _pcg_form_worker.py FORM OUT_NPZ     (the form's environment is set by the parent)
Runs every small case of pcg_reference.py through R1 - R4 on the indirect back-end, asserts the back-end and the SpMV layout
the form demands, and writes every call's x, y, status, iteration count, residuals, rho updates, statistics and the iterate
after the last call to OUT_NPZ, keyed "<case>/<run>/<call>/<field>"."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    form, out = sys.argv[1], sys.argv[2]
    import numpy as np

    import osqp_jl_amd as oq
    import pcg_drive as pd
    import pcg_reference as pr

    lib = oq.load_library()
    rec = {}
    for name in pr.SMALL:
        for run in ("R1", "R2", "R3", "R4"):
            calls, _ = pr.cached_run(name, run)
            got = pd.drive(lib, name, run, calls, "pcg", after_setup=lambda m: pd.assert_form(m, form != "csr", form), get_iterate=True)
            for k, g in enumerate(got):
                for field, v in g.items():
                    rec[f"{name}/{run}/{k}/{field}"] = np.asarray(v)
    np.savez(out, **rec)


if __name__ == "__main__":
    main()
