"""bench.py's plain run on the GPU: exactly `--steps` timed steps, none of the `--full` legs, and `--dump-outputs`
writing what the timed path computed in its last step -- for a single QP the iterate after W + K iterations, the same
bits the library gives when driven directly; for the batch the packed x / y / info of all 4096 instances."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(argv, timeout=600):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR", "LOCAL_WORLD_SIZE", "OSQP_AMD_BENCH_SPAWNED")
           and not k.startswith("TORCHELASTIC_")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=timeout)
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, p.stderr.decode()[-3000:] + p.stdout.decode()[-1000:]
    return json.loads(lines[0])


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_dumps_the_iterate_of_its_last_step(product_lib, tmp_path):
    import osqp_jl_amd as oq

    W, K = 3, 7
    rec = _bench(["--workload", "rand-2e4", "--steps", str(K), "--warmup", str(W), "--dump-outputs", str(tmp_path / "a")])
    assert (rec["steps"], rec["warmup"], rec["n_gpus"]) == (K, W, 1)
    assert rec["metric"] == "ADMM iterations/sec" and rec["unit"] == "iterations/s" and rec["higher_is_better"] and rec["dtype"] == "f64"
    assert rec["ms_per_step"] > 0 and abs(rec["value"] - 1e3 / rec["ms_per_step"]) <= 1e-2 * rec["value"]
    for key in ("time_to_eps_s", "roofline", "cpu_baseline", "other_workloads", "per_rank"):
        assert key not in rec, key  # --full only
    x, y = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "y.npy")
    assert x.dtype == y.dtype == np.float64 and x.shape == (rec["config"]["n"],) and y.shape == (rec["config"]["m"],)

    # the library driven directly: the same instance, W then K iterations, the iterate in the caller's units
    bench = _bench_module()
    kind, n, per_row, linsys = bench.WORKLOADS["rand-2e4"]
    m = oq.Model(product_lib)
    oq.setup_generated(m, kind, n, per_row, 1, linsys_solver=linsys, **bench.SETTINGS)
    assert product_lib.osqp_amd_iterate(m.workspace, W) == 0 and product_lib.osqp_amd_iterate(m.workspace, K) == 0
    xr, yr = np.empty(x.size), np.empty(y.size)
    ptr = C.POINTER(C.c_double)
    assert product_lib.osqp_amd_get_iterate(m.workspace, xr.ctypes.data_as(ptr), yr.ctypes.data_as(ptr)) == 0
    oq.clean(m)
    assert np.array_equal(x, xr) and np.array_equal(y, yr)

    # the same arguments give the same inputs, hence the same outputs
    _bench(["--workload", "rand-2e4", "--steps", str(K), "--warmup", str(W), "--dump-outputs", str(tmp_path / "b")])
    assert np.array_equal(x, np.load(tmp_path / "b" / "x.npy")) and np.array_equal(y, np.load(tmp_path / "b" / "y.npy"))


def test_plain_batch_run_dumps_the_whole_packed_batch(product_lib, tmp_path):
    rec = _bench(["--workload", "mpc-batch", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["cpu_baseline"] is None and rec["roofline"]["traffic"] is None
    x, y, info = (np.load(tmp_path / (k + ".npy")) for k in ("x", "y", "info"))
    assert x.shape == (4096, 100) and y.shape == (4096, 200) and info.shape == (4096, 4)
    assert int((info[:, 1] == 1).sum()) == rec["solved"] == 4096
    assert np.isfinite(x).all() and np.isfinite(y).all()
