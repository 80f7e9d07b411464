"""bench.py's --dump-outputs writer and its options, on the host: float64 .npy files, and past the size limit the same
fixed, seeded sample of every array in every run."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_options_default_to_a_plain_run():
    bench = _bench()
    a = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"
    assert bench.parse_args(["--cpu-full"]).full  # the CPU record belongs to the --full line
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_outputs_are_written_as_float64(tmp_path):
    bench = _bench()
    x = np.arange(10, dtype=np.float32)
    info = np.arange(12).reshape(3, 4)
    bench.dump_outputs(str(tmp_path / "d"), {"x": x, "info": info})
    assert sorted(os.listdir(tmp_path / "d")) == ["info.npy", "x.npy"]
    gx, gi = np.load(tmp_path / "d" / "x.npy"), np.load(tmp_path / "d" / "info.npy")
    assert gx.dtype == gi.dtype == np.float64
    assert np.array_equal(gx, x) and np.array_equal(gi, info)


def test_outputs_past_the_limit_are_a_fixed_seeded_sample(tmp_path):
    bench = _bench()
    bench.DUMP_LIMIT_BYTES = 8000
    rng = np.random.default_rng(3)
    arrays = {"x": rng.standard_normal(1000), "y": rng.standard_normal((40, 50))}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    total = 0
    for name, full in arrays.items():
        idx = np.load(tmp_path / "a" / (name + "_index.npy"))
        val = np.load(tmp_path / "a" / (name + ".npy"))
        assert val.dtype == np.float64 and 0 < val.size == idx.size < full.size
        assert np.array_equal(val, full.reshape(-1)[idx.astype(np.int64)])
        assert np.array_equal(idx, np.load(tmp_path / "b" / (name + "_index.npy")))
        assert np.array_equal(val, np.load(tmp_path / "b" / (name + ".npy")))
        total += idx.nbytes + val.nbytes
    assert total <= bench.DUMP_LIMIT_BYTES
