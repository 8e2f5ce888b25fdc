"""bench.py's options beside the timed path: --full is off by default and gates the
legs beside the headline figure; --dump-outputs writes the coordinates whole when they
fit DUMP_BYTES and as a fixed, seeded, ascending row sample when they do not."""
import importlib.util
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    keys = ("OMP_PROC_BIND", "OMP_PLACES")  # bench.py sets these for its own process
    before = {k: os.environ.get(k) for k in keys}
    spec = importlib.util.spec_from_file_location("ge_bench", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(mod)
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return mod


def test_plain_run_is_the_default(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse()
    assert args.full and args.dump_outputs == "d"


def test_dump_outputs_whole_and_sampled(bench, tmp_path, monkeypatch):
    import torch
    dim = 3
    X = torch.arange(1000 * dim, dtype=torch.float64).reshape(1000, dim)
    bench.dump_outputs(str(tmp_path / "whole"), X)
    got = np.load(tmp_path / "whole" / "X.npy")
    assert got.dtype == np.float64 and np.array_equal(got, X.numpy())
    # an array above the limit: the same ascending sample of whole rows on every call
    monkeypatch.setattr(bench, "DUMP_BYTES", 100 * 8 * dim)
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), X)
    a, b = np.load(tmp_path / "a" / "X.npy"), np.load(tmp_path / "b" / "X.npy")
    assert a.shape == (100, dim) and a.dtype == np.float64 and np.array_equal(a, b)
    rows = (a[:, 0] / dim).astype(np.int64)
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, X.numpy()[rows])
