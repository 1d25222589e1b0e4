"""bench.py command-line contract, on a tiny CPU-sized problem: --steps
is honoured, --full is accepted, the result line carries ms_per_step, and
--dump-outputs writes the last step's arrays with identical inputs from
run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--nodes", "3000",
        "--edges", "20000", "--batch-size", "64", "--fanout", "3,2",
        "--feat-dim", "16", "--hidden", "16", "--classes", "5"]


def _start(out_dir, *extra):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    return subprocess.Popen(
        [sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, *extra,
         "--dump-outputs", str(out_dir)],
        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env,
        cwd=ROOT)


def _finish(p):
    out, err = p.communicate(timeout=120)
    assert p.returncode == 0, err[-2000:]
    return json.loads(out.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def two_runs(tmp_path_factory):
    a = tmp_path_factory.mktemp("dump_a")
    b = tmp_path_factory.mktemp("dump_b")
    pa, pb = _start(a), _start(b, "--full")  # side by side: import-bound
    return (_finish(pa), a), (_finish(pb), b)


def test_result_line(two_runs):
    for res, _ in two_runs:
        assert res["steps"] == 3 and res["warmup"] == 1
        assert res["ms_per_step"] > 0
        assert res["unit"] == "batches/s" and res["higher_is_better"] is True
        assert res["value"] == pytest.approx(1000.0 / res["ms_per_step"],
                                             rel=1e-2)
        assert {"metric", "dtype"} <= set(res)
        assert res["deterministic"] is True


def test_dump_outputs_files_and_same_inputs(two_runs):
    (_, a), (_, b) = two_runs
    names = sorted(os.listdir(a))
    assert names == ["labels.npy", "logits.npy", "loss.npy",
                     "seed_nodes.npy"]
    assert sorted(os.listdir(b)) == names
    arr = {n: (np.load(os.path.join(a, n)), np.load(os.path.join(b, n)))
           for n in names}
    for x, y in arr.values():
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape
    assert arr["logits.npy"][0].shape == (64, 5)
    assert arr["loss.npy"][0].shape == (1,)
    assert np.isfinite(arr["logits.npy"][0]).all()
    # same arguments -> same batch, same labels, and (CPU kernels are
    # sequential) the same numbers
    assert np.array_equal(*arr["seed_nodes.npy"])
    assert np.array_equal(*arr["labels.npy"])
    assert np.array_equal(*arr["logits.npy"])
    assert np.array_equal(*arr["loss.npy"])
