"""bench.py's command line: `--steps` is the number of timed steps, `--dump-outputs DIR` writes what the last timed
step computed (its loss and the updated parameters) as float .npy files within the 64 MB budget, and a run without
`--full` prints the headline figure alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--layers", "2", "--batch", "8", "--seq", "64"]


def test_bench_refuses_zero_timed_steps():
    """No timed step means no ms_per_step: refused on the command line, before torch or the GPU is touched."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


@pytest.mark.gpu
def test_bench_dump_outputs_holds_the_last_timed_step(tmp_path):
    import bench
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)] + SMALL, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["metric"] == "train samples/sec BioBERT-base NER seq256" and line["unit"] == "samples/s"
    assert line["higher_is_better"] is True and line["dtype"] == "bf16" and line["value"] > 0
    # no --full: nothing beyond the headline was measured
    assert not {"roofline", "f32", "loss_at_step100", "cpu_baseline", "tf_reference"} & set(line)
    assert sorted(os.listdir(out_dir)) == ["loss.npy", "params.npy"]
    arrays = {n: np.load(out_dir / n, allow_pickle=False) for n in os.listdir(out_dir)}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    loss, params = arrays["loss.npy"], arrays["params.npy"]
    assert loss.shape == (1,) and round(float(loss[0]), 5) == line["loss_last"]
    # BERT-base width with 2 layers is larger than the budget: a seeded sample of DUMP_SAMPLE distinct parameters
    assert params.shape == (bench.DUMP_SAMPLE,)
    assert np.isfinite(params).all() and np.abs(params).max() > 0
