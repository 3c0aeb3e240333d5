"""`python bench.py --gpus 1 --steps K --warmup W`: a plain run times the headline only (the secondary legs run with
``--full``), and ``--dump-outputs`` writes what the last timed step returned -- the same arrays from run to run, since
every input is seeded."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench(args, timeout=600):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1"] + args, capture_output=True, text=True, timeout=timeout,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_its_outputs(tmp_path):
    out = _bench(["--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path / "a")])
    assert out["steps"] == 4 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "sub-steps/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    E, N = out["config"]["envs_per_gpu"], out["config"]["grid_points"]
    assert out["value"] == pytest.approx(E * 250 / (out["ms_per_step"] * 1e-3), rel=1e-9)
    for leg in ("cpu_baseline", "end_to_end", "episode_inclusive", "workload_c2", "tbptt", "burgers_fno"):
        assert leg not in out, leg
    assert "hbm_copy_measured" not in out["roofline"]

    def load(run, name):
        return np.load(tmp_path / run / f"{name}.npy")
    kinds = {"obs": ((E, N), np.float32), "ssq": ((E,), np.float64), "status": ((E,), np.float64),
             "state": ((E, N), np.float64)}
    for name, (shape, dtype) in kinds.items():
        x = load("a", name)
        assert x.shape == shape and x.dtype == dtype and np.isfinite(x).all(), name
    assert not load("a", "status").any()
    assert (load("a", "ssq") > 0).all()
    # the observation is the fp32 rounding of the state the step ended in
    np.testing.assert_array_equal(load("a", "obs"), load("a", "state").astype(np.float32))

    _bench(["--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path / "b")])
    for name in kinds:
        np.testing.assert_array_equal(load("a", name), load("b", name), err_msg=name)
