"""GPU: a plain bench.py run (no --full) on a small member of the family -- it times the steps, writes what --dump-outputs asks for and prints
ONE line that carries the headline and nothing that only a --full run measures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_alone(tmp_path):
    dump = str(tmp_path / "out")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--views", "2", "--image", "128",
           "--volume", "32", "--layers", "18", "--dtype", "fp32", "--preroll-s", "0", "--dump-outputs", dump]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["unit"] == "samples/s" and res["higher_is_better"] is True and res["dtype"] == "fp32"
    assert res["steps"] == 2 and res["warmup"] == 1 and res["value"] > 0 and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(2 * 1e3 / res["ms_per_step"], rel=1e-4)          # samples per step / time per step
    for k in ("roofline", "roofline_hbm", "parity", "fp32_parity_mode", "batch_sweep", "cpu_baseline", "config4", "train", "full_record"):
        assert k not in res, k
    assert res["dumped_outputs"] == dump
    kp = np.load(os.path.join(dump, "keypoints_3d.npy"))
    assert kp.shape == (2, 17, 3) and np.isfinite(kp).all()
