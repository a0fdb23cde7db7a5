"""bench.py's plain run on one GPU: the headline line only, `--steps` timed steps, and with --dump-outputs the frame the timed
steps computed -- the same frame from two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_frame_of_its_timed_steps(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    out = bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(a))
    assert out["steps"] == 3 and out["value"] > 0 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
    assert out["unit"] == "Mpath-samples/s" and out["dtype"] == "f32"
    for key in ("roofline", "secondary", "cpu_baseline", "summary"):   # what only --full measures
        assert key not in out, key
    hdr = np.load(a / "hdr.npy")
    assert hdr.dtype == np.float32 and hdr.shape == (1080, 1920, 3) and np.isfinite(hdr).all() and hdr.max() > 0
    bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(b))
    assert np.array_equal(hdr.view(np.uint32), np.load(b / "hdr.npy").view(np.uint32))
