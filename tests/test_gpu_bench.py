"""bench.py's plain run and --dump-outputs: the line holds the headline alone, and two runs with the same arguments
write the same arrays (the timed pass restarts the stream after the spin-up)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_dump_outputs_are_reproducible(tmp_path):
    outs = []
    for i in range(2):
        d = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / str(i)))
        assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False and d["dtype"] == "f32"
        assert d["ms_per_step"] > 0 and d["higher_is_better"] is True and d["unit"] == "frames/s"
        B = d["config"]["windows_per_gpu"]
        assert abs(d["value"] * d["ms_per_step"] / 1e3 - B) < 0.01 * B
        for k in ("roofline", "kernel_ms", "cpu_baseline", "ms_per_step_no_spinup", "ms_per_step_cached_input",
                  "experimental_split_bf16", "collective"):
            assert k not in d, k                                # measured with --full only
        assert sorted(d["dumped_outputs"]) == ["blendshapes", "ema_state"]
        outs.append({n: np.load(tmp_path / str(i) / (n + ".npy")) for n in d["dumped_outputs"]})
    for n, a in outs[0].items():
        assert a.dtype == np.float32 and a.shape == (B, 52) and np.isfinite(a).all(), n
        assert np.array_equal(a, outs[1][n]), n
