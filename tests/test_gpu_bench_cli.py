"""bench.py's command line: a plain run prints the headline line only (``--steps`` timed steps, ``ms_per_step``),
``--full`` is what adds every other measurement, and ``--dump-outputs`` writes the last timed step's outputs
as float32 / float64 ``.npy`` files of at most 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "roofline_attention", "train_step_with_adam", "bf16_mode", "dp_schedule", "cpu_baseline")


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    T, steps, nv = 256, 3, 2
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--T", str(T), "--dump-outputs", str(out)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["full"] is False and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0
    # value = frames of the timed steps / their wall time, ms_per_step = that wall time / steps (both rounded)
    assert d["value"] * d["ms_per_step"] * 1e-3 == pytest.approx(nv * T, rel=1e-2)
    assert not [k for k in FULL_ONLY if k in d]
    names = sorted(os.listdir(out))
    assert all(n.endswith(".npy") for n in names)
    arrs = {n[:-4]: np.load(out / n) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 * 2 ** 20
    assert all(np.isfinite(a).all() for a in arrs.values())
    assert arrs["loss"].shape == (1,) and arrs["loss"][0] > 0
    C = arrs["frame_clogit_b0_v0"].shape[1]
    for v in range(nv):
        assert arrs[f"pred_v{v}"].shape == (T,)
        assert arrs[f"frame_clogit_b3_v{v}"].shape == (T, C)
    assert arrs["tdu_segments"].tolist() == d["config"]["tdu_segments_after_timing"]
    assert arrs["grad_param_l2"].shape == arrs["grad_param_sum"].shape and (arrs["grad_param_l2"] > 0).any()
    assert np.abs(arrs["grad_sample"]).max() > 0


def test_full_and_dump_options_exist():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout, r.stderr[-2000:]
