"""GPU: one plain bench.py run. It prints the headline line without the legs that
--full adds, and --dump-outputs leaves the actions of the last timed step: the
seeded observations (seed 1 + rank, the same in every run) through the policy,
checked against the fp64 oracle at the parity bound of test_gpu_parity.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import abs_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dumped_actions(tmp_path, synth_path):
    import torch
    from oracle import mlp_ref
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--settle-s", "0", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["n_gpus"] == 1 and d["dtype"] == "f32" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and d["kernel_us"] > 0
    assert abs(d["value"] - 4096 / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    for leg in ("cpu_baseline", "gru256", "controller_tick", "latency_b1_p50_us", "latency_b1_act_cpp"):
        assert leg not in d, leg
    assert d["host_enqueue_us"] is None
    a = np.load(out / "actions.npy")
    assert a.dtype == np.float32 and a.shape == (1, 4096, 12) and d["outputs"]["shape"] == [1, 4096, 12]
    obs = torch.randn((1, 4096, 48), generator=torch.Generator(device="cpu").manual_seed(1)).numpy()
    ref = mlp_ref.MlpRef.from_onnx(synth_path("go2_mlp_512"))
    assert abs_err(a[0], ref.f64(obs[0])) <= 1e-5
