"""CPU: bench.py's multi-GPU contract without a GPU (--dry-run: no device work).

`python3 bench.py --gpus N` (WORLD_SIZE unset, the driver's single-command form)
must start N ranks itself, one process per GPU, and report n_gpus = N with the
whole-job global batch; under torch.distributed.run (WORLD_SIZE set) a mismatch
between --gpus and the world size is an error (BASELINE configs[3])."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra=None, timeout=180):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout, env=env)


@pytest.mark.parametrize("n", [2, 3])
def test_bench_launches_its_own_ranks(n):
    r = _run(["--gpus", str(n), "--same-device", "--dist-backend", "gloo", "--dry-run", "--steps", "5",
              "--warmup", "1"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == n
    assert d["config"]["global_batch"] == 4096 * n
    assert d["config"]["parallelism"].startswith(f"dp{n}")
    assert d["scaling"] == "weak" and d["steps"] == 5 and d["dry_run"]
    assert d["metric"].startswith("control steps/sec")


def test_bench_world_mismatch_fails():
    r = _run(["--gpus", "4", "--dry-run", "--steps", "1"], {"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in r.stderr


def test_bench_failing_rank_fails_the_job():
    # ranks that cannot start (here: an RCCL process group on a host without a GPU)
    # must fail the job with a non-zero status, not leave the launcher waiting
    r = _run(["--gpus", "2", "--dry-run", "--steps", "1", "--dist-backend", "nccl"], timeout=120)
    assert r.returncode != 0


def test_bench_options_parse_and_line_fields():
    """--full and --dump-outputs exist; a dry run (no device work) computes nothing, so it
    writes no outputs, and its line carries the headline fields with ms_per_step."""
    r = _run(["--gpus", "1", "--steps", "7", "--warmup", "2", "--dry-run", "--full", "--dump-outputs",
              os.path.join(ROOT, "build", "never_written")])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["steps"] == 7 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["unit"] == "control steps/sec" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] >= 0 and d["value"] > 0
    assert not os.path.exists(os.path.join(ROOT, "build", "never_written"))


def test_models_go_elsewhere_when_the_tree_cannot_be_written(tmp_path, monkeypatch):
    """The benchmark may run from a checkout its user cannot write: what it generates goes
    to build/ in the tree when that can be made, else to a per-user directory under the
    temp dir, and the model written there is the pinned one."""
    import hashlib
    import tempfile
    sys.path.insert(0, ROOT)
    import bench
    from go2_onnx_controller_amd import synth
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    assert bench.work_dir() == str(tmp_path / "build")
    blocker = tmp_path / "not_a_directory"
    blocker.write_text("")
    monkeypatch.setattr(bench, "ROOT", str(blocker))  # build/ cannot be made under a file
    monkeypatch.setattr(tempfile, "tempdir", str(tmp_path / "tmp"))
    (tmp_path / "tmp").mkdir()
    d = bench.work_dir()
    assert d.startswith(str(tmp_path / "tmp")) and os.path.isdir(os.path.join(d, "models"))
    path = bench.synth_model("tiny")
    assert os.path.dirname(path) == os.path.join(d, "models")
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == synth.sha256("tiny")


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """dump_outputs writes float32 [ticks, robots, out]; above the size limit it keeps a
    fixed sorted sample of the robot rows, the same rows on every call."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    act = torch.arange(3 * 50 * 12, dtype=torch.float32).reshape(3, 50, 12)
    info = bench.dump_outputs(str(tmp_path / "a"), "actions", act)
    a = np.load(tmp_path / "a" / "actions.npy")
    assert a.dtype == np.float32 and np.array_equal(a, act.numpy())
    assert info["file"] == "actions.npy" and info["sampled_rows"] is None and info["shape"] == [3, 50, 12]
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 7 * 3 * 12 * 4 + 5)  # room for 7 robots' rows
    got = []
    for sub in ("b", "c"):
        info = bench.dump_outputs(str(tmp_path / sub), "actions", act)
        got.append(np.load(tmp_path / sub / "actions.npy"))
        assert info["sampled_rows"] == 7 and info["shape"] == [3, 7, 12] and info["shape_full"] == [3, 50, 12]
        assert got[-1].nbytes <= bench.DUMP_LIMIT_BYTES
    assert np.array_equal(got[0], got[1])
    rows = (got[0][0, :, 0] / 12).astype(int)  # element [0, r, 0] of `act` is 12 r
    assert len(set(rows)) == 7 and list(rows) == sorted(rows)
    assert np.array_equal(got[0], act.numpy()[:, rows, :])


def test_traffic_null_when_profile_is_stale(tmp_path, monkeypatch):
    """roofline.traffic comes from the committed --pmc summary only while the kernel
    sources are the ones it was measured on: a summary entry
    with another source digest yields None and says why."""
    sys.path.insert(0, ROOT)
    import bench
    from go2_onnx_controller_amd.provenance import kernel_source_digest
    kern = "policy_mlp_kernel<8, 1, 3, 1, 3, 4>"
    name = f"void go2pi::{kern}(go2pi::DevProgram const*, float const*, float*, int)"
    (tmp_path / "profiles").mkdir()
    summary = tmp_path / "profiles" / "pmc_summary.json"
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    for digest, want in [(kernel_source_digest(), 19.0e6), ("0123456789abcdef", None), (None, None)]:
        entry = {"hbm_bytes_per_launch": 19.0e6, "source": "rXX_mlp512_kernel_stats.csv"}
        if digest:
            entry["src_digest"] = digest
        summary.write_text(json.dumps({"workloads": {"go2_mlp_512_b4096": {name: entry}}}))
        got, note = bench.load_pmc("go2_mlp_512_b4096", kern)
        assert got == want, note
        assert ("stale" in note) == (want is None)
    assert bench.load_pmc("other_workload", kern) == (None, "no committed rocprofv3 --pmc summary of this kernel")
