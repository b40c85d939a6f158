"""GPU: residual MLP policies on the 4-wave pipeline (GO2PI_RESIDUAL_BATCHED:
policy_mlp_res_kernel<tiles per wave, head tiles>), against the float64 reference at the
project's 1e-5 and, for the integer probes, exactly. tests/test_cpu_res_batched.py checks on the
same inputs (res_batched_specs.inputs) that float32 arithmetic alone stays under a third of the
tolerance.

The carried value of this kernel lives in each lane's registers from the source layer's
epilogue to the consumer's, so beside parity the tests look at what that can get wrong: a
consumer at either epilogue site, a layer that is consumer and source, a carried value held
across layers that neither write nor read it, a second step of a device sequence, a smaller
batch behind a larger one, row shards, a NaN row, and each hidden layer's own activation.

The switch is read when an engine is created, so every test sets it first (monkeypatch
restores the environment).
"""
import os
import subprocess

import numpy as np
import pytest

import policy_specs as ps
import res_batched_specs as rb
from conftest import abs_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
SW = rb.SW
CHAIN = "gemv_layer_kernel graph"
OTHER_SWITCHES = ("GO2PI_RESIDUAL_SMALL", "GO2PI_SKIP_SMALL", "GO2PI_SMALL_CHAIN", "GO2PI_NO_W4", "GO2PI_NO_HEAD_FUSE")


def _env(monkeypatch, on=True):
    for s in OTHER_SWITCHES:
        monkeypatch.delenv(s, raising=False)
    if on:
        monkeypatch.setenv(SW, "1")
    else:
        monkeypatch.delenv(SW, raising=False)


def _engine(name, **kw):
    """An engine created under the switch (the caller has set it): the pipeline's residual kernel."""
    from go2_onnx_controller_amd import Engine
    kw.setdefault("max_batch", 128)
    e = Engine(ps.path(name), **kw)
    assert e.batched_kernel == rb.KERNEL[name], e.batched_kernel
    return e


def _check(e, name, B, k=0):
    y = e.run(ps.obs(name, B, k))
    err = abs_err(y, ps.want(name, B, k))
    print(f"{name} B={B}: abs err {err:.3g}")
    assert np.isfinite(y).all() and err <= TOL, (name, B, err)
    return y


# ---- 1. the kernel's name on the device, with and without the switch
def test_kernel_name(monkeypatch):
    from go2_onnx_controller_amd import Engine
    _env(monkeypatch, on=False)
    with Engine(ps.path("resb_t4_simba2"), max_batch=64) as e:
        assert e.batched_kernel.startswith(rb.GENERAL), e.batched_kernel
    _env(monkeypatch)
    for name in ("resb_t2_post_h2", "resb_t4_simba2", "resb_t8_v1"):
        with Engine(ps.path(name), max_batch=64) as e:
            assert e.batched_kernel == rb.KERNEL[name], e.batched_kernel
            assert e.small_kernel == CHAIN
    with Engine(ps.path("simba_64"), max_batch=64) as e:  # one tile per wave: the general body
        assert e.batched_kernel.startswith(rb.GENERAL), e.batched_kernel
        _check(e, "simba_64", 33)
    with Engine(ps.path("resb_t4_simba2"), max_batch=64, waves=8) as e:
        assert e.batched_kernel.startswith(rb.GENERAL), e.batched_kernel


# ---- 2. parity
@pytest.mark.parametrize("name", rb.NAMES)
def test_parity(name, monkeypatch):
    _env(monkeypatch)
    with _engine(name, small_batch=-1) as e:  # every batch on the pipeline
        assert e.small_kernel == rb.KERNEL[name], e.small_kernel
        for B in rb.RES_BATCHED.parity_batches:
            _check(e, name, B)
    with _engine(name) as e:  # the default small_batch: the chain up to 8, the pipeline from 9
        assert e.small_kernel == CHAIN
        for B in rb.RES_BATCHED.small_batches:
            _check(e, name, B)


# ---- 3. the hand-over: the chain, the pipeline, the chain, on one engine
@pytest.mark.parametrize("name", ["resb_t2_adjacent", "resb_t4_simba2"])
def test_handover(name, monkeypatch):
    _env(monkeypatch)
    with _engine(name) as e:
        assert e.small_kernel == CHAIN
        first = _check(e, name, 8)
        _check(e, name, 9)
        again = _check(e, name, 8)
    assert np.array_equal(first, again)


# ---- 4. the probes, exactly; the general body on the same engine options gives the same integers
@pytest.mark.parametrize("name", rb.PROBES)
def test_probes_exact(name, monkeypatch):
    _env(monkeypatch)
    got = {}
    with _engine(name, small_batch=-1) as e:
        assert e.small_kernel == rb.KERNEL[name]
        for B in rb.RES_BATCHED.probe_batches:
            x = ps.probe_obs(name, B)
            got[B] = e.run(x)
            assert np.array_equal(got[B], np.rint(got[B])), (name, B)
            assert np.array_equal(got[B].astype(np.int64), ps.probe_forward(name, x)), (name, B)
    _env(monkeypatch, on=False)
    from go2_onnx_controller_amd import Engine
    with Engine(ps.path(name), max_batch=128, small_batch=-1) as e:
        assert e.batched_kernel.startswith(rb.GENERAL), e.batched_kernel
        for B in rb.RES_BATCHED.probe_batches:
            assert np.array_equal(e.run(ps.probe_obs(name, B)), got[B]), (name, "general", B)


# ---- 5. a fresh launch at the workload's size: one workgroup per CU, and one row more
def test_fresh_launch_at_workload_size(monkeypatch):
    _env(monkeypatch)
    name = "resb_t8_simba"
    with _engine(name, max_batch=4097) as e:
        _check(e, name, 4097)


# ---- 6. shards and repeats
@pytest.mark.parametrize("name", ["resb_t4_simba2", "resb_t2_post_h2"])
def test_shards_and_repeats_bitwise(name, monkeypatch):
    _env(monkeypatch)
    x = ps.obs(name, 1024)
    with _engine(name, max_batch=1024) as e:
        full = _check(e, name, 1024)
        assert np.array_equal(e.run(x), full)
        for lo, hi in ((0, 512), (17, 530), (1000, 1024)):
            assert np.array_equal(e.run(x[lo:hi]), full[lo:hi]), (lo, hi)


# ---- 7. a device sequence: every step starts from a cleared carried value
def test_sequence_equals_single_runs(monkeypatch):
    import torch
    _env(monkeypatch)
    name, B, T = "resb_t4_far", 100, 3
    xs = np.stack([ps.obs(name, B, k) for k in range(T)])
    with _engine(name) as e:
        xd = torch.from_numpy(xs).cuda()
        seq = e.run_sequence_torch(xd)
        single = torch.stack([e.run_torch(xd[t].contiguous()) for t in range(T)])
        torch.cuda.synchronize()
    seq, single = seq.cpu().numpy(), single.cpu().numpy()
    assert np.array_equal(seq, single)
    for t in range(T):
        assert abs_err(seq[t], ps.want(name, B, t)) <= TOL
    assert not np.array_equal(seq[0], seq[1])


# ---- 8. a NaN stays in its row
def test_nan_stays_in_its_row(monkeypatch):
    _env(monkeypatch)
    name, B, r = "resb_t4_simba2", 33, 5
    x = ps.obs(name, B)
    bad = x.copy()
    bad[r, 10] = np.nan
    with _engine(name, small_batch=-1) as e:
        clean = _check(e, name, B)
        y = e.run(bad)
        after = e.run(x)
    assert np.isnan(y[r]).all(), y[r]
    keep = np.arange(B) != r
    assert np.array_equal(y[keep].view(np.uint32), clean[keep].view(np.uint32))
    assert np.array_equal(after, clean)


# ---- 9. the drop-in actors: act() at batch 1 still answers (the small path is unchanged)
def test_python_onnx_actor(monkeypatch):
    from go2_onnx_controller_amd import ONNXActor
    name = "simba_256"
    _env(monkeypatch)
    monkeypatch.delenv("GO2PI_RESIDENT_MS", raising=False)
    monkeypatch.delenv("GO2PI_LN_SMALL", raising=False)
    obs, act = np.zeros(ps.in_dim(name), np.float32), np.zeros(12, np.float32)
    actor = ONNXActor(ps.path(name), obs, act)
    assert actor.check_dims()
    assert actor._engine.batched_kernel == rb.KERNEL[name]
    assert actor._engine.small_kernel == CHAIN and actor._engine.resident_kernel.startswith("none")
    x = ps.obs(name, 8)
    for i in range(8):
        obs[:] = x[i]  # the caller writes in place, like populate_buffer
        actor.act()
        assert abs_err(act, ps.want(name, 8)[i]) <= TOL, i


def test_cpp_onnx_actor_ticks(tmp_path):
    """tests/cpp/controller_shape.cpp's "ticks" mode on simba_256 in a fresh child process under
    the switch. Its observation buffer is a Go2 controller's 98 floats; the model reads the
    first 48 (check_dims reports the mismatch, act() serves the model's own width)."""
    from test_cpu_boundary import build_controller_shape
    name = "simba_256"
    exe = build_controller_shape()
    dump, ticks = tmp_path / "actions.bin", 20
    env = {k: v for k, v in os.environ.items() if k not in OTHER_SWITCHES + ("GO2PI_LN_SMALL",)}
    env.update(GO2PI_RESIDENT_MS="100", GO2PI_RESIDUAL_BATCHED="1")
    r = subprocess.run([exe, ps.path(name), "ticks", str(ticks), str(dump)], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "check_dims: 0" in r.stdout
    got = np.fromfile(dump, np.float32).reshape(ticks, 12)
    o, seq = np.zeros(98, np.float32), np.empty((ticks, 98), np.float32)
    for t in range(ticks):
        o[t % 98] += np.float32(0.001)
        seq[t] = o
    assert abs_err(got, ps.ref(name).f64(seq[:, :48])) <= TOL
    assert not np.array_equal(got[0], got[1])


# ---- 10. the controller tick stays refused
def test_controller_step_is_refused(monkeypatch):
    from go2_onnx_controller_amd import Go2piError
    from oracle import controller_ref as cr
    _env(monkeypatch)
    name = "resb_ctl"  # a Go2 controller's I/O: 98 observations, 12 actions
    rng = np.random.default_rng(0)
    with _engine(name) as e:
        for B in (1, 33):
            st, joy = cr.synthetic_states(rng, B), cr.synthetic_joy(rng, B)
            obs, act = np.zeros((B, 98), np.float32), np.zeros((B, 12), np.float32)
            with pytest.raises(Go2piError, match="does not serve a policy with residual connections") as ex:
                e.controller_step(st, obs, act, joy=joy)
            assert ex.value.code == -1  # GO2PI_E_INVALID
        _check(e, name, 33)  # the engine still serves run()
