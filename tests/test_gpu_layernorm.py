"""GPU parity of LayerNormalization policies (ONNX opset 17) against tests/ln_ref.py.

Tolerance: abs_err <= 1e-5 against the fp64 reference (the project's parity contract),
"bitwise" where a test says so. tests/test_cpu_layernorm.py checks that fp32 arithmetic
alone stays under a third of that on every input used here (same generator calls).
"""
import functools
import os

import numpy as np
import pytest

import ln_ref
from conftest import GOLDEN, abs_err, realistic_obs, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5


@functools.lru_cache(maxsize=None)
def _ref(path):
    return ln_ref.LnRef(path)


@functools.lru_cache(maxsize=None)
def _want(path, name, B, scale=1.0, seed=None):
    """(observations, fp64 actions) of a test's batch: computed once, shared, never written."""
    ref = _ref(path)
    x = ln_ref.obs_for(name, B, ref.g.inputs[0][1][1], scale, seed)
    y = ref.f64(x)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def _check(e, x, want, what):
    y = e.run(x)
    err = abs_err(y, want)
    print(f"{what}: abs err {err:.3g}")
    assert np.all(np.isfinite(y)) and err <= TOL, (what, err)


# 1. parity, default options (B <= 8: the GEMV chain by graph replay; above: the general body).
# Beside the five models of the issue, ln_wide_pre: 600 columns, the LN pass's path for rows
# wider than the 512 columns it keeps in registers.
@pytest.mark.parametrize("name", ln_ref.MLP_MODELS)
def test_parity(synth_path, name):
    from go2_onnx_controller_amd import Engine
    p = synth_path(name)
    with Engine(p, max_batch=128) as e:
        assert e.batched_kernel.startswith("policy_fused_kernel<8, 0, 0, 0, 0,"), e.batched_kernel
        assert e.resident_kernel == "none"
        for B in ln_ref.PARITY_BATCHES:
            x, want = _want(p, name, B)
            _check(e, x, want, f"{name} B={B}")


def test_parity_realistic_observations(synth_path):
    """The controller's observation layout (conftest.realistic_obs) through ln_ctl_post."""
    from go2_onnx_controller_amd import Engine
    p = synth_path("ln_ctl_post")
    x = realistic_obs(64)
    with Engine(p, max_batch=64) as e:
        _check(e, x, _ref(p).f64(x), "ln_ctl_post realistic B=64")
        _check(e, x[:3], _ref(p).f64(x[:3]), "ln_ctl_post realistic B=3")


# 2. + 6. every workgroup shape of the general body (batches <= 8 included) and the chain,
# on the model with the padded Sigmoid + post-LN layer (200 of 256 columns)
@pytest.mark.parametrize("small_batch", [-1, 8])
@pytest.mark.parametrize("waves", [4, 8, 16])
def test_kernel_variants(synth_path, waves, small_batch):
    from go2_onnx_controller_amd import Engine
    p = synth_path("ln_mixed")
    with Engine(p, max_batch=64, waves=waves, small_batch=small_batch) as e:
        assert e.batched_kernel.startswith(f"policy_fused_kernel<{waves}, 0, 0, 0, 0,"), e.batched_kernel
        for B in (1, 3, 8, 40):
            x, want = _want(p, "ln_mixed", B, 1.0, 50 + B)
            _check(e, x, want, f"ln_mixed waves={waves} small_batch={small_batch} B={B}")


# 3. the workload's shape: one workgroup per CU, and one row more
def test_workload_shape(synth_path):
    from go2_onnx_controller_amd import Engine
    p = synth_path("ln_512_pre")
    x, want = _want(p, "ln_512_pre", 4097)
    with Engine(p, max_batch=8192) as e:
        assert e.batched_kernel.startswith("policy_fused_kernel<8, 0, 0, 0, 0,"), e.batched_kernel
        _check(e, x[:4096], want[:4096], "ln_512_pre B=4096")
        _check(e, x, want, "ln_512_pre B=4097")
        c = e.cost
        assert c["flops_per_row"] == 2.0 * (48 * 512 + 2 * 512 * 512 + 512 * 12)
        assert c["weight_bytes"] == 4.0 * (48 * 512 + 2 * 512 * 512 + 512 * 12 + 3 * 512 + 12 + 3 * 2 * 512)


# 4. shards of a batch and repeats are bitwise the full batch
def test_shards_and_repeats_bitwise(synth_path):
    from go2_onnx_controller_amd import Engine
    p = synth_path("ln_512_pre")
    x, want = _want(p, "ln_512_pre", 1024)
    with Engine(p, max_batch=1024) as e:
        full = e.run(x)
        assert abs_err(full, want) <= TOL
        assert np.array_equal(e.run(x), full)
        for lo, hi in ((0, 512), (17, 530), (1000, 1024)):
            assert np.array_equal(e.run(x[lo:hi]), full[lo:hi]), (lo, hi)


# 5. known answers
@pytest.mark.parametrize("B", [1, 20])
def test_zero_variance_layer(tmp_path, B):
    """Layer 0: zero weights, a constant bias, then a pre-LN. The variance is exactly 0, so
    the layer's output is its LN bias and the action is W2 . b_ln + b2 for any observation."""
    from go2_onnx_controller_amd import Engine, onnx_writer as ow
    rng = np.random.default_rng(3)
    N = 72
    g = rng.uniform(0.75, 1.25, N).astype(np.float32)
    b_ln = rng.uniform(-0.25, 0.25, N).astype(np.float32)
    W2 = (rng.standard_normal((5, N)) / 8).astype(np.float32)
    b2 = rng.standard_normal(5).astype(np.float32)
    inits = [("w0", np.zeros((N, 10), np.float32)), ("b0", np.full(N, 0.625, np.float32)), ("g", g), ("c", b_ln),
             ("w2", W2), ("b2", b2)]
    nodes = [ow.node("Gemm", ["observation", "w0", "b0"], ["a"], "g0", [ow.attr_int("transB", 1)]),
             ow.node("LayerNormalization", ["a", "g", "c"], ["n"], "ln", [ow.attr_int("axis", -1)]),
             ow.node("Gemm", ["n", "w2", "b2"], ["action"], "g1", [ow.attr_int("transB", 1)])]
    model = ow.model(nodes, inits, [("observation", ["batch", 10])], [("action", ["batch", 5])])
    want = W2.astype(np.float64) @ b_ln.astype(np.float64) + b2
    x = (rng.standard_normal((B, 10)) * 10).astype(np.float32)
    with Engine(model, max_batch=32) as e:
        y = e.run(x)
    assert abs_err(y, np.tile(want, (B, 1))) <= TOL
    assert np.array_equal(y, np.tile(y[:1], (B, 1)))  # independent of the observation, bitwise


def test_epsilon_attribute(synth_path):
    """ln_mixed's last LN has epsilon 1e-3; inputs scaled by 1e-2 keep the variances small
    enough that epsilon decides the result: a kernel with 1e-5 built in misses by far more
    than the tolerance (checked against the reference evaluated with that epsilon)."""
    from go2_onnx_controller_amd import Engine
    p = synth_path("ln_mixed")
    x, want = _want(p, "ln_mixed", 20, 1e-2, 77)
    g = ln_ref.onnx_ref.load(p)
    for nd in g.nodes:
        if nd.op_type == "LayerNormalization":
            nd.attrs["epsilon"] = 1e-5
    wrong = ln_ref.run(g, {"observation": x})["action"]
    assert abs_err(wrong, want) > 100 * TOL  # the case can tell the two apart
    with Engine(p, max_batch=32) as e:
        _check(e, x, want, "ln_mixed epsilon B=20")
        _check(e, x[:2], want[:2], "ln_mixed epsilon B=2")


@pytest.mark.parametrize("name", ["ln_pre_small", "ln_mixed"])
def test_golden_fixture(synth_path, name):
    from go2_onnx_controller_amd import Engine
    fx = np.load(os.path.join(GOLDEN, "golden_ln.npz"))
    x, want = fx[f"{name}_x"], fx[f"{name}_y"]
    with Engine(synth_path(name), max_batch=32) as e:
        _check(e, x, want, f"{name} golden B=24")
        _check(e, x[:8], want[:8], f"{name} golden B=8")


# 7. controller tick (the general body's policy_fused_ctl_kernel), as tests/test_gpu_controller.py
# checks dense policies: bit-identical observation rows, actions within the policy tolerance
@pytest.mark.parametrize("B", [1, 8, 33])
def test_controller_tick(synth_path, B):
    from go2_onnx_controller_amd import Engine
    from oracle import controller_ref as cr
    p = synth_path("ln_ctl_post")
    ref = _ref(p)
    with Engine(p, max_batch=64) as e:
        assert e.ctl_history() == 2
        obs = np.zeros((B, e.in_dim), np.float32)
        act = np.zeros((B, 12), np.float32)
        for st, joy in ln_ref.ctl_inputs(B, 3):
            o0, a0 = obs.copy(), act.copy()
            q_des, kp, kd, status = e.controller_step(st, obs, act, joy=joy)
            want_obs, a_ref, _, kp_ref, kd_ref, want_status = cr.tick(ref.f64, st, joy, o0, a0, 2)
            assert np.array_equal(obs, want_obs, equal_nan=True), np.argwhere(obs != want_obs)[:5]
            assert rel_err(act, a_ref) <= TOL
            p0 = cr.default_params()
            assert np.array_equal(q_des, np.asarray(p0["q0"])[None] + act.astype(np.float64) * p0["action_scale"])
            assert np.array_equal(kp, kp_ref) and np.array_equal(kd, kd_ref)
            assert np.array_equal(status, want_status)


# 8. recurrent: the generic GRU cell in front of a pre-LN head
@pytest.mark.parametrize("B", [1, 20])
def test_recurrent(synth_path, B):
    from go2_onnx_controller_amd import Engine
    p = synth_path("gru_ln")
    xs = ln_ref.obs_for("gru_ln", 5 * B, 10).reshape(5, B, 10)
    want_y, want_h = _ref(p).rollout(xs, np.zeros((B, 32)))
    with Engine(p, max_batch=32) as e:
        assert e.batched_kernel.startswith("policy_fused_kernel<8, 0, 0, 0, 0,"), e.batched_kernel
        e.reset_hidden()
        for t in range(5):
            assert abs_err(e.run(xs[t]), want_y[t]) <= TOL, t
        assert abs_err(e.get_hidden(B), want_h) <= TOL


# 9. the drop-in default: resident_ms > 0 as ONNXActor sets it; LN policies take the graph replay
def test_drop_in_default_fresh_input_each_replay(synth_path):
    from go2_onnx_controller_amd import Engine
    p = synth_path("ln_pre_small")
    with Engine(p, resident_ms=100) as e:
        assert e.resident_kernel == "none"
        outs = []
        for i in range(3):
            x, want = _want(p, "ln_pre_small", 1, 1.0, 90 + i)
            _check(e, x, want, f"ln_pre_small drop-in call {i}")
            outs.append(e.run(x))
        assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])
        assert e.resident_launches == 0


# 10. a sequence launch equals its single steps, bitwise
def test_sequence_equals_single_steps(synth_path):
    import torch
    from go2_onnx_controller_amd import Engine
    p = synth_path("ln_pre_small")
    x, want = _want(p, "ln_pre_small", 300, 1.0, 95)
    with Engine(p, max_batch=128) as e:
        obs = torch.from_numpy(x.reshape(3, 100, -1).copy()).cuda()
        seq = e.run_sequence_torch(obs)
        steps = torch.stack([e.run_torch(obs[t]) for t in range(3)])
        torch.cuda.synchronize()
        assert torch.equal(seq, steps)
        assert abs_err(seq.cpu().numpy().reshape(300, -1), want) <= TOL


# programs without LayerNormalization select what they selected before it existed
# (the names the parent commit's library reports for the same models)
@pytest.mark.parametrize("name,batched,resident", [
    ("go2_mlp_512", "policy_mlp_kernel<8, 1, 3, 1, 3, 4>", "policy_wide_kernel<4, 8, 12, 0>"),
    ("shipped", "policy_mlp_kernel<2, 1, 3, 1, 3, 4>", "policy_act1_kernel"),
    ("go2_gru_256", "policy_gru_kernel<8, 1, 4>", "policy_resident_kernel"),
    ("go2_lstm_256", "policy_lstm_kernel<8, 1, 4>", "policy_resident_kernel"),
])
def test_kernel_selection_unchanged(synth_path, shipped_path, name, batched, resident):
    from go2_onnx_controller_amd import Engine
    p = shipped_path if name == "shipped" else synth_path(name)
    with Engine(p, max_batch=64) as e:
        assert e.batched_kernel == batched and e.resident_kernel == "none"
    with Engine(p, max_batch=64, resident_ms=100) as e:
        assert e.batched_kernel == batched
        kernel, ring = e.resident_kernel.split(" ring=")
        if name == "go2_mlp_512" and ring == "host":  # the wide kernel polls a request ring in device memory
            resident = "policy_resident_kernel"
        assert kernel == resident, e.resident_kernel
