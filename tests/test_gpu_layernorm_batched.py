"""GPU: dense LayerNormalization policies on the 4-wave pipeline's LN kernel
(Engine(ln_batched=True): policy_mlp_ln_kernel<tiles per wave, head tiles>) against
tests/ln_ref.py.

Tolerance: abs_err <= 1e-5 against the fp64 reference (the project's parity contract),
"bitwise" where a test says so. tests/test_cpu_layernorm_batched.py checks that fp32
arithmetic alone stays under a third of that on every input used here
(tests/ln_batched_models.py cases(): the same generator calls).
"""
import functools

import numpy as np
import pytest

import ln_batched_models as lb
import ln_ref
from conftest import abs_err

pytestmark = pytest.mark.gpu

TOL = lb.TOL


@functools.lru_cache(maxsize=None)
def _ref(path):
    return ln_ref.LnRef(path)


@functools.lru_cache(maxsize=None)
def _want(path, name, B, seed=None, scale=1.0):
    """(observations, fp64 actions) of a test's batch: computed once, shared, never written."""
    x = lb.obs(name, B, seed, scale)
    y = _ref(path).f64(x)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def _check(e, x, want, what):
    y = e.run(x)
    err = abs_err(y, want)
    print(f"{what}: abs err {err:.3g}")
    assert np.all(np.isfinite(y)) and err <= TOL, (what, err)
    return y


# 1. parity at the tile edge and a partial tile, every batch on the new kernel; and
# 8. the same inputs on an engine without the bit (the general body) agree within 2 TOL
@pytest.mark.parametrize("name", lb.ALL_MODELS)
def test_parity(tmp_path, name):
    from go2_onnx_controller_amd import Engine
    p = lb.model_path(name, tmp_path)
    got = {}
    with Engine(p, max_batch=64, small_batch=-1, ln_batched=True) as e:
        assert e.batched_kernel == lb.KERNEL[name], e.batched_kernel
        assert e.small_kernel == lb.KERNEL[name], e.small_kernel
        for B in lb.PARITY_BATCHES:
            x, want = _want(p, name, B)
            got[B] = _check(e, x, want, f"{name} B={B}")
    with Engine(p, max_batch=64, small_batch=-1) as e:
        assert e.batched_kernel.startswith(lb.GENERAL), e.batched_kernel
        for B in lb.PARITY_BATCHES:
            x, _ = _want(p, name, B)
            d = abs_err(e.run(x), got[B])
            print(f"{name} B={B}: against the general body {d:.3g}")
            assert d <= 2 * TOL, (name, B, d)


# 2. the hand-over from the small-batch paths with both bits
@pytest.mark.parametrize("name", lb.HANDOVER_MODELS)
def test_handover(tmp_path, name):
    import torch
    from go2_onnx_controller_amd import Engine
    p = lb.model_path(name, tmp_path)
    with Engine(p, max_batch=64, ln_small=True, ln_batched=True) as e:
        assert e.batched_kernel == lb.KERNEL[name] and e.small_kernel == "policy_latency_kernel"
        for B in (8, 9):
            x, want = _want(p, name, B)
            _check(e, x, want, f"{name} hand-over B={B}")
        # run_torch has no small-batch path: the batched kernel at batch 3
        x, want = _want(p, name, 3)
        y = e.run_torch(torch.from_numpy(x.copy()).cuda()).cpu().numpy()
        assert abs_err(y, want) <= TOL


# 3. the workload's shape: one workgroup per CU, and one row more
def test_workload_shape(synth_path):
    from go2_onnx_controller_amd import Engine
    p = synth_path("ln_512_pre")
    x, want = _want(p, "ln_512_pre", lb.WORKLOAD_ROWS)
    with Engine(p, max_batch=8192, ln_batched=True) as e:
        assert e.batched_kernel == lb.KERNEL["ln_512_pre"]
        _check(e, x[:4096], want[:4096], "ln_512_pre B=4096")
        _check(e, x, want, "ln_512_pre B=4097")


# 4. bitwise determinism: repeats, row shards, a device-side sequence
@pytest.mark.parametrize("name", lb.SHARD_MODELS)
def test_shards_and_repeats_bitwise(tmp_path, name):
    from go2_onnx_controller_amd import Engine
    p = lb.model_path(name, tmp_path)
    x, want = _want(p, name, lb.SHARD_ROWS)
    with Engine(p, max_batch=lb.SHARD_ROWS, ln_batched=True) as e:
        assert e.batched_kernel == lb.KERNEL[name]
        full = _check(e, x, want, f"{name} B={lb.SHARD_ROWS}")
        assert np.array_equal(e.run(x), full)
        for lo, hi in lb.SHARDS:
            assert np.array_equal(e.run(x[lo:hi]), full[lo:hi]), (lo, hi)


def test_sequence_equals_single_steps(tmp_path):
    import torch
    from go2_onnx_controller_amd import Engine
    name, T, R = lb.SEQ_MODEL, lb.SEQ_STEPS, lb.SEQ_ROWS
    p = lb.model_path(name, tmp_path)
    x, want = _want(p, name, T * R)
    with Engine(p, max_batch=128, ln_batched=True) as e:
        assert e.batched_kernel == lb.KERNEL[name]
        obs = torch.from_numpy(x.reshape(T, R, -1).copy()).cuda()
        seq = e.run_sequence_torch(obs)
        steps = torch.stack([e.run_torch(obs[t]) for t in range(T)])
        torch.cuda.synchronize()
        assert torch.equal(seq, steps)
        assert abs_err(seq.cpu().numpy().reshape(T * R, -1), want) <= TOL


# 5. known answer: a layer of exactly zero variance
@pytest.mark.parametrize("B", [1, 20])
def test_zero_variance_layer(B):
    from go2_onnx_controller_amd import Engine
    model, want = lb.zero_variance_model()
    x = (np.random.default_rng(3 + B).standard_normal((B, 10)) * 10).astype(np.float32)
    with Engine(model, max_batch=32, small_batch=-1, ln_batched=True) as e:
        assert e.batched_kernel == "policy_mlp_ln_kernel<2, 1>", e.batched_kernel
        y = e.run(x)
    assert abs_err(y, np.tile(want, (B, 1))) <= TOL
    assert np.array_equal(y, np.tile(y[:1], (B, 1)))  # independent of the observation, bitwise


# 6. the epsilon of each layer
def test_epsilon_attribute(tmp_path):
    """lnb_t8_eps's second LN has epsilon 1e-3; inputs scaled by 1e-2 keep the variances small
    enough that epsilon decides the result: a kernel with 1e-5 built in (or the first layer's)
    misses by far more than the tolerance."""
    from go2_onnx_controller_amd import Engine
    name = lb.EPS_MODEL
    p = lb.model_path(name, tmp_path)
    x, want = _want(p, name, lb.EPS_ROWS, lb.EPS_SEED, lb.EPS_SCALE)
    g = ln_ref.onnx_ref.load(p)
    for nd in g.nodes:
        if nd.op_type == "LayerNormalization":
            nd.attrs["epsilon"] = 1e-5
    wrong = ln_ref.run(g, {g.inputs[0][0]: x})[g.outputs[0][0]]
    print(f"{name}: epsilon 1e-5 everywhere differs by {abs_err(wrong, want):.3g}")
    assert abs_err(wrong, want) > 100 * TOL  # the case can tell the two apart
    with Engine(p, max_batch=32, small_batch=-1, ln_batched=True) as e:
        assert e.batched_kernel == lb.KERNEL[name]
        _check(e, x, want, f"{name} epsilon B={lb.EPS_ROWS}")


# 7. a NaN stays in its row
def test_nan_stays_in_its_row(tmp_path):
    from go2_onnx_controller_amd import Engine
    name, B, r = lb.NAN_MODEL, lb.NAN_ROWS, lb.NAN_ROW
    p = lb.model_path(name, tmp_path)
    x, want = _want(p, name, B)
    bad = x.copy()
    bad[r, 7] = np.nan
    with Engine(p, max_batch=64, small_batch=-1, ln_batched=True) as e:
        assert e.batched_kernel == lb.KERNEL[name]
        clean = _check(e, x, want, f"{name} B={B}")
        y = e.run(bad)
    assert np.all(np.isnan(y[r]))
    others = np.arange(B) != r
    assert np.array_equal(y[others], clean[others])
