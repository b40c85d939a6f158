"""LayerNormalization policies on the small-batch kernels, without a GPU: the input
condition of tests/test_gpu_layernorm_small.py, the three models tests/ln_small_models.py
adds, and the ln_small option through the C ABI and its Python mirror.
"""
import ctypes
import inspect

import numpy as np
import pytest

import ln_ref
import ln_small_models as lm
from conftest import abs_err


@pytest.mark.parametrize("name", lm.ALL_MODELS)
def test_input_condition(tmp_path, name):
    """The parity contract is max|err| <= 1e-5 against fp64: on every (model, batch, seed)
    the GPU tests feed, fp32 arithmetic alone stays under a third of it."""
    ref = ln_ref.LnRef(lm.model_path(name, tmp_path))
    assert ref.g.inputs[0][1][1] == lm.in_dim(name)
    mine = [c for c in lm.cases() if c[0] == name]
    assert len(mine) >= len(lm.LAUNCH_BATCHES) + lm.RESIDENT_REQUESTS
    worst = 0.0
    for _, B, seed in mine:
        x = lm.obs(name, B, seed)
        e = abs_err(ref.f32(x), ref.f64(x))
        worst = max(worst, e)
        assert e <= 1e-5 / 3, (name, B, seed, e)
    print(f"{name}: worst fp32-vs-fp64 error {worst:.3g} over {len(mine)} inputs")


def test_input_condition_drop_in(synth_path):
    """The drop-in test's observations (tests/cpp/controller_shape.cpp: "twos", and its
    "ticks" sequence) meet the same condition on ln_ctl_post."""
    ref = ln_ref.LnRef(synth_path("ln_ctl_post"))
    for x in (np.full((1, 98), 2, np.float32), lm.dropin_observations()):
        assert abs_err(ref.f32(x), ref.f64(x)) <= 1e-5 / 3


def test_input_condition_plain_wide():
    from go2_onnx_controller_amd import synth
    ref = ln_ref.LnRef(synth.mlp_model_bytes(**lm.PLAIN_WIDE))
    for B in (6, 7, 8):
        x = lm.plain_wide_obs(B)
        assert abs_err(ref.f32(x), ref.f64(x)) <= 1e-5 / 3


def test_resident_batches_cover_one_to_eight():
    bs = lm.resident_batches()
    assert len(bs) == lm.RESIDENT_REQUESTS and sorted(set(bs)) == list(range(1, 9))
    assert any(a != b for a, b in zip(bs, bs[1:]))


@pytest.mark.parametrize("name", list(lm.NEW_MODELS))
def test_inspect_new_models(tmp_path, name):
    from go2_onnx_controller_amd.engine import inspect_model
    kw, want = lm.NEW_MODELS[name]
    layers = inspect_model(lm.model_path(name, tmp_path))["layers"]
    assert [L["ln"] for L in layers] == want
    assert [L["N"] for L in layers] == list(kw["dims"][1:])


def test_new_models_stay_out_of_the_registry():
    """tests/golden/make_golden.py hashes synth.MODELS: the new models live in the tests."""
    from go2_onnx_controller_amd import synth
    assert not set(lm.NEW_MODELS) & set(synth.MODELS)
    assert set(lm.REGISTRY_MODELS) <= set(synth.MODELS)
    assert set(lm.REGISTRY_MODELS) == set(ln_ref.MLP_MODELS)


def test_opts_have_ln_small_default_off():
    from go2_onnx_controller_amd.engine import Opts, lib
    assert Opts._fields_[-1] == ("ln_small", ctypes.c_int32)
    assert Opts.ln_small.offset == Opts.resident_ms.offset + 4
    o = Opts()
    o.ln_small = 7
    lib().go2pi_default_opts(ctypes.byref(o))
    assert o.ln_small == 0 and o.resident_ms == 0
    assert o.struct_size == ctypes.sizeof(Opts)


def test_header_declares_the_field_and_the_call():
    import os
    from conftest import ROOT
    h = open(os.path.join(ROOT, "include", "go2pi.h")).read()
    body = h[h.index("typedef struct go2pi_opts"):h.index("} go2pi_opts;")]
    assert body.rstrip().endswith("int32_t ln_small;"), body[-200:]  # the last field
    assert "int go2pi_small_kernel(const go2pi_engine *e, char *buf, size_t cap);" in h
    from go2_onnx_controller_amd.engine import lib
    assert hasattr(lib(), "go2pi_small_kernel")


def test_engine_accepts_the_keyword():
    """The keyword reaches go2pi_create (which then fails for want of a device here, or
    succeeds on a GPU machine): no TypeError, and False is the default."""
    from go2_onnx_controller_amd import Engine, Go2piError, synth
    assert inspect.signature(Engine.__init__).parameters["ln_small"].default is False
    try:
        with Engine(synth.ensure_model("ln_pre_small"), max_batch=8, ln_small=True) as e:
            assert e.small_kernel == "policy_latency_kernel"
    except Go2piError as ex:
        assert "no CPU fallback" in str(ex) or "GO2PI_E_DEVICE" in str(ex), str(ex)


def test_actor_reads_the_environment(monkeypatch):
    """actor.py turns ln_small on for GO2PI_LN_SMALL=1 only, as it reads GO2PI_RESIDENT_MS."""
    from go2_onnx_controller_amd import actor
    seen = {}

    class FakeEngine:
        inputs = [("observation", [1, 4])]
        outputs = [("action", [1, 2])]
        in_dim, out_dim = 4, 2

        def __init__(self, path, **kw):
            seen.update(kw)

    monkeypatch.setattr(actor, "Engine", FakeEngine)
    obs, act = np.zeros(4, np.float32), np.zeros(2, np.float32)
    for env, want in ((None, False), ("0", False), ("1", True)):
        if env is None:
            monkeypatch.delenv("GO2PI_LN_SMALL", raising=False)
        else:
            monkeypatch.setenv("GO2PI_LN_SMALL", env)
        seen.clear()
        actor.ONNXActor("m.onnx", obs, act)
        assert seen["ln_small"] is want, (env, seen)
