"""The batched LayerNormalization pipeline without a GPU: the input condition of
tests/test_gpu_layernorm_batched.py, the models tests/ln_batched_models.py adds, the
planner's choice (tests/cpp/plan_probe.cpp through test_cpu_plan.plan) and the ln_batched
option through the C header and its Python mirror.
"""
import inspect
import os

import pytest

import ln_batched_models as lb
import ln_ref
from conftest import ROOT, SHIPPED, abs_err
from test_cpu_plan import _write, plan


@pytest.mark.parametrize("name", lb.ALL_MODELS)
def test_input_condition(tmp_path, name):
    """The parity contract is max|err| <= 1e-5 against fp64: on every (model, batch, seed,
    scale) the GPU tests feed, fp32 arithmetic alone stays under a third of it."""
    ref = ln_ref.LnRef(lb.model_path(name, tmp_path))
    assert ref.g.inputs[0][1][1] == lb.dims(name)[0]
    mine = [c for c in lb.cases() if c[0] == name]
    assert len(mine) >= len(lb.PARITY_BATCHES)
    worst = 0.0
    for _, B, seed, scale in mine:
        x = lb.obs(name, B, seed, scale)
        e = abs_err(ref.f32(x), ref.f64(x))
        worst = max(worst, e)
        assert e <= lb.TOL / 3, (name, B, seed, e)
    print(f"{name}: worst fp32-vs-fp64 error {worst:.3g} over {len(mine)} inputs")


@pytest.mark.parametrize("name", lb.ALL_MODELS)
def test_inspect_models(tmp_path, name):
    from go2_onnx_controller_amd.engine import inspect_model
    layers = inspect_model(lb.model_path(name, tmp_path))["layers"]
    assert [L["ln"] for L in layers] == lb.LN_MODES[name]
    assert [L["N"] for L in layers] == list(lb.dims(name)[1:])


def test_new_models_stay_out_of_the_registry():
    from go2_onnx_controller_amd import synth
    assert not set(lb.NEW_MODELS) & set(synth.MODELS)


@pytest.mark.parametrize("name", lb.ALL_MODELS)
def test_selection(tmp_path, name):
    p = lb.model_path(name, tmp_path)
    for bits in (2, 3):
        got = plan(p, ln_small=bits)
        assert got["batched_kernel"] == lb.KERNEL[name], (bits, got["batched_kernel"])
        # the program stays the general body's: 8 waves, no pipeline fields, layer 0 padded to 64
        assert (got["waves"], got["w4_tpw"], got["w4_plain"], got["lds"]["k0_pad"] % 64) == (8, 0, 0, 0)
    general = plan(p)["batched_kernel"]
    assert general.startswith(lb.GENERAL)
    for bits in (0, 1, 4, 7, -1):  # (outside 0 .. 3: read as 0, for both bits)
        got = plan(p, ln_small=bits)
        assert got["batched_kernel"] == general, (bits, got["batched_kernel"])
        if bits != 1:
            assert got["small_kernel"] == "gemv_layer_kernel graph", (bits, got["small_kernel"])
    assert plan(p, ln_small=3)["small_kernel"] == "policy_latency_kernel"
    assert plan(p, ln_small=1)["small_kernel"] == "policy_latency_kernel"
    assert plan(p, ln_small=2)["small_kernel"] == "gemv_layer_kernel graph"
    # small_batch = -1 (the GPU parity test): every batch takes the new kernel
    assert plan(p, ln_small=2, small_batch=-1)["small_kernel"] == lb.KERNEL[name]


def test_the_bit_changes_nothing_else_in_the_plan(tmp_path):
    """Everything the probe prints but the batched kernel's name is the same with and without
    the bit: the controller tick, the resident forms, the program's scalars, the buffers."""
    for name in lb.ALL_MODELS:
        p = lb.model_path(name, tmp_path)
        for extra in ({}, {"resident_ms": 5000}):
            a, b = plan(p, ln_small=1, **extra), plan(p, ln_small=3, **extra)
            assert a.pop("batched_kernel") != b.pop("batched_kernel")
            assert a == b, name
    p = lb.model_path("ln_ctl_post", tmp_path)
    assert plan(p, ln_small=2)["controller_kernel"] == plan(p)["controller_kernel"]
    assert plan(p, ln_small=3, resident_ms=5000)["controller_kernel"] == \
        plan(p, ln_small=1, resident_ms=5000)["controller_kernel"]


@pytest.mark.parametrize("what,args,opts", [
    ("waves", [], dict(waves=8)),
    ("no_w4", ["GO2PI_NO_W4"], {}),
    ("no_head_fuse", ["GO2PI_NO_HEAD_FUSE"], {}),
    ("obs_mean", [], dict(obs_mean=0.1)),
    ("obs_clip", [], dict(obs_clip=5.0)),
    ("action_clip", [], dict(action_clip=1)),
    ("action_tanh", [], dict(action_tanh=1)),
])
def test_fallbacks_by_option(synth_path, what, args, opts):
    p = synth_path("ln_512_pre")
    assert plan(p, ln_small=2)["batched_kernel"] == lb.KERNEL["ln_512_pre"]
    got = plan(p, *args, ln_small=2, **opts)
    want = f"policy_fused_kernel<{opts.get('waves', 8)}, 0, 0, 0, 0,"
    assert got["batched_kernel"].startswith(want), (what, got["batched_kernel"])


@pytest.mark.parametrize("name", ["gru_ln", "ln_mixed", "ln_wide_pre", "ln_post_small"])
def test_fallbacks_by_registry_shape(synth_path, name):
    """A recurrent LN policy; hidden widths that do not pad to one 64 * TPW, or to none of 128 /
    256 / 512. (ln_pre_small's 100 and 72 columns both pad to 128: served, test_selection.)"""
    p = synth_path(name)
    assert plan(p, ln_small=2)["batched_kernel"] == plan(p)["batched_kernel"]
    assert plan(p)["batched_kernel"].startswith(lb.GENERAL)


@pytest.mark.parametrize("what,kw", [
    ("an observation wider than the hidden layers", dict(dims=(200, 128, 128, 12), seed=60, layer_norm="pre")),
    ("a three-tile head", dict(dims=(48, 128, 128, 40), seed=61, layer_norm="pre")),
    ("a two-tile head at 8 tiles per wave", dict(dims=(48, 512, 512, 20), seed=62, layer_norm="post")),
    ("two hidden activations", dict(dims=(48, 128, 128, 12), seed=63, act=("Elu", "Tanh"), layer_norm="pre")),
])
def test_fallbacks_by_shape(tmp_path, what, kw):
    from go2_onnx_controller_amd import synth
    p = _write(tmp_path, "fallback", synth.mlp_model_bytes(**kw))
    assert plan(p, ln_small=2)["batched_kernel"].startswith(lb.GENERAL), what


@pytest.mark.parametrize("name,batched", [
    ("go2_mlp_512", "policy_mlp_kernel<8, 1, 3, 1, 3, 4>"),
    ("shipped", "policy_mlp_kernel<2, 1, 3, 1, 3, 4>"),
    ("go2_gru_256", "policy_gru_kernel<8, 1, 4>"),
    ("go2_lstm_256", "policy_lstm_kernel<8, 1, 4>"),
])
def test_policies_without_ln_select_what_they_selected(synth_path, name, batched):
    """tests/test_gpu_layernorm.py test_kernel_selection_unchanged's names, with the bit set."""
    p = SHIPPED if name == "shipped" else synth_path(name)
    for bits in (2, 3):
        got, base = plan(p, ln_small=bits), plan(p)
        assert got["batched_kernel"] == batched
        assert got == base


def test_header_has_both_bits():
    h = open(os.path.join(ROOT, "include", "go2pi.h")).read()
    assert "#define GO2PI_LN_SMALL 1" in h and "#define GO2PI_LN_BATCHED 2" in h
    body = h[h.index("typedef struct go2pi_opts"):h.index("} go2pi_opts;")]
    assert body.rstrip().endswith("int32_t ln_small;"), body[-200:]  # still the last field


def test_engine_accepts_the_keyword():
    """ln_batched is the last keyword, False by default, and reaches go2pi_create (which fails
    for want of a device here, or succeeds on a GPU machine): no TypeError."""
    from go2_onnx_controller_amd import Engine, Go2piError, synth
    params = inspect.signature(Engine.__init__).parameters
    assert list(params)[-1] == "ln_batched" and params["ln_batched"].default is False
    try:
        with Engine(synth.ensure_model("ln_ctl_post"), max_batch=32, ln_batched=True) as e:
            assert e.batched_kernel == lb.KERNEL["ln_ctl_post"]
    except Go2piError as ex:
        assert "no CPU fallback" in str(ex) or "GO2PI_E_DEVICE" in str(ex), str(ex)


def test_engine_sets_both_bits(monkeypatch):
    """Engine(ln_small=a, ln_batched=b) passes ln_small = a | 2 b to go2pi_create."""
    from go2_onnx_controller_amd import engine
    seen = []

    class Stop(Exception):
        pass

    real = engine.lib()

    class Spy:
        def __getattr__(self, k):
            return getattr(real, k)

        def go2pi_create(self, path, opts, out):
            seen.append(opts._obj.ln_small)
            raise Stop

    monkeypatch.setattr(engine, "lib", lambda: Spy())
    from go2_onnx_controller_amd import synth
    for a, b in ((False, False), (True, False), (False, True), (True, True)):
        with pytest.raises(Stop):
            engine.Engine(synth.ensure_model("ln_ctl_post"), ln_small=a, ln_batched=b)
    assert seen == [0, 1, 2, 3]
