"""GPU: LayerNormalization policies at batch <= 8 on the single-launch kernel and the
resident kernels (Engine(ln_small=True)), against tests/ln_ref.py.

Tolerance: abs_err <= 1e-5 against the fp64 reference (the project's parity contract),
"bitwise" where a test says so. tests/test_cpu_layernorm_small.py checks that fp32
arithmetic alone stays under a third of that on every input used here
(tests/ln_small_models.py: the same generator calls).
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import ln_ref
import ln_small_models as lm
from conftest import abs_err, rel_err
from test_cpu_boundary import build_controller_shape

pytestmark = pytest.mark.gpu

TOL = 1e-5
RES_MS = 5000


@functools.lru_cache(maxsize=None)
def _ref(path):
    return ln_ref.LnRef(path)


@functools.lru_cache(maxsize=None)
def _want(path, name, B, seed):
    """(observations, fp64 actions) of one input: computed once, shared, never written."""
    x = lm.obs(name, B, seed)
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


# ---- 1. selection
@pytest.mark.parametrize("name", lm.ALL_MODELS)
def test_selection(tmp_path, name):
    from go2_onnx_controller_amd import Engine
    p = lm.model_path(name, tmp_path)
    with Engine(p, max_batch=64, ln_small=True) as e:
        assert e.small_kernel == "policy_latency_kernel"
        assert e.resident_kernel == "none"
        assert e.batched_kernel.startswith("policy_fused_kernel<8, 0, 0, 0, 0,"), e.batched_kernel
    with Engine(p, max_batch=64, ln_small=True, resident_ms=RES_MS) as e:
        assert e.small_kernel == "policy_latency_kernel"
        assert e.resident_kernel.startswith(lm.RESIDENT_FORM[name] + " ring="), e.resident_kernel
    for res in (0, RES_MS):
        with Engine(p, max_batch=64, resident_ms=res) as e:  # ln_small off: what the parent commit ran
            assert e.small_kernel == "gemv_layer_kernel graph", e.small_kernel
            assert e.resident_kernel == "none"
    with Engine(p, max_batch=64, use_graph=False) as e:
        assert e.small_kernel == "gemv_layer_kernel"
    with Engine(p, max_batch=64, small_batch=-1, ln_small=True) as e:
        assert e.small_kernel == e.batched_kernel


@pytest.mark.parametrize("env", ["GO2PI_RES_MULTI", "GO2PI_RES_R1W"])
def test_selection_never_the_r04_or_wide_kernel(synth_path, env, monkeypatch):
    """GO2PI_RES_MULTI=1 and GO2PI_RES_R1W=1 both put an act1-shaped LN policy on the
    multi-workgroup kernel (never policy_resident1_kernel), and the 512-wide one is never
    on policy_wide_kernel."""
    from go2_onnx_controller_amd import Engine
    monkeypatch.setenv(env, "1")  # read at engine creation
    for name in ("ln_ctl_post", "ln_pre_small", "ln_512_pre"):
        with Engine(synth_path(name), max_batch=8, ln_small=True, resident_ms=RES_MS) as e:
            assert e.resident_kernel.startswith("policy_resident_kernel ring="), (name, e.resident_kernel)


def test_selection_act1_shape_left_to_the_multi_workgroup_form(tmp_path):
    """200 -> 128^2 -> 12 is an act1 shape (<3, 128, 4>) whose LN form would spill registers
    to scratch: an LN policy of that shape takes the multi-workgroup kernel."""
    from go2_onnx_controller_amd import Engine, synth
    p = tmp_path / "m.onnx"
    p.write_bytes(synth.mlp_model_bytes((200, 128, 128, 12), seed=43, layer_norm="pre"))
    with Engine(str(p), max_batch=8, ln_small=True, resident_ms=RES_MS) as e:
        assert e.resident_kernel.startswith("policy_resident_kernel ring="), e.resident_kernel
        assert e.small_kernel == "policy_latency_kernel"


@pytest.mark.parametrize("name", ["shipped", "go2_mlp_512", "go2_gru_256", "go2_lstm_256"])
def test_selection_of_policies_without_ln_unchanged(synth_path, shipped_path, name):
    from go2_onnx_controller_amd import Engine
    p = shipped_path if name == "shipped" else synth_path(name)
    for res in (0, 100):
        with Engine(p, max_batch=64, resident_ms=res) as a, Engine(p, max_batch=64, resident_ms=res, ln_small=True) as b:
            assert (a.batched_kernel, a.resident_kernel, a.small_kernel) == \
                   (b.batched_kernel, b.resident_kernel, b.small_kernel)
            recurrent = name in ("go2_gru_256", "go2_lstm_256")
            assert a.small_kernel == (a.batched_kernel if recurrent else "policy_latency_kernel")


def test_recurrent_ln_policy_keeps_the_general_body(synth_path):
    from go2_onnx_controller_amd import Engine
    with Engine(synth_path("gru_ln"), max_batch=32, ln_small=True, resident_ms=RES_MS) as e:
        assert e.resident_kernel == "none"
        assert e.small_kernel == e.batched_kernel and e.batched_kernel.startswith("policy_fused_kernel<8,")


# ---- 2. the single launch, and the hand-over to the batched body above batch 8
@pytest.mark.parametrize("name", lm.ALL_MODELS)
def test_single_launch(tmp_path, name):
    from go2_onnx_controller_amd import Engine
    p = lm.model_path(name, tmp_path)
    with Engine(p, max_batch=64, ln_small=True) as e:
        assert e.small_kernel == "policy_latency_kernel"
        for B in lm.LAUNCH_BATCHES:
            x, want = _want(p, name, B, lm.launch_seed(name, B))
            _check(e, x, want, f"{name} single launch B={B}")
        assert e.resident_launches == 0


@pytest.mark.parametrize("res", [0, RES_MS])
def test_layer_wider_than_512_at_batch_8_without_ln(res):
    """24 -> 600 -> 8 without LN: at batch 7 and 8 layer 1's input rows are more than the
    4096 granules the eight waves sweep in one round (single launch and multi-workgroup
    resident kernel alike)."""
    from go2_onnx_controller_amd import Engine, synth
    model = synth.mlp_model_bytes(**lm.PLAIN_WIDE)
    ref = ln_ref.LnRef(model)
    with Engine(model, max_batch=8, resident_ms=res) as e:
        assert e.small_kernel == "policy_latency_kernel"
        assert e.resident_kernel.startswith("policy_resident_kernel" if res else "none")
        for B in (6, 7, 8):
            x = lm.plain_wide_obs(B)
            _check(e, x, ref.f64(x), f"plain 600-wide resident_ms={res} B={B}")
        assert e.resident_launches == (1 if res else 0)


# ---- 3. the resident kernels, each form
def _resident_run(e, p, name, form):
    for i, B in enumerate(lm.resident_batches()):
        x, want = _want(p, name, B, lm.resident_seed(name, i))
        _check(e, x, want, f"{name} {form} request {i} B={B}")
    # one launch served them all: a kernel that gives up on every request still answers
    # right through a relaunch per call (tests/test_gpu_resident.py test_resident_kernel_stays_live)
    assert e.resident_launches == 1, e.resident_launches


@pytest.mark.parametrize("name", lm.ALL_MODELS)
def test_resident_default_form(tmp_path, name):
    from go2_onnx_controller_amd import Engine
    p = lm.model_path(name, tmp_path)
    with Engine(p, max_batch=8, ln_small=True, resident_ms=RES_MS) as e:
        assert e.resident_kernel.startswith(lm.RESIDENT_FORM[name]), e.resident_kernel
        _resident_run(e, p, name, "resident")


@pytest.mark.parametrize("name,env", [
    ("ln_ctl_post", "GO2PI_RES_MULTI"),   # multi-workgroup LOCAL0, NF = 8
    ("ln_pre_small", "GO2PI_RES_MULTI"),  # multi-workgroup, tiled layer 0
    ("ln_pre_small", "GO2PI_REQ_HOST"),   # act1, the request ring in pinned host memory
    ("ln_mixed", "GO2PI_REQ_HOST"),       # multi-workgroup, the same
    ("ln_pre_small", "GO2PI_A1_DEPTH"),   # act1 under the poll-depth switch (the generic shapes fix their depth)
])
def test_resident_other_forms(synth_path, name, env, monkeypatch):
    from go2_onnx_controller_amd import Engine
    monkeypatch.setenv(env, "1")  # read at engine creation
    p = synth_path(name)
    with Engine(p, max_batch=8, ln_small=True, resident_ms=RES_MS) as e:
        kernel, ring = e.resident_kernel.split(" ring=")
        assert kernel == ("policy_resident_kernel" if env == "GO2PI_RES_MULTI" else lm.RESIDENT_FORM[name])
        if env == "GO2PI_REQ_HOST":
            assert ring == "host"
        _resident_run(e, p, name, env)


# ---- 4. the multi-workgroup form with a tiled layer 0 is the single launch, bit for bit:
# both run latency_body's per-output order, and the LN pass adds no difference of its own
@pytest.mark.parametrize("name", lm.BITWISE_MODELS)
def test_resident_tiled0_bitwise_equals_single_launch(synth_path, name, monkeypatch):
    from go2_onnx_controller_amd import Engine
    monkeypatch.setenv("GO2PI_RES_MULTI", "1")   # read at engine creation
    monkeypatch.setenv("GO2PI_RES_TILED0", "1")  # read at engine creation
    p = synth_path(name)
    with Engine(p, max_batch=8, ln_small=True, resident_ms=RES_MS) as r, Engine(p, max_batch=8, ln_small=True) as s:
        assert r.resident_kernel.startswith("policy_resident_kernel") and s.small_kernel == "policy_latency_kernel"
        for B in lm.BITWISE_BATCHES:
            x, want = _want(p, name, B, lm.bitwise_seed(name, B))
            yr = _check(r, x, want, f"{name} tiled0 resident B={B}")
            ys = _check(s, x, want, f"{name} single launch B={B}")
            assert np.array_equal(yr, ys), (name, B, abs_err(yr, ys))
        assert r.resident_launches == 1 and s.resident_launches == 0


# ---- 5. NaN rows and a zero-variance layer
FORMS = {"launch": (0, None), "act1": (RES_MS, None), "multi": (RES_MS, "GO2PI_RES_MULTI")}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["ln_pre_small", "ln_512_pre"])
def test_nan_row_stays_in_its_row(synth_path, name, form, monkeypatch):
    """A NaN observation row gives a NaN action row; the other rows stay within tolerance.
    (Elu policies: both pass a NaN on. ln_512_pre has no act1 form: its "act1" case is the
    multi-workgroup kernel with a local layer 0, "multi" the same kernel again.)"""
    from go2_onnx_controller_amd import Engine
    res, env = FORMS[form]
    if env:
        monkeypatch.setenv(env, "1")
    p = synth_path(name)
    x, want = _want(p, name, 5, lm.launch_seed(name, 5))
    x = x.copy()
    x[2, 3] = np.nan
    with Engine(p, max_batch=8, ln_small=True, resident_ms=res) as e:
        for _ in range(2):
            y = e.run(x)
            assert np.all(np.isnan(y[2])), y[2]
            keep = [0, 1, 3, 4]
            assert np.all(np.isfinite(y[keep])) and abs_err(y[keep], want[keep]) <= TOL
        y1 = e.run(x[2:3])
        assert np.all(np.isnan(y1))
        _check(e, x[:2], want[:2], f"{name} {form} after the NaN row")
        assert e.resident_launches == (1 if res else 0)


@pytest.mark.parametrize("form", list(FORMS))
def test_zero_variance_layer(form, monkeypatch):
    """Variance exactly 0: the finite b-only output, whatever the observation, on all three."""
    from go2_onnx_controller_amd import Engine
    res, env = FORMS[form]
    if env:
        monkeypatch.setenv(env, "1")
    model, want = lm.zero_variance_model()
    rng = np.random.default_rng(5)
    with Engine(model, max_batch=8, ln_small=True, resident_ms=res) as e:
        assert e.small_kernel == "policy_latency_kernel"
        if res:
            assert e.resident_kernel.startswith("policy_resident_kernel" if env else "policy_act1_kernel")
        for B in (1, 8, 3):
            x = (rng.standard_normal((B, 10)) * 10).astype(np.float32)
            y = e.run(x)
            assert np.all(np.isfinite(y)) and abs_err(y, np.tile(want, (B, 1))) <= TOL
            assert np.array_equal(y, np.tile(y[:1], (B, 1)))  # independent of the observation, bitwise
        assert e.resident_launches == (1 if res else 0)


# ---- 6. the controller tick: policy_latency_ctl_kernel at batch <= 8 (no resident controller form)
@pytest.mark.parametrize("res", [0, RES_MS])
@pytest.mark.parametrize("B", [1, 8])
def test_controller_tick(synth_path, B, res):
    """As tests/test_gpu_layernorm.py test_controller_tick: bit-identical observation rows,
    actions within the policy tolerance. With a resident kernel, run() calls between the
    ticks: each tick stops the live act() kernel, the next run() relaunches it."""
    from go2_onnx_controller_amd import Engine
    from oracle import controller_ref as cr
    p = synth_path("ln_ctl_post")
    ref = _ref(p)
    with Engine(p, max_batch=8, ln_small=True, resident_ms=res) as e:
        assert e.ctl_history() == 2
        obs = np.zeros((B, e.in_dim), np.float32)
        act = np.zeros((B, 12), np.float32)
        for t, (st, joy) in enumerate(ln_ref.ctl_inputs(B, 3)):
            o0, a0 = obs.copy(), act.copy()
            q_des, kp, kd, status = e.controller_step(st, obs, act, joy=joy)
            want_obs, a_ref, _, kp_ref, kd_ref, want_status = cr.tick(ref.f64, st, joy, o0, a0, 2)
            assert np.array_equal(obs, want_obs, equal_nan=True), np.argwhere(obs != want_obs)[:5]
            assert rel_err(act, a_ref) <= TOL
            p0 = cr.default_params()
            assert np.array_equal(q_des, np.asarray(p0["q0"])[None] + act.astype(np.float64) * p0["action_scale"])
            assert np.array_equal(kp, kp_ref) and np.array_equal(kd, kd_ref)
            assert np.array_equal(status, want_status)
            if res:
                for i in (t, t + 8):
                    Bi = lm.resident_batches()[i]
                    x, want = _want(p, "ln_ctl_post", Bi, lm.resident_seed("ln_ctl_post", i))
                    _check(e, x, want, f"ln_ctl_post run() after tick {t} B={Bi}")
                assert e.resident_launches == t + 1
        if not res:
            assert e.resident_launches == 0


# ---- 7. the drop-in: the C++ ONNXActor and its Python mirror with GO2PI_LN_SMALL=1
@pytest.mark.parametrize("ln_small", ["1", "0"])
def test_cpp_onnx_actor(synth_path, tmp_path, ln_small):
    """tests/cpp/controller_shape.cpp (shaped for 98 -> 12) on ln_ctl_post, as
    tests/test_gpu_boundary.py runs it on the shipped model: the printed action of the
    "twos" observation and every tick's action against fp64."""
    p = synth_path("ln_ctl_post")
    exe = build_controller_shape()
    env = dict(os.environ, GO2PI_LN_SMALL=ln_small)
    r = subprocess.run([exe, p, "twos"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[:5] == ["Input dimension: 98", "Output dimension: 12", "Input name: observation",
                         "Output name: action", "check_dims: 1"]
    act = np.array([float(v) for v in next(l for l in lines if l.startswith("Action:")).split()[1:]])
    assert abs_err(act, _ref(p).f64(np.full((1, 98), 2, np.float32))[0]) <= TOL
    dump = tmp_path / "actions.bin"
    r = subprocess.run([exe, p, "ticks", str(lm.DROPIN_TICKS), str(dump)], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(dump, np.float32).reshape(lm.DROPIN_TICKS, 12)
    assert abs_err(got, _ref(p).f64(lm.dropin_observations())) <= TOL
    assert len(np.unique(got[:, 0])) > lm.DROPIN_TICKS // 2  # the actions follow the changing observation


def test_python_onnx_actor(synth_path, monkeypatch):
    from go2_onnx_controller_amd import ONNXActor
    p = synth_path("ln_ctl_post")
    obs, act = np.zeros(98, np.float32), np.zeros(12, np.float32)
    monkeypatch.delenv("GO2PI_LN_SMALL", raising=False)
    assert ONNXActor(p, obs, act)._engine.resident_kernel == "none"  # off unless asked for
    monkeypatch.setenv("GO2PI_LN_SMALL", "1")
    actor = ONNXActor(p, obs, act)
    assert actor._engine.resident_kernel.startswith("policy_act1_kernel")
    for i in range(5):
        x, want = _want(p, "ln_ctl_post", 1, lm.resident_seed("ln_ctl_post", i))
        obs[:] = x[0]  # the caller writes in place, like populate_buffer
        actor.act()
        assert abs_err(act, want[0]) <= TOL
    assert actor._engine.resident_launches == 1
