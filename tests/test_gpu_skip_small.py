"""GPU: policies with observation skip inputs at batch <= 8 on the single launch
(policy_latency_kernel) and the multi-workgroup resident kernel (policy_resident_kernel), the
opt-in of GO2PI_SKIP_SMALL, against the float64 oracle at the project's 1e-5 and, for the
integer probes, exactly. tests/test_cpu_skip_small.py and tests/test_cpu_skip.py check on the
same inputs that float32 arithmetic alone stays under a third of the tolerance.

The switch is read when an engine is created, so every test sets it first.
"""
import os
import subprocess
import time
import warnings

import numpy as np
import pytest

import policy_specs as ps
from conftest import abs_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
RES_MS = 5000
SW = "GO2PI_SKIP_SMALL"
LATENCY = "policy_latency_kernel"
MULTI = "policy_resident_kernel"
FORMS = ("launch", "resident")


def _engine(name, form, **kw):
    """An engine created under the switch (the caller has set it): the single launch, or the
    resident kernel."""
    from go2_onnx_controller_amd import Engine
    kw.setdefault("max_batch", 8)
    if name == "ea_ln":
        kw.setdefault("ln_small", True)
    e = Engine(ps.path(name), resident_ms=RES_MS if form == "resident" else 0, **kw)
    assert e.small_kernel == LATENCY, e.small_kernel
    if form == "resident":
        assert e.resident_kernel.startswith(MULTI + " ring="), e.resident_kernel
    else:
        assert e.resident_kernel == "none"
    return e


def _served_by(e, form):
    assert e.resident_launches == (1 if form == "resident" else 0), (form, e.resident_launches)


# ---- 1. selection on the device
def test_selection(monkeypatch):
    from go2_onnx_controller_amd import Engine
    monkeypatch.delenv(SW, raising=False)
    with Engine(ps.path("ea_98"), max_batch=8, resident_ms=RES_MS) as e:  # as tests/test_gpu_skip.py pins it
        assert e.small_kernel == "gemv_layer_kernel graph" and e.resident_kernel.startswith("none")
    monkeypatch.setenv(SW, "1")
    with Engine(ps.path("ea_98"), max_batch=64, resident_ms=RES_MS) as e:
        assert e.small_kernel == LATENCY
        assert e.resident_kernel.startswith(MULTI + " ring="), e.resident_kernel
        assert e.batched_kernel.startswith("policy_fused_kernel<8, 0, 0, 0, 0,")
        assert abs_err(e.run(ps.obs("ea_98", 33)), ps.ref("ea_98").f64(ps.obs("ea_98", 33))) <= TOL  # the batched body
        assert abs_err(e.run(ps.obs("ea_98", 5)), ps.want("ea_98", 5)) <= TOL


# ---- 2. parity
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ps.SMALL_NAMES)
def test_parity(name, form, monkeypatch):
    monkeypatch.setenv(SW, "1")
    with _engine(name, form) as e:
        for B in ps.SKIP_SMALL.small_batches:
            y = e.run(ps.obs(name, B))
            err = abs_err(y, ps.want(name, B))
            print(f"{name} {form} B={B}: {err:.3g}")
            assert np.isfinite(y).all() and err <= TOL, (name, form, B, err)
        _served_by(e, form)


@pytest.mark.parametrize("env", ["GO2PI_RES_TILED0", "GO2PI_REQ_HOST"])
@pytest.mark.parametrize("name", ["ea_98", "ea_round2"])
def test_parity_resident_variants(name, env, monkeypatch):
    monkeypatch.setenv(SW, "1")
    monkeypatch.setenv(env, "1")
    with _engine(name, "resident") as e:
        if env == "GO2PI_REQ_HOST":
            assert e.resident_kernel.endswith("ring=host")
        for B in ps.SKIP_SMALL.small_batches:
            err = abs_err(e.run(ps.obs(name, B)), ps.want(name, B))
            print(f"{name} {env} B={B}: {err:.3g}")
            assert err <= TOL, (name, env, B, err)
        _served_by(e, "resident")


# ---- 3. the probes, exactly, in an order that would show a stale row of a larger request
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ps.SMALL_PROBES)
def test_probes_exact(name, form, monkeypatch):
    monkeypatch.setenv(SW, "1")
    with _engine(name, form) as e:
        for B in ps.SKIP_SMALL.probe_batches:
            x = ps.probe_obs(name, B)
            got = e.run(x)
            assert np.array_equal(got, np.rint(got)), (name, form, B)
            assert np.array_equal(got.astype(np.int64), ps.probe_forward(name, x)), (name, form, B)
        _served_by(e, form)


def test_probe_local0_tiled(monkeypatch):
    """probe_local0 with layer 0 tiled: the skip on layer 1 behind a sweep, not behind local layer 0."""
    monkeypatch.setenv(SW, "1")
    monkeypatch.setenv("GO2PI_RES_TILED0", "1")
    with _engine("probe_local0", "resident") as e:
        for B in ps.SKIP_SMALL.probe_batches:
            x = ps.probe_obs("probe_local0", B)
            assert np.array_equal(e.run(x).astype(np.int64), ps.probe_forward("probe_local0", x)), B
        _served_by(e, "resident")


# ---- 4. a fresh observation reaches the skip columns
@pytest.mark.parametrize("form,kw", [("resident", {}), ("launch", {"use_graph": False}), ("launch", {"use_graph": True})])
def test_second_request_reads_its_own_skip_columns(form, kw, monkeypatch):
    """ea_l0slice: layer 0 reads obs[49:98], the skip obs[0:49]. Two requests that differ in
    obs[0:49] alone differ through the skip alone."""
    monkeypatch.setenv(SW, "1")
    name = "ea_l0slice"
    a = ps.obs(name, 5)
    b = a.copy()
    b[:, :49] = ps.obs(name, 5, 1)[:, :49]
    with _engine(name, form, **kw) as e:
        ya, yb, ya2 = e.run(a), e.run(b), e.run(a)
        _served_by(e, form)
    assert abs_err(ya, ps.ref(name).f64(a)) <= TOL and abs_err(yb, ps.ref(name).f64(b)) <= TOL
    assert not np.array_equal(ya, yb) and np.array_equal(ya, ya2)


# ---- 5. placement
@pytest.mark.parametrize("form", FORMS)
def test_nan_in_a_skip_only_column_stays_in_its_row(form, monkeypatch):
    monkeypatch.setenv(SW, "1")
    name, B = "ea_l0slice", 5
    x = ps.obs(name, B)
    bad = x.copy()
    bad[2, 3] = np.nan  # read by the skip alone
    with _engine(name, form) as e:
        clean, y = e.run(x), e.run(bad)
        _served_by(e, form)
    assert np.isnan(y[2]).all(), y[2]
    keep = np.arange(B) != 2
    assert np.array_equal(y[keep], clean[keep])


@pytest.mark.parametrize("form", FORMS)
def test_inf_in_a_skip_column_is_clipped_by_the_prologue(form, monkeypatch):
    """ea_front: the skip reads the normalised, clipped observation; +inf is the Clip's upper bound."""
    monkeypatch.setenv(SW, "1")
    name, B = "ea_front", 5
    x = ps.obs(name, B)
    x[1, 7] = np.inf
    big = x.copy()
    big[1, 7] = 1e30  # clipped to the same bound
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want = ps.ref(name).f64(x)
    assert np.isfinite(want).all()
    with _engine(name, form) as e:
        y, yb = e.run(x), e.run(big)
        _served_by(e, form)
    assert np.isfinite(y).all() and abs_err(y, want) <= TOL
    assert np.array_equal(y, yb)


# ---- 6. the forms agree
@pytest.mark.parametrize("name", ["ea_k64", "ea_two"])
def test_resident_tiled0_bitwise_equals_single_launch(name, monkeypatch):
    monkeypatch.setenv(SW, "1")
    with _engine(name, "launch") as s:
        single = {B: s.run(ps.obs(name, B)) for B in (1, 8)}
    monkeypatch.setenv("GO2PI_RES_TILED0", "1")
    with _engine(name, "resident") as r:
        for B in (1, 8):
            assert np.array_equal(r.run(ps.obs(name, B)), single[B]), (name, B)
        _served_by(r, "resident")


# ---- 7. idle exit and relaunch
def test_idle_exit_and_relaunch(monkeypatch):
    from go2_onnx_controller_amd import Engine
    monkeypatch.setenv(SW, "1")
    name = "ea_98"
    with Engine(ps.path(name), max_batch=8, resident_ms=4) as e:
        assert e.resident_kernel.startswith(MULTI)
        assert abs_err(e.run(ps.obs(name, 5)), ps.want(name, 5)) <= TOL
        assert e.resident_launches == 1
        time.sleep(0.05)  # past resident_ms: the kernel has left
        assert abs_err(e.run(ps.obs(name, 8)), ps.want(name, 8)) <= TOL
        assert e.resident_launches == 2


# ---- 8. the drop-in
def test_python_onnx_actor(monkeypatch):
    from go2_onnx_controller_amd import ONNXActor
    name = "ea_k64"
    obs, act = np.zeros(ps.in_dim(name), np.float32), np.zeros(12, np.float32)
    monkeypatch.delenv("GO2PI_RESIDENT_MS", raising=False)
    monkeypatch.delenv(SW, raising=False)
    assert ONNXActor(ps.path(name), obs, act)._engine.resident_kernel.startswith("none")  # off unless asked for
    monkeypatch.setenv(SW, "1")
    actor = ONNXActor(ps.path(name), obs, act)
    assert actor.check_dims()
    assert actor._engine.small_kernel == LATENCY and actor._engine.resident_kernel.startswith(MULTI)
    x = np.concatenate([ps.obs(name, 8, k) for k in range(3)])[:20]
    want = ps.ref(name).f64(x)
    for i in range(20):
        obs[:] = x[i]  # the caller writes in place, like populate_buffer
        actor.act()
        assert abs_err(act, want[i]) <= TOL, i
    assert actor._engine.resident_launches == 1


@pytest.mark.parametrize("resident", ["100", "0"])
def test_cpp_onnx_actor_ticks(resident, tmp_path):
    """tests/cpp/controller_shape.cpp's "ticks" mode (shaped for 98 -> 12) on ea_98 in a child
    process under the switch, as tests/test_gpu_skip.py runs it without."""
    from test_cpu_boundary import build_controller_shape
    exe = build_controller_shape()
    dump, ticks = tmp_path / "actions.bin", 60
    r = subprocess.run([exe, ps.path("ea_98"), "ticks", str(ticks), str(dump)], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, GO2PI_RESIDENT_MS=resident, GO2PI_SKIP_SMALL="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "check_dims: 1" in r.stdout
    got = np.fromfile(dump, np.float32).reshape(ticks, 12)
    o, seq = np.zeros(98, np.float32), np.empty((ticks, 98), np.float32)
    for t in range(ticks):
        o[t % 98] += np.float32(0.001)
        seq[t] = o
    assert abs_err(got, ps.ref("ea_98").f64(seq)) <= TOL
    assert not np.array_equal(got[0], got[1])


# ---- 9. the controller tick stays refused
def test_controller_step_is_refused(monkeypatch):
    from go2_onnx_controller_amd import Go2piError
    from oracle import controller_ref as cr
    monkeypatch.setenv(SW, "1")
    rng = np.random.default_rng(0)
    with _engine("ea_98", "resident") as e:
        for B in (1, 8):
            st, joy = cr.synthetic_states(rng, B), cr.synthetic_joy(rng, B)
            obs, act = np.zeros((B, 98), np.float32), np.zeros((B, 12), np.float32)
            with pytest.raises(Go2piError, match="does not serve a policy with observation skip inputs"):
                e.controller_step(st, obs, act, joy=joy)
        assert abs_err(e.run(ps.obs("ea_98", 5)), ps.want("ea_98", 5)) <= TOL  # the engine still serves run()
