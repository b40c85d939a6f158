"""GPU: residual MLP policies at batch <= 8 on the single launch (policy_latency_kernel, its
policy_latency_res_kernel instantiation) and the multi-workgroup resident kernel
(policy_resident_kernel), the opt-in of GO2PI_RESIDUAL_SMALL, against the float64 oracle at the
project's 1e-5 and, for the integer probes, exactly. tests/test_cpu_res_small.py and
tests/test_cpu_res.py check on the same inputs that float32 arithmetic alone stays under a third
of the tolerance.

The carried value of these two kernels lives in the publishing lanes' registers across layers
(and, in the resident kernel, across requests), so beside parity the tests look at what that
can get wrong: a workgroup that skips a layer between source and consumer (probe_neck), a
consumer padded wider than its source (probe_wide_consumer, res_skip), a second request on the
same engine, a smaller request behind a larger one, a NaN row, and the (sum + bias) + carried
order, bit for bit against the GEMV chain.

The switches are read when an engine is created, so every test sets them first.
"""
import os
import subprocess
import time

import numpy as np
import pytest

import policy_specs as ps
import res_small_specs as rs
from conftest import abs_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
RES_MS = 5000
SW = rs.SW
CHAIN = "gemv_layer_kernel graph"
LATENCY = "policy_latency_kernel"
MULTI = "policy_resident_kernel"
FORMS = ("launch", "resident")
ALL_SWITCHES = (SW, "GO2PI_SKIP_SMALL", "GO2PI_SMALL_CHAIN", "GO2PI_RES_MULTI", "GO2PI_RES_TILED0", "GO2PI_REQ_HOST")


def _env(monkeypatch, name, *extra):
    """The environment of an engine for `name` on the small-batch kernels, and nothing else."""
    for s in ALL_SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for s in rs.switches(name) + extra:
        monkeypatch.setenv(s, "1")


def _engine(name, form, **kw):
    """An engine created under the switches (the caller has set them): the single launch, or
    the resident kernel."""
    from go2_onnx_controller_amd import Engine
    kw.setdefault("max_batch", 8)
    for k, v in rs.opts(name).items():
        kw.setdefault(k, bool(v))
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
    name = "simba_64"
    _env(monkeypatch, name)
    monkeypatch.delenv(SW)
    with Engine(ps.path(name), max_batch=8, resident_ms=RES_MS, ln_small=True) as e:  # as tests/test_gpu_res.py pins it
        assert e.small_kernel == CHAIN and e.resident_kernel.startswith("none")
    monkeypatch.setenv(SW, "1")
    with Engine(ps.path(name), max_batch=8, resident_ms=RES_MS) as e:  # without the LN bit: the chain
        assert e.small_kernel == CHAIN and e.resident_kernel.startswith("none")
    with Engine(ps.path(name), max_batch=64, resident_ms=RES_MS, ln_small=True) as e:
        assert e.small_kernel == LATENCY
        assert e.resident_kernel.startswith(MULTI + " ring="), e.resident_kernel
        assert e.batched_kernel.startswith("policy_fused_res_kernel<8>")
        assert abs_err(e.run(ps.obs(name, 33)), ps.want(name, 33)) <= TOL  # the batched body
        assert abs_err(e.run(ps.obs(name, 5)), ps.want(name, 5)) <= TOL
    _env(monkeypatch, "res_skip")
    monkeypatch.delenv("GO2PI_SKIP_SMALL")
    with Engine(ps.path("res_skip"), max_batch=8, resident_ms=RES_MS) as e:  # without GO2PI_SKIP_SMALL: the chain
        assert e.small_kernel == CHAIN and e.resident_kernel.startswith("none")


# ---- 2. parity
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", rs.NAMES)
def test_parity(name, form, monkeypatch):
    _env(monkeypatch, name)
    worst = 0.0
    with _engine(name, form) as e:
        for B in rs.RES_SMALL.small_batches:
            y = e.run(ps.obs(name, B))
            err = abs_err(y, ps.want(name, B))
            worst = max(worst, err)
            assert np.isfinite(y).all() and err <= TOL, (name, form, B, err)
        _served_by(e, form)
    print(f"{name} {form}: worst abs err {worst:.3g}")


@pytest.mark.parametrize("name", ["simba_256", "res_skip"])
def test_parity_ring_in_host_memory(name, monkeypatch):
    _env(monkeypatch, name, "GO2PI_REQ_HOST")
    worst = 0.0
    with _engine(name, "resident") as e:
        assert e.resident_kernel.endswith("ring=host")
        for B in rs.RES_SMALL.small_batches:
            err = abs_err(e.run(ps.obs(name, B)), ps.want(name, B))
            worst = max(worst, err)
            assert err <= TOL, (name, B, err)
        _served_by(e, "resident")
    print(f"{name} GO2PI_REQ_HOST: worst abs err {worst:.3g}")


# ---- 3. the probes, exactly, in an order that would show a stale row of a larger request
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", rs.PROBES)
def test_probes_exact(name, form, monkeypatch):
    _env(monkeypatch, name)
    with _engine(name, form) as e:
        for B in rs.RES_SMALL.probe_batches:
            x = ps.probe_obs(name, B)
            got = e.run(x)
            assert np.array_equal(got, np.rint(got)), (name, form, B)
            assert np.array_equal(got.astype(np.int64), ps.probe_forward(name, x)), (name, form, B)
        _served_by(e, form)


# ---- 4. the three forms return the same bits
def _three_forms(name, monkeypatch):
    from go2_onnx_controller_amd import Engine
    kw = {k: bool(v) for k, v in rs.opts(name).items()}
    xs = {B: ps.obs(name, B, 2) for B in rs.RES_SMALL.small_batches}
    got = {}
    for form, extra, res_ms in (("chain", ("GO2PI_SMALL_CHAIN",), 0), ("launch", (), 0),
                                ("resident", ("GO2PI_RES_MULTI",), RES_MS)):
        _env(monkeypatch, name, *extra)
        with Engine(ps.path(name), max_batch=8, resident_ms=res_ms, **kw) as e:
            assert e.small_kernel == (CHAIN if form == "chain" else LATENCY), (name, form, e.small_kernel)
            if form == "resident":
                assert e.resident_kernel.startswith(MULTI + " ring="), e.resident_kernel
            else:
                assert e.resident_kernel.startswith("none")
            got[form] = {B: e.run(x) for B, x in xs.items()}
            assert e.resident_launches == (1 if form == "resident" else 0)
    return xs, got


@pytest.mark.parametrize("name", ["simba_64", "res_adjacent", "res_post", "res_skip", "simba_round2"])
def test_three_forms_bitwise_equal(name, monkeypatch):
    """tests/test_gpu_small_forms.py's claim with the carried add in it: equal bits only if the
    add is (sum + bias) + carried in all three."""
    xs, got = _three_forms(name, monkeypatch)
    for B, x in xs.items():
        want = ps.ref(name).f64(x)
        for form, ys in got.items():
            err = abs_err(ys[B], want)
            print(f"{name} {form} B={B}: abs err {err:.3g}")
            assert np.isfinite(ys[B]).all() and err <= TOL, (name, form, B, err)
        for form in ("launch", "resident"):
            diff = int(np.count_nonzero(got[form][B].view(np.uint32) != got["chain"][B].view(np.uint32)))
            print(f"{name} {form} vs chain B={B}: {diff} of {got[form][B].size} words differ")
            assert diff == 0, (name, form, B)


# ---- 5. a second request carries nothing of the first
@pytest.mark.parametrize("form,kw", [("resident", {}), ("launch", {"use_graph": False}), ("launch", {"use_graph": True})])
@pytest.mark.parametrize("name", ["simba_64", "res_neck"])
def test_second_request_carries_its_own_value(name, form, kw, monkeypatch):
    _env(monkeypatch, name)
    a, b = ps.obs(name, 5), ps.obs(name, 5, 1)
    with _engine(name, form, **kw) as e:
        ya, yb, ya2 = e.run(a), e.run(b), e.run(a)
        y1 = e.run(b[:1])  # a smaller request behind a larger one
        _served_by(e, form)
    assert abs_err(ya, ps.want(name, 5)) <= TOL and abs_err(yb, ps.want(name, 5, 1)) <= TOL
    assert not np.array_equal(ya, yb) and np.array_equal(ya, ya2)
    assert np.array_equal(y1[0], yb[0])


# ---- 6. a NaN stays in its row
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["simba_64", "res_v1"])
def test_nan_stays_in_its_row(name, form, monkeypatch):
    _env(monkeypatch, name)
    B = 5
    x = ps.obs(name, B)
    bad = x.copy()
    bad[2, 10] = np.nan
    with _engine(name, form) as e:
        clean, y, after = e.run(x), e.run(bad), e.run(x)  # ... and the carried rows keep nothing of it
        _served_by(e, form)
    assert np.isnan(y[2]).all(), y[2]
    keep = np.arange(B) != 2
    assert np.array_equal(y[keep].view(np.uint32), clean[keep].view(np.uint32))
    assert np.array_equal(after, clean)


# ---- 7. idle exit and relaunch: the new launch starts from cleared carried rows
def test_idle_exit_and_relaunch(monkeypatch):
    from go2_onnx_controller_amd import Engine
    name = "simba_64"
    _env(monkeypatch, name)
    with Engine(ps.path(name), max_batch=8, resident_ms=4, ln_small=True) as e:
        assert e.resident_kernel.startswith(MULTI)
        first = e.run(ps.obs(name, 5))
        assert abs_err(first, ps.want(name, 5)) <= TOL
        assert e.resident_launches == 1
        time.sleep(0.05)  # past resident_ms: the kernel has left
        again = e.run(ps.obs(name, 5))
        assert e.resident_launches == 2
        assert np.array_equal(first, again)


# ---- 8. the drop-in
def test_python_onnx_actor(monkeypatch):
    from go2_onnx_controller_amd import ONNXActor
    name = "simba_64"
    obs, act = np.zeros(ps.in_dim(name), np.float32), np.zeros(12, np.float32)
    _env(monkeypatch, name)
    monkeypatch.delenv(SW)
    monkeypatch.delenv("GO2PI_RESIDENT_MS", raising=False)
    monkeypatch.setenv("GO2PI_LN_SMALL", "1")
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
    """tests/cpp/controller_shape.cpp's "ticks" mode on simba_64 in a fresh child process under
    the switches. Its observation buffer is a Go2 controller's 98 floats; the model reads the
    first 48 (check_dims reports the mismatch, act() serves the model's own width)."""
    from test_cpu_boundary import build_controller_shape
    name = "simba_64"
    exe = build_controller_shape()
    dump, ticks = tmp_path / "actions.bin", 60
    env = {k: v for k, v in os.environ.items() if k not in ALL_SWITCHES}
    env.update(GO2PI_RESIDENT_MS=resident, GO2PI_RESIDUAL_SMALL="1", GO2PI_LN_SMALL="1")
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


# ---- 9. the controller tick stays refused
def test_controller_step_is_refused(monkeypatch):
    from go2_onnx_controller_amd import Go2piError
    from oracle import controller_ref as cr
    name = "res_skip"  # a Go2 controller's I/O: 98 observations, 12 actions
    _env(monkeypatch, name)
    rng = np.random.default_rng(0)
    with _engine(name, "resident") as e:
        for B in (1, 8):
            st, joy = cr.synthetic_states(rng, B), cr.synthetic_joy(rng, B)
            obs, act = np.zeros((B, 98), np.float32), np.zeros((B, 12), np.float32)
            with pytest.raises(Go2piError, match="does not serve a policy with residual connections"):
                e.controller_step(st, obs, act, joy=joy)
        assert abs_err(e.run(ps.obs(name, 5)), ps.want(name, 5)) <= TOL  # the engine still serves run()
