"""GPU: residual MLP policies (the res family of tests/policy_specs.py) on the two kernels that serve them: the
general batched body with a carried tile (policy_fused_res_kernel<8>, fused_impl.hpp RES) and
the GEMV chain with its carry buffers (gemv_layer_kernel), against the float64 reference at
the project's 1e-5 and, for the integer probes, exactly. tests/test_cpu_res.py checks on the
same inputs that float32 arithmetic alone stays under a third of the tolerance.
"""
import os
import subprocess

import numpy as np
import pytest

import policy_specs as ps
from conftest import abs_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
GEMV = "gemv_layer_kernel graph"
BODY = "policy_fused_res_kernel<8>"


def _engine(name, **kw):
    from go2_onnx_controller_amd import Engine
    kw.setdefault("max_batch", 128)
    return Engine(ps.path(name), **kw)


# ---- 1. parity
@pytest.mark.parametrize("name", ps.RES.names)
def test_parity(name):
    with _engine(name, resident_ms=100) as e:
        assert e.batched_kernel.startswith(BODY), e.batched_kernel
        assert e.small_kernel == GEMV
        assert e.resident_kernel.startswith("none"), e.resident_kernel
        assert e.in_dim == ps.in_dim(name)
        for B in ps.RES.parity_batches:
            err = abs_err(e.run(ps.obs(name, B)), ps.want(name, B))
            print(f"{name} B={B}: {err:.3g}")
            assert err <= TOL, (name, B, err)


# ---- 2. the probes, exactly
@pytest.mark.parametrize("name", ps.RES.probes)
def test_probes_exact(name):
    with _engine(name, small_batch=-1) as e:  # the body at every batch
        assert e.small_kernel.startswith(BODY)
        for B in (33, 1, 16, 17):
            x = ps.probe_obs(name, B)
            got = e.run(x)
            assert np.array_equal(got, np.rint(got)) and np.array_equal(got.astype(np.int64), ps.probe_forward(name, x)), \
                (name, "body", B)
    with _engine(name) as e:  # the chain
        assert e.small_kernel == GEMV
        for B in (8, 1, 5):
            x = ps.probe_obs(name, B)
            got = e.run(x)
            assert np.array_equal(got, np.rint(got)) and np.array_equal(got.astype(np.int64), ps.probe_forward(name, x)), \
                (name, "chain", B)


# ---- 3. the replayed graph reads fresh carry rows
@pytest.mark.parametrize("name", ["res_adjacent", "simba_64"])
def test_graph_replay(name):
    with _engine(name) as e:
        assert e.small_kernel == GEMV
        for B in (1, 5):
            xs = [ps.obs(name, B, k) for k in (0, 1, 0)]
            ys = [e.run(x) for x in xs]
            for k, y in zip((0, 1, 0), ys):
                assert abs_err(y, ps.want(name, B, k)) <= TOL, (name, B, k)
            assert np.array_equal(ys[0], ys[2]) and not np.array_equal(ys[0], ys[1])


# ---- 4. non-finite inputs stay in their row
@pytest.mark.parametrize("B", [5, 33])  # the chain, the body
@pytest.mark.parametrize("name", ["simba_64", "res_adjacent", "res_skip"])
def test_nan_stays_in_its_row(name, B):
    """The rows beside a NaN row equal the clean run bit for bit: garbage in the carried
    tile or in a carry buffer would move them."""
    x = ps.obs(name, B)
    with _engine(name) as e:
        clean = e.run(x)
        bad = x.copy()
        bad[2, 10] = np.nan
        y = e.run(bad)
        after = e.run(x)  # ... and the carried rows keep nothing of it
    assert np.isnan(y[2]).all(), y[2]
    keep = np.arange(B) != 2
    assert np.array_equal(y[keep], clean[keep])
    assert np.array_equal(after, clean)


# ---- 5. clean pads
@pytest.mark.parametrize("B", [5, 33])
@pytest.mark.parametrize("name", ["res_skip", "res_sig"])
def test_clean_pads(name, B):
    """res_skip: the consumer is padded past its source, so part of the carried tile (and of
    the carry buffer) is written by no layer. res_sig: the written pads hold sums of 0.5s.
    Twice, each time on a fresh engine."""
    for _ in range(2):
        with _engine(name) as e:
            y = e.run(ps.obs(name, B))
        assert np.isfinite(y).all()
        assert abs_err(y, ps.want(name, B)) <= TOL


# ---- 6. device sequence
def test_sequence_equals_single_runs():
    import torch
    name, B, T = "simba_64", 33, 3
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


# ---- 7. shards and repeats
@pytest.mark.parametrize("name", ["simba_256", "res_v1"])
def test_shards_and_repeats_bitwise(name):
    x = ps.obs(name, 33)
    with _engine(name) as e:
        whole = e.run(x)
        again = e.run(x)
        parts = np.concatenate([e.run(x[:16]), e.run(x[16:])])
        small = [e.run(x[:5]), e.run(x[:5])]
    assert np.array_equal(whole, again)
    assert np.array_equal(whole, parts)
    assert np.array_equal(small[0], small[1])


# ---- 8. the drop-in actors
def test_python_onnx_actor():
    from go2_onnx_controller_amd import ONNXActor
    name = "simba_64"
    obs, act = np.zeros(48, np.float32), np.zeros(12, np.float32)
    actor = ONNXActor(ps.path(name), obs, act)
    assert actor.check_dims()
    x = ps.obs(name, 5)
    seen = []
    for i in (0, 1, 0):
        obs[:] = x[i]
        actor.act()
        assert abs_err(act, ps.want(name, 5)[i]) <= TOL, i
        seen.append(act.copy())
    assert not np.array_equal(seen[0], seen[1]) and np.array_equal(seen[0], seen[2])


@pytest.mark.parametrize("resident", ["100", "0"])
def test_cpp_onnx_actor_ticks(resident, tmp_path):
    """tests/cpp/controller_shape.cpp's "ticks" mode on res_skip (98 observations, 12 actions):
    the observation changes in place before each act(); every tick against the reference."""
    from test_cpu_boundary import build_controller_shape
    exe = build_controller_shape()
    dump, ticks = tmp_path / "actions.bin", 60
    r = subprocess.run([exe, ps.path("res_skip"), "ticks", str(ticks), str(dump)], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, GO2PI_RESIDENT_MS=resident))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "check_dims: 1" in r.stdout
    got = np.fromfile(dump, np.float32).reshape(ticks, 12)
    o, seq = np.zeros(98, np.float32), np.empty((ticks, 98), np.float32)
    for t in range(ticks):
        o[t % 98] += np.float32(0.001)
        seq[t] = o
    assert abs_err(got, ps.ref("res_skip").f64(seq)) <= TOL
    assert len(np.unique(got[:, 0])) > ticks // 2


# ---- 9. error paths
def test_controller_step_is_refused():
    from go2_onnx_controller_amd import Go2piError
    from oracle import controller_ref as cr
    rng = np.random.default_rng(0)
    name = "res_skip"  # a Go2 controller's I/O: 98 observations, 12 actions
    with _engine(name) as e:
        for B in (1, 33):
            st, joy = cr.synthetic_states(rng, B), cr.synthetic_joy(rng, B)
            obs, act = np.zeros((B, 98), np.float32), np.zeros((B, 12), np.float32)
            with pytest.raises(Go2piError, match="the controller tick does not serve a policy with residual connections"):
                e.controller_step(st, obs, act, joy=joy)
        assert abs_err(e.run(ps.obs(name, 5)), ps.want(name, 5)) <= TOL  # the engine still serves run()


def test_explicit_waves_are_refused():
    from go2_onnx_controller_amd import Engine, Go2piError
    for waves in (4, 16):
        with pytest.raises(Go2piError, match="residual connections"):
            Engine(ps.path("simba_64"), max_batch=8, waves=waves)
