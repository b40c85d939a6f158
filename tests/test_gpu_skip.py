"""GPU: estimator-actor policies (observation skip inputs, the skip family of tests/policy_specs.py) on the two
kernels that serve them: the general batched body (skip_tile / gather_stage, fused_impl.hpp)
and the GEMV chain (gemv_layer_kernel), against the float64 oracle at the project's 1e-5
and, for the integer probes, exactly. tests/test_cpu_skip.py checks on the same inputs that
float32 arithmetic alone stays under a third of the tolerance.
"""
import os
import subprocess
import warnings

import numpy as np
import pytest

import policy_specs as ps
from conftest import abs_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
GEMV = "gemv_layer_kernel graph"


def _engine(name, **kw):
    from go2_onnx_controller_amd import Engine
    kw.setdefault("max_batch", 128)
    return Engine(ps.path(name), **kw)


def _fused_name(nw):
    return f"policy_fused_kernel<{nw}, 0, 0, 0, 0,"


# ---- 1. parity
@pytest.mark.parametrize("name", ps.SKIP.names)
def test_parity(name):
    with _engine(name, resident_ms=100) as e:
        assert e.batched_kernel.startswith(_fused_name(8)), e.batched_kernel
        assert e.small_kernel == GEMV
        assert e.resident_kernel.startswith("none"), e.resident_kernel
        assert e.in_dim == ps.in_dim(name)
        for B in ps.SKIP.parity_batches:
            err = abs_err(e.run(ps.obs(name, B)), ps.want(name, B))
            print(f"{name} B={B}: {err:.3g}")
            assert err <= TOL, (name, B, err)


# ---- 2. the probes, exactly
@pytest.mark.parametrize("name", ps.SKIP.probes)
def test_probes_exact(name):
    with _engine(name, small_batch=-1) as e:  # the general body at every batch
        assert e.small_kernel.startswith(_fused_name(8))
        for B in (33, 1, 16, 17):
            x = ps.probe_obs(name, B)
            assert np.array_equal(e.run(x).astype(np.int64), ps.probe_forward(name, x)), (name, "body", B)
    with _engine(name) as e:  # the chain
        assert e.small_kernel == GEMV
        for B in (8, 1, 5):
            x = ps.probe_obs(name, B)
            got = e.run(x)
            assert np.array_equal(got, np.rint(got)) and np.array_equal(got.astype(np.int64), ps.probe_forward(name, x)), \
                (name, "chain", B)


# ---- 3. waves x small_batch
@pytest.mark.parametrize("small_batch", [-1, 8])
@pytest.mark.parametrize("waves", [4, 8, 16])
@pytest.mark.parametrize("name", ["ea_two", "ea_ln"])
def test_waves(name, waves, small_batch):
    with _engine(name, waves=waves, small_batch=small_batch) as e:
        assert e.batched_kernel.startswith(_fused_name(waves)), e.batched_kernel
        assert e.small_kernel == GEMV if small_batch == 8 else e.small_kernel.startswith(_fused_name(waves))
        for B in (1, 8, 17, 33):
            assert abs_err(e.run(ps.obs(name, B)), ps.want(name, B)) <= TOL, (name, waves, small_batch, B)


# ---- 4. non-finite inputs
@pytest.mark.parametrize("B", [5, 33])
@pytest.mark.parametrize("name,col", [("ea_l0slice", 3),    # read only by the skip
                                      ("ea_l0slice", 70),   # read only by the encoder
                                      ("ea_98", 80),        # the encoder only (the skip reads [0, 49))
                                      ("ea_two", 10)])      # both
def test_nan_stays_in_its_row(name, col, B):
    x = ps.obs(name, B)
    with _engine(name) as e:
        clean = e.run(x)
        bad = x.copy()
        bad[2, col] = np.nan
        y = e.run(bad)
    assert np.isnan(y[2]).all(), y[2]
    keep = np.arange(B) != 2
    assert np.array_equal(y[keep], clean[keep])


@pytest.mark.parametrize("B", [5, 33])
def test_inf_in_a_column_layer0_does_not_read(B):
    """ea_l0slice: +inf in a column only the skip reads. Layer 0 gathers its own columns, so
    the encoder stays finite; the pattern per output is the oracle's in float32."""
    name = "ea_l0slice"
    x = ps.obs(name, B)
    x[1, 7] = np.inf
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (inf - inf in the oracle's own matmul)
        want, want64 = ps.ref(name).f32(x), ps.ref(name).f64(x)
    with _engine(name) as e:
        y = e.run(x)

    def pattern(a):
        return np.where(np.isnan(a), 2, np.where(np.isinf(a), np.sign(a), 0))
    assert np.array_equal(pattern(y), pattern(want))
    assert np.isfinite(y[np.arange(B) != 1]).all() and not np.isfinite(y[1]).all()
    fin = np.isfinite(want)
    assert abs_err(y[fin], want64[fin]) <= TOL


# ---- 5. device sequence
@pytest.mark.parametrize("name", ["ea_98", "ea_l0slice"])
def test_sequence_reads_each_steps_rows(name):
    import torch
    B, T = 33, 3
    xs = np.stack([ps.obs(name, B, k) for k in range(T)])
    with _engine(name) as e:
        xd = torch.from_numpy(xs).cuda()
        seq = e.run_sequence_torch(xd)
        single = torch.stack([e.run_torch(xd[t].contiguous()) for t in range(T)])
        torch.cuda.synchronize()
    seq, single = seq.cpu().numpy(), single.cpu().numpy()
    assert np.array_equal(seq, single)
    for t in range(2):
        assert abs_err(seq[t], ps.want(name, B, t)) <= TOL
    assert not np.array_equal(seq[0], seq[1])


# ---- 6. shards and repeats
@pytest.mark.parametrize("name", ["ea_k64", "ea_front"])
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


# ---- 7. the drop-in actor: the replayed graph re-reads the skip columns
def test_python_onnx_actor_two_observations():
    from go2_onnx_controller_amd import ONNXActor
    name = "ea_98"
    obs, act = np.zeros(98, np.float32), np.zeros(12, np.float32)
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
    # only the skip columns differ: the chain's skip layer must read the fresh row
    obs[:] = x[0]
    obs[:49] = x[1][:49]
    actor.act()
    assert abs_err(act, ps.ref(name).f64(obs[None])[0]) <= TOL
    assert not np.array_equal(act, seen[0])


@pytest.mark.parametrize("resident", ["100", "0"])
def test_cpp_onnx_actor_ticks(resident, tmp_path):
    """tests/cpp/controller_shape.cpp's "ticks" mode on ea_98: the observation changes in
    place before each act(); every tick's action against the oracle."""
    from test_cpu_boundary import build_controller_shape
    exe = build_controller_shape()
    dump, ticks = tmp_path / "actions.bin", 60
    r = subprocess.run([exe, ps.path("ea_98"), "ticks", str(ticks), str(dump)], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, GO2PI_RESIDENT_MS=resident))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "check_dims: 1" in r.stdout
    got = np.fromfile(dump, np.float32).reshape(ticks, 12)
    o, seq = np.zeros(98, np.float32), np.empty((ticks, 98), np.float32)
    for t in range(ticks):
        o[t % 98] += np.float32(0.001)
        seq[t] = o
    assert abs_err(got, ps.ref("ea_98").f64(seq)) <= TOL
    assert len(np.unique(got[:, 0])) > ticks // 2
    # ticks 0 .. 48 change columns the skip reads (and the encoder): the action moves with them
    assert not np.array_equal(got[0], got[1])


# ---- 8. error paths
def test_controller_step_is_refused():
    from go2_onnx_controller_amd import Go2piError
    from oracle import controller_ref as cr
    rng = np.random.default_rng(0)
    with _engine("ea_98") as e:
        for B in (1, 33):
            st, joy = cr.synthetic_states(rng, B), cr.synthetic_joy(rng, B)
            obs, act = np.zeros((B, 98), np.float32), np.zeros((B, 12), np.float32)
            with pytest.raises(Go2piError, match="does not serve a policy with observation skip inputs"):
                e.controller_step(st, obs, act, joy=joy)
        assert abs_err(e.run(ps.obs("ea_98", 5)), ps.want("ea_98", 5)) <= TOL  # the engine still serves run()


def test_gru_with_a_skip_is_refused_at_load(tmp_path):
    from go2_onnx_controller_amd import Engine, Go2piError
    from test_cpu_skip import _refusal
    p = tmp_path / "gru_skip.onnx"
    p.write_bytes(_refusal("gru"))
    with pytest.raises(Go2piError, match="a skip Concat in a policy with a GRU or LSTM cell"):
        Engine(str(p), max_batch=8)
