"""The device ABI's buffer contract (include/go2pi.h, "Buffer contract"): a call touches rows
[0, batch) of the buffers it is given and nothing else.

The parity tests compare results; none looks at what a kernel does outside the rows it was
given. The device entry points (go2pi_run_device, go2pi_run_sequence_device,
go2pi_controller_step_device) hand the caller's pointers straight to the kernels, and every
kernel family guards its ragged last tile with a `row < B` of its own. Here every buffer is the
middle of a larger allocation whose other rows hold a sentinel (tests/abi_guard.py), and for
every batched body the planner can name (TABLE; the expected kernel is asserted, so a planner
change cannot drop one silently), at batches 1, 5, 8 (the small-batch paths of the same entry
point), 9 (the first batched launch), 17 (one row into a second tile) and 47 (one short of
three tiles):

* the bands come back bit-identical, every payload element is written and the result is within
  1e-5 of the fp64 oracle (in the model's own metric: _err);
* the result does not depend on what lies behind the caller's last row of obs (NaN or 1e30), and
  obs comes back bit-identical;
* a device-side sequence writes [T][B][out] and nothing else;
* the engine's own hidden rows >= batch keep their bits through every path that advances or
  resets the state;
* an act / obs pointer that is only 4-byte aligned gives bitwise the aligned result (the head
  epilogues' scalar-store form);
* the controller tick writes rows [0, batch) of its seven buffers, leaves state / joy alone,
  and refuses output pointers that break its 16-byte alignment contract before anything runs;
* the host entry points (go2pi_run, go2pi_controller_step) copy back exactly `batch` rows, on
  every resident form.

A device error (a fault, not a wrong answer) ends the session: nothing more is started on a GPU
that has just faulted.
"""
import collections
import functools
import zlib

import numpy as np
import pytest

import abi_guard as ag
from conftest import SHIPPED, abs_err, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
BATCHES = (1, 5, 8, 9, 17, 47)
DEV = "cuda:0"

# model: "shipped", "synth:<synth.MODELS name>", "spec:<policy_specs name>", "tanh_head" (the lean
# shape with an activation on the head), "rnn:<cell>" (the smallest lean recurrent tick of
# tests/test_gpu_rnn_widths.py); opts: Engine options; env: GO2PI_* switches read at create;
# kernel: the prefix Engine.batched_kernel must have; small: Engine.small_kernel (what a batch
# <= 8 is served by; None: the batched kernel, as for every recurrent policy)
Row = collections.namedtuple("Row", "id model opts env kernel small")
LAT, CHAIN = "policy_latency_kernel", "gemv_layer_kernel graph"
RESB = {"GO2PI_RESIDUAL_BATCHED": "1"}

DENSE = [
    # the general body: 8 waves (5 outputs: the scalar store), 4 and 16 waves (30 outputs)
    Row("gen8_relu_o5", "synth:mlp_small_relu", {}, {}, "policy_fused_kernel<8, 0, 0, 0, 0, -1, 0>", LAT),
    Row("gen4_relu_o5", "synth:mlp_small_relu", {"waves": 4}, {}, "policy_fused_kernel<4, 0, 0, 0, 0, -1, 0>", LAT),
    Row("gen4_tanh_o30", "synth:pipe_128_tanh_h2", {"waves": 4}, {"GO2PI_NO_W4": "1"},
        "policy_fused_kernel<4, 0, 0, 0, 0, -1, 0>", LAT),
    Row("gen16_tanh_o30", "synth:pipe_128_tanh_h2", {"waves": 16}, {}, "policy_fused_kernel<16, 0, 0, 0, 0, -1, 0>", LAT),
    # the 4-wave pipeline's general body (a dense program the lean kernel does not take)
    Row("w4gen_h2_o12", "synth:ctl_h3", {}, {}, "policy_fused_kernel<4, 2, 1, 0, 0, -1, 0>", LAT),
    Row("w4gen_noplain", "shipped", {}, {"GO2PI_NO_PLAIN": "1"}, "policy_fused_kernel<4, 2, 1, 3, 0, 1, 3>", LAT),
    # the lean kernel: 2 / 4 / 8 tiles per wave, one and two head tiles
    Row("lean_t2_o12", "shipped", {}, {}, "policy_mlp_kernel<2, 1, 3, 1, 3, 4>", LAT),
    Row("lean_t2_o30", "synth:pipe_128_tanh_h2", {}, {}, "policy_mlp_kernel<2, 2,", LAT),
    Row("lean_t4_o20", "synth:pipe_256_h2", {}, {}, "policy_mlp_kernel<4, 2,", LAT),
    Row("lean_t4_one_hidden", "synth:pipe_one_hidden", {}, {}, "policy_mlp_kernel<4, 1,", LAT),
    Row("lean_t8_o7", "synth:pipe_512_relu", {}, {}, "policy_mlp_kernel<8, 1, 0,", LAT),
    Row("lean_t8_o12", "synth:go2_mlp_512", {}, {}, "policy_mlp_kernel<8, 1, 3, 1, 3, 4>", LAT),
    Row("lean_seq_tanh_head", "tanh_head", {}, {}, "policy_mlp_seq_kernel<4, 1,", LAT),
    # LayerNormalization: the pipeline's LN kernel, and the general body
    Row("ln_pipe_t8", "synth:ln_512_pre", {"ln_batched": True}, {}, "policy_mlp_ln_kernel<8, 1>", CHAIN),
    Row("ln_pipe_t2", "synth:ln_pre_small", {"ln_batched": True}, {}, "policy_mlp_ln_kernel<2, 1>", CHAIN),
    Row("ln_gen_pre", "synth:ln_pre_small", {}, {}, "policy_fused_kernel<8, 0, 0, 0, 0, -1, 0>", CHAIN),
    Row("ln_gen_mixed", "synth:ln_mixed", {}, {}, "policy_fused_kernel<8, 0, 0, 0, 0, -1, 0>", CHAIN),
    # residual connections: the general residual kernel, and the pipeline's
    Row("res_gen_sig", "spec:res_sig", {}, {}, "policy_fused_res_kernel<8>", CHAIN),
    Row("res_gen_simba", "spec:simba_64", {}, {}, "policy_fused_res_kernel<8>", CHAIN),
    Row("res_pipe_t2", "spec:resb_t2_min", {}, RESB, "policy_mlp_res_kernel<2, 1>", CHAIN),
    Row("res_pipe_t2_h2", "spec:resb_t2_post_h2", {}, RESB, "policy_mlp_res_kernel<2, 2>", CHAIN),
    # observation skip inputs: a layer-0 gather, and a skip on a later layer
    Row("skip_l0_gather", "spec:ea_l0slice", {}, {}, "policy_fused_kernel<8, 0, 0, 0, 0, -1, 0>", CHAIN),
    Row("skip_later", "spec:ea_sig", {}, {}, "policy_fused_kernel<8, 0, 0, 0, 0, -1, 0>", CHAIN),
    # the small-batch variants: the chain without a graph, a plain policy on the chain, and the
    # batched kernel from batch 5 on
    Row("chain_no_graph", "synth:ln_pre_small", {"use_graph": False}, {}, "policy_fused_kernel<8, 0,", "gemv_layer_kernel"),
    Row("chain_plain", "shipped", {}, {"GO2PI_SMALL_CHAIN": "1"}, "policy_mlp_kernel<2, 1,", CHAIN),
    Row("small_batch_4", "synth:ln_mixed", {"small_batch": 4}, {}, "policy_fused_kernel<8, 0,", CHAIN),
]

RECURRENT = [
    Row("gru_small", "synth:gru_small", {}, {}, "policy_fused_kernel<8, 0, 0, 0, 0, -1, 0>", None),
    Row("lstm_small", "synth:lstm_small", {}, {}, "policy_fused_kernel<8, 0, 0, 0, 1, -1, 0>", None),
    Row("gru_lbr0_128", "synth:gru_lbr0_128", {}, {}, "policy_fused_kernel<8, 0, 0, 0, 0, -1, 0>", None),
    Row("gru_128", "synth:gru_128", {}, {}, "policy_fused_kernel<4, 4, 1, 0, 0, -1, 0>", None),
    Row("lstm_128", "synth:lstm_128", {}, {}, "policy_fused_kernel<4, 4, 1, 0, 1, -1, 0>", None),
    Row("gru_128_deep", "synth:gru_128_deep", {}, {}, "policy_gru_kernel<4, 1, 2>", None),
    Row("lstm_lean", "rnn:lstm", {}, {}, "policy_lstm_kernel<2, 1, 2>", None),
]

TABLE = DENSE + RECURRENT
_rid = lambda r: r.id  # noqa: E731

# every batched body the planner can name (kernels.hip batched_kernel_name), as prefixes:
# tests/test_cpu_plan.py asserts that each has a row, and every row's kernel of the plan
FAMILIES = ("policy_fused_kernel<4, 0,", "policy_fused_kernel<8, 0,", "policy_fused_kernel<16, 0,",
            "policy_fused_kernel<4, 2,", "policy_fused_kernel<4, 4,", "policy_mlp_kernel<", "policy_mlp_seq_kernel<",
            "policy_gru_kernel<", "policy_lstm_kernel<", "policy_mlp_ln_kernel<", "policy_fused_res_kernel<8>",
            "policy_mlp_res_kernel<")


# --------------------------------------------------------------------------------------
# models, oracle, inputs: computed once, read-only

@functools.lru_cache(maxsize=None)
def _source(model):
    """A path or the ONNX bytes."""
    kind, _, name = model.partition(":")
    if kind == "shipped":
        return SHIPPED
    if kind == "synth":
        from go2_onnx_controller_amd import synth
        return synth.ensure_model(name)
    if kind == "spec":
        import policy_specs as ps
        import res_batched_specs  # noqa: F401  (adds its names to policy_specs' table)
        return ps.path(name)
    if kind == "tanh_head":
        import test_gpu_lean_tick as lean_tick
        return lean_tick._tanh_head_bytes()
    if kind == "rnn":
        import test_gpu_rnn_widths as rw
        return rw.model_bytes(rw.Case(name, 98, 128, (128, 128, 128, 12), (), ""))
    raise KeyError(model)


class Oracle:
    """fp64 evaluation of the model's own graph (tests/ln_ref.py: node by node through
    oracle/onnx_ref.py, LayerNormalization in numpy). A recurrent policy's state is one
    [B, state] array: GRU h; LSTM h | c."""

    def __init__(self, src):
        import ln_ref
        from oracle import onnx_ref
        self.run, self.g = ln_ref.run, onnx_ref.load(src)
        self.state_in = [n for n, _ in self.g.inputs[1:]]
        self.state_out = [n for n, _ in self.g.outputs[1:]]
        self.H = self.g.inputs[1][1][2] if self.state_in else 0

    def step(self, x, st=None):
        feeds = {self.g.inputs[0][0]: np.asarray(x, np.float32)}
        for k, name in enumerate(self.state_in):
            feeds[name] = np.asarray(st, np.float64)[None, :, k * self.H:(k + 1) * self.H]
        out = self.run(self.g, feeds)
        y = out[self.g.outputs[0][0]]
        return (y, np.concatenate([out[n][0] for n in self.state_out], axis=1)) if self.state_in else (y, None)

    def rollout(self, xs, s0=None):
        """xs [T, B, I] from state s0 (zeros if None) -> (actions [T, B, out], final state)."""
        st = s0
        if self.state_in and st is None:
            st = np.zeros((xs.shape[1], self.H * len(self.state_in)))
        ys = []
        for x in xs:
            y, st = self.step(x, st)
            ys.append(y)
        return np.stack(ys), st


@functools.lru_cache(maxsize=None)
def _oracle(model):
    return Oracle(_source(model))


def _err(model):
    """The model's own metric: tests/test_gpu_parity.py and tests/test_gpu_controller.py hold the
    shipped policy (actions of a few units) to max(1, |ref|)-relative error, every synthetic
    model's test to absolute error."""
    return rel_err if model == "shipped" else abs_err


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=None)
def _obs(model, B, T=1):
    """N(0, 1) observations [T, B, in_dim] float32, a fixed function of (model, B, T)."""
    in_dim = _oracle(model).g.inputs[0][1][1]
    x = _rng("obs", model, B, T).standard_normal((T, B, in_dim)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _want(model, B, T=1):
    """The oracle's actions [T, B, out] and final state of _obs(model, B, T) from a zero state."""
    y, st = _oracle(model).rollout(_obs(model, B, T))
    y.setflags(write=False)
    return y, st


# --------------------------------------------------------------------------------------
# engine and launches

def _engine(row, max_batch, monkeypatch, **more):
    from go2_onnx_controller_amd import Engine
    for k, v in row.env.items():
        monkeypatch.setenv(k, v)  # read at engine creation
    e = Engine(_source(row.model), max_batch=max_batch, **{**row.opts, **more})
    assert e.batched_kernel.startswith(row.kernel), (row.id, e.batched_kernel)
    if "small_batch" not in more:
        assert e.small_kernel == (row.small or e.batched_kernel), (row.id, e.small_kernel)
    return e


@functools.lru_cache(maxsize=None)
def _stream():
    import torch
    return torch.cuda.Stream(device=DEV)  # the caller's stream: not the default one


def _finish(e):
    """Wait for the caller's stream and the engine; a device error ends the session."""
    from go2_onnx_controller_amd.engine import Go2piError
    try:
        _stream().synchronize()
        e.sync()
    except Go2piError as ex:
        if ex.code != -3:
            raise
        pytest.exit(f"device error, stopping: {ex}", returncode=3)
    except RuntimeError as ex:
        pytest.exit(f"device error, stopping: {ex}", returncode=3)


def _launch(e, obs, act, B, T=None):
    """run_device (T None) or run_sequence_device on the caller's stream, from a zero state."""
    import torch
    if e.hidden_dim:
        e.reset_hidden()
    torch.cuda.synchronize()  # the uploads (default stream) are in front of the launch
    if T is None:
        e.run_device(obs.data_ptr(), act.data_ptr(), B, _stream().cuda_stream)
    else:
        e.run_sequence_device(obs.data_ptr(), act.data_ptr(), T, B, _stream().cuda_stream)
    _finish(e)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# --------------------------------------------------------------------------------------
# 1. confinement and parity; 2. independence of what lies behind the batch

@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("row", TABLE, ids=_rid)
def test_confinement_and_parity(row, B, monkeypatch):
    import torch
    with _engine(row, B, monkeypatch) as e:
        obs = _dev(_obs(row.model, B)[0])
        whole, act = ag.banded(B, e.out_dim, torch.float32, device=DEV)
        _launch(e, obs, act, B)
        ag.assert_bands_intact(whole, ag.FRONT, B, what=f"{row.id} B={B} act")
        ag.assert_all_written(act, what=f"{row.id} B={B} act")
        err = _err(row.model)(act.cpu().numpy(), _want(row.model, B)[0][0])
        print(f"{row.id} B={B}: {e.batched_kernel if B > 8 else e.small_kernel} err {err:.3g}")
        assert err <= TOL
        if e.hidden_dim:
            assert abs_err(e.get_hidden(B), _want(row.model, B)[1]) <= TOL


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("row", TABLE, ids=_rid)
def test_independent_of_rows_behind_the_batch(row, B, monkeypatch):
    """The rows of obs in front of and behind the batch hold NaN, then 1e30: the actions are
    bitwise the same, and obs (payload and bands) is what was uploaded."""
    import torch
    with _engine(row, B, monkeypatch) as e:
        obs_whole, obs = ag.banded(B, e.in_dim, torch.float32, device=DEV)
        obs.copy_(_dev(_obs(row.model, B)[0]))
        got = []
        for fill in (None, 1e30):
            if fill is not None:
                ag.fill_bands(obs_whole, ag.FRONT, B, fill)
            uploaded = ag.bits(obs_whole)
            whole, act = ag.banded(B, e.out_dim, torch.float32, device=DEV)
            _launch(e, obs, act, B)
            ag.assert_bits_equal(obs_whole, uploaded, what=f"{row.id} B={B} obs (bands {fill})")
            ag.assert_bands_intact(whole, ag.FRONT, B, what=f"{row.id} B={B} act")
            ag.assert_all_written(act, what=f"{row.id} B={B} act")
            got.append(ag.bits(act))
        ag.assert_bits_equal(got[1], got[0], what=f"{row.id} B={B} act with 1e30 behind the batch")
        assert _err(row.model)(act.cpu().numpy(), _want(row.model, B)[0][0]) <= TOL


# --------------------------------------------------------------------------------------
# 3. sequences

T_SEQ = 3
# (small_batch = -1: the entry point's batch <= 8 launches are the batched kernel's too, which
# the bitwise comparison with the sequence's steps needs)
SEQ_DENSE = [r for r in DENSE if r.id in ("lean_t4_o20", "lean_seq_tanh_head")]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("row", SEQ_DENSE + RECURRENT, ids=_rid)
def test_sequence_confinement(row, B, monkeypatch):
    import torch
    dense = row in SEQ_DENSE
    with _engine(row, B, monkeypatch, **({"small_batch": -1} if dense else {})) as e:
        xs = _obs(row.model, B, T_SEQ)
        want_y, want_st = _want(row.model, B, T_SEQ)
        obs_whole, _ = ag.banded(T_SEQ * B, e.in_dim, torch.float32, device=DEV)
        obs = obs_whole[ag.FRONT:ag.FRONT + T_SEQ * B].view(T_SEQ, B, e.in_dim)
        obs.copy_(_dev(xs))
        uploaded = ag.bits(obs_whole)
        whole, flat = ag.banded(T_SEQ * B, e.out_dim, torch.float32, device=DEV)  # [T][B][out] with bands
        _launch(e, obs, flat, B, T=T_SEQ)
        ag.assert_bands_intact(whole, ag.FRONT, T_SEQ * B, what=f"{row.id} B={B} act")
        ag.assert_all_written(flat, what=f"{row.id} B={B} act")
        ag.assert_bits_equal(obs_whole, uploaded, what=f"{row.id} B={B} obs")
        seq = flat.cpu().numpy().reshape(T_SEQ, B, e.out_dim)
        for t in range(T_SEQ):
            assert abs_err(seq[t], want_y[t]) <= TOL, t
        if e.hidden_dim:
            assert abs_err(e.get_hidden(B), want_st) <= TOL
        else:
            for t in range(T_SEQ):
                w1, a1 = ag.banded(B, e.out_dim, torch.float32, device=DEV)
                _launch(e, obs[t], a1, B)
                ag.assert_bands_intact(w1, ag.FRONT, B)
                ag.assert_bits_equal(a1, seq[t], what=f"{row.id} B={B} step {t}: run_device against the sequence")


# --------------------------------------------------------------------------------------
# recurrent state: the engine's own hidden rows >= batch

SLACK = 48


def _state0(model, rows, width):
    s = (0.5 * _rng("state", model, rows).standard_normal((rows, width))).astype(np.float32)
    s.setflags(write=False)
    return s


def _check_state(e, row, B, s0, want_st, what):
    st = e.get_hidden(e.max_batch)
    ag.assert_bits_equal(st[B:], s0[B:], what=f"{row.id} B={B} {what}: hidden rows >= batch")
    assert abs_err(st[:B], want_st) <= TOL, what


@pytest.mark.parametrize("path", ["run", "run_device", "run_sequence_device"])
@pytest.mark.parametrize("B", [5, 17, 47])
@pytest.mark.parametrize("row", RECURRENT, ids=_rid)
def test_hidden_rows_behind_the_batch(row, B, path, monkeypatch):
    """All max_batch = B + 48 hidden rows set, B rows run: the rows behind keep their bits, the
    rows run hold the oracle's state (GRU h; LSTM h | c)."""
    import torch
    T = T_SEQ if path == "run_sequence_device" else 1
    with _engine(row, B + SLACK, monkeypatch) as e:
        s0 = _state0(row.model, B + SLACK, e.hidden_dim)
        xs = _obs(row.model, B, T)
        want_y, want_st = _oracle(row.model).rollout(xs, s0[:B])
        e.set_hidden(s0)
        ag.assert_bits_equal(e.get_hidden(B + SLACK), s0)
        if path == "run":
            y = e.run(xs[0])[None]
        else:
            obs = _dev(xs)
            whole, flat = ag.banded(T * B, e.out_dim, torch.float32, device=DEV)
            torch.cuda.synchronize()
            if path == "run_device":
                e.run_device(obs.data_ptr(), flat.data_ptr(), B, _stream().cuda_stream)
            else:
                e.run_sequence_device(obs.data_ptr(), flat.data_ptr(), T, B, _stream().cuda_stream)
            _finish(e)
            ag.assert_bands_intact(whole, ag.FRONT, T * B, what=f"{row.id} B={B} act")
            y = flat.cpu().numpy().reshape(T, B, e.out_dim)
        assert abs_err(y, want_y) <= TOL
        _check_state(e, row, B, s0, want_st, path)


# what serves a host run() at batch <= 8 with resident_ms > 0 (plan.cpp plan_resident): the
# multi-workgroup resident kernel's recurrent form where the cell fits it, else a launch
RESIDENT_RNN = {"gru_128": "policy_resident_kernel", "lstm_128": "policy_resident_kernel",
                "gru_128_deep": "policy_resident_kernel", "lstm_lean": "policy_resident_kernel"}


@pytest.mark.parametrize("B", [1, 5, 8])
@pytest.mark.parametrize("row", RECURRENT, ids=_rid)
def test_hidden_rows_behind_the_batch_resident(row, B, monkeypatch):
    """The same through host run() with resident_ms = 500: two ticks, the second served by the
    kernel the first one started."""
    with _engine(row, B + SLACK, monkeypatch, resident_ms=500) as e:
        if row.id in RESIDENT_RNN:
            assert e.resident_kernel.startswith(RESIDENT_RNN[row.id]), e.resident_kernel
        s0 = _state0(row.model, B + SLACK, e.hidden_dim)
        xs = _obs(row.model, B, 2)
        want_y, want_st = _oracle(row.model).rollout(xs, s0[:B])
        e.set_hidden(s0)
        whole, act = ag.banded_np(B, e.out_dim, np.float32)
        for t in range(2):
            e.run_ptr(xs[t].ctypes.data, act.ctypes.data, B)
            ag.assert_bands_intact(whole, ag.FRONT, B, what=f"{row.id} B={B} act")
            assert abs_err(act, want_y[t]) <= TOL, t
        _check_state(e, row, B, s0, want_st, "resident run")


def _masks(B):
    alt = np.arange(B) % 2 == 0
    ends = np.zeros(B, bool)
    ends[:2] = ends[-3:] = True
    one = np.zeros(B, bool)
    one[B // 2] = True
    return {"alternating": alt, "runs_at_both_ends": ends, "all_zero": np.zeros(B, bool), "single_row": one}


@pytest.mark.parametrize("B", [5, 17, 47])
@pytest.mark.parametrize("row", RECURRENT, ids=_rid)
def test_reset_hidden_mask_is_exact(row, B, monkeypatch):
    """reset_hidden(mask, batch) zeroes exactly the masked rows; unmasked rows and rows >= batch
    keep their bits."""
    with _engine(row, B + SLACK, monkeypatch) as e:
        s0 = _state0(row.model, B + SLACK, e.hidden_dim)
        for name, m in _masks(B).items():
            e.set_hidden(s0)
            e.reset_hidden(m.astype(np.uint8), B)
            want = s0.copy()
            want[:B][m] = 0.0
            ag.assert_bits_equal(e.get_hidden(B + SLACK), want, what=f"{row.id} B={B} mask {name}")


@pytest.mark.parametrize("B", [5, 17, 47])
def test_hidden_rows_behind_the_batch_controller(B, monkeypatch):
    """gru_ctl through the host controller tick."""
    from oracle import controller_ref as cr
    row = Row("gru_ctl", "synth:gru_ctl", {}, {}, "policy_fused_kernel<4, 2, 1, 0, 0, -1, 0>", None)
    rng = _rng("gru_ctl", B)
    with _engine(row, B + SLACK, monkeypatch) as e:
        s0 = _state0(row.model, B + SLACK, e.hidden_dim)
        e.set_hidden(s0)
        st, joy = cr.synthetic_states(rng, B), cr.synthetic_joy(rng, B)
        obs, act = np.zeros((B, e.in_dim), np.float32), np.zeros((B, 12), np.float32)
        e.controller_step(st, obs, act, joy=joy)
        y, want_st = _oracle(row.model).step(obs, s0[:B])
        a_ref = cr.post_process(y, joy)[0]
        assert rel_err(act, a_ref) <= TOL
        _check_state(e, row, B, s0, want_st, "controller_step")


# --------------------------------------------------------------------------------------
# alignment: the head epilogues' scalar-store form (act only 4-byte aligned)

_BY_ID = {r.id: r for r in TABLE}
ALIGN_ROWS = [
    _BY_ID["w4gen_h2_o12"],  # fused_impl.hpp: the pipeline's general body
    _BY_ID["lean_t2_o12"],   # fused_impl.hpp: the lean kernel
    _BY_ID["ln_pipe_t2"],    # w4ln_impl.hpp: the LN pipeline
    Row("res_pipe_t2_adj", "spec:resb_t2_adjacent", {}, RESB, "policy_mlp_res_kernel<2, 1>", CHAIN),  # ... its residual form
    _BY_ID["gru_128_deep"],  # the lean recurrent tick
]


@pytest.mark.parametrize("B", [17, 47])
@pytest.mark.parametrize("row", ALIGN_ROWS, ids=_rid)
def test_unaligned_pointers_give_the_aligned_result(row, B, monkeypatch):
    """act at base + 1, 2, 3 floats and obs at base + 1 float: only the store instruction
    differs, so the actions are bitwise those of the 16-byte-aligned call."""
    import torch
    with _engine(row, B, monkeypatch) as e:
        assert e.out_dim == 12  # a 48-byte row: the 16-byte store is the aligned call's form
        x = _dev(_obs(row.model, B)[0])
        obs_whole, obs = ag.banded(B, e.in_dim, torch.float32, device=DEV)
        obs.copy_(x)
        whole, act = ag.banded(B, 12, torch.float32, device=DEV)
        assert obs.data_ptr() % 16 == 0 and act.data_ptr() % 16 == 0
        _launch(e, obs, act, B)
        aligned = ag.bits(act)
        assert _err(row.model)(act.cpu().numpy(), _want(row.model, B)[0][0]) <= TOL
        obs_whole, _ = ag.banded(B, e.in_dim, torch.float32, device=DEV)
        obs = ag.shifted(obs_whole, ag.FRONT, B, 1)
        obs.copy_(x)
        uploaded = ag.bits(obs_whole)
        for k in (1, 2, 3):
            whole, _ = ag.banded(B, 12, torch.float32, device=DEV)
            act = ag.shifted(whole, ag.FRONT, B, k)
            assert act.data_ptr() % 16 == 4 * k and obs.data_ptr() % 16 == 4
            _launch(e, obs, act, B)
            ag.assert_bands_intact(whole, ag.FRONT, B, shift=k, what=f"{row.id} B={B} act + {k} floats")
            ag.assert_bits_equal(act, aligned, what=f"{row.id} B={B} act + {k} floats against the aligned call")
            ag.assert_bits_equal(obs_whole, uploaded, what=f"{row.id} B={B} obs + 1 float")


# --------------------------------------------------------------------------------------
# the controller tick, device path

CtlRow = collections.namedtuple("CtlRow", "id model env hist")
CTL_ROWS = [
    CtlRow("shipped_lean_tick", "shipped", {}, 2),
    CtlRow("shipped_general", "shipped", {"GO2PI_CTL_GENERAL": "1"}, 2),
    CtlRow("ctl_h3_deep", "synth:ctl_h3_deep", {}, 3),   # the lean tick, K padded to 64
    CtlRow("ctl_h1", "synth:ctl_h1", {}, 1),             # B = 5: the single launch
    CtlRow("gru_ctl", "synth:gru_ctl", {}, 2),
]
CTL_BATCHES = (5, 17, 47)


class CtlBuffers:
    """The tick's eight buffers, each the middle of a banded allocation on the GPU."""
    SPEC = (("state", 36, "float32"), ("joy", 5, "float32"), ("obs", None, "float32"), ("action", 12, "float32"),
            ("q_des", 12, "float64"), ("kp", 12, "float64"), ("kd", 12, "float64"), ("status", 1, "int32"))

    def __init__(self, B, in_dim):
        import torch
        self.B, self.whole, self.view = B, {}, {}
        for name, width, dt in self.SPEC:
            self.whole[name], self.view[name] = ag.banded(B, width or in_dim, getattr(torch, dt), device=DEV)
        self.view["obs"].zero_()
        self.view["action"].zero_()

    def ptrs(self, skip=(), shift=None):
        """The eight pointers in the entry point's order (skip: passed as NULL; shift: that
        output's pointer one element further)."""
        out = []
        for name, _, _ in self.SPEC:
            v = self.view[name]
            out.append(None if name in skip else v.data_ptr() + (v.element_size() if name == shift else 0))
        return out

    def host(self, name):
        return self.view[name].cpu().numpy()

    def outs(self):
        return (self.host("q_des"), self.host("kp"), self.host("kd"), self.host("status").reshape(-1))

    def assert_bands(self, what, skip=()):
        for name, _, _ in self.SPEC:
            ag.assert_bands_intact(self.whole[name], ag.FRONT, self.B, what=f"{what} {name}")
            if name in skip:  # a NULL output: its buffer was not passed at all
                assert np.all(ag.bits(self.view[name]) == ag.sentinel(self.view[name].dtype)), name


def _ctl_policy(crow, B):
    """obs -> the policy's fp64 output; a recurrent policy's state advances once per call."""
    orc = _oracle(crow.model)
    state = {"st": None}

    def policy_y(obs):
        if not orc.state_in:
            return orc.step(obs)[0]
        st = np.zeros((B, orc.H)) if state["st"] is None else state["st"]
        y, state["st"] = orc.step(obs, st)
        return y
    return policy_y


def _ctl_engine(crow, B, monkeypatch):
    from go2_onnx_controller_amd import Engine
    for k, v in crow.env.items():
        monkeypatch.setenv(k, v)
    e = Engine(_source(crow.model), max_batch=B)
    assert e.ctl_history() == crow.hist
    if e.hidden_dim:
        e.reset_hidden()
    return e


def _tick(e, bufs, st, joy, skip=(), shift=None):
    import torch
    bufs.view["state"].copy_(_dev(st))
    bufs.view["joy"].copy_(_dev(joy))
    torch.cuda.synchronize()
    e.controller_step_device(*bufs.ptrs(skip, shift), bufs.B, _stream().cuda_stream)
    _finish(e)


@pytest.mark.parametrize("B", CTL_BATCHES)
@pytest.mark.parametrize("crow", CTL_ROWS, ids=_rid)
def test_controller_tick_device_confinement(crow, B, monkeypatch):
    """Three ticks: every buffer's bands intact, state / joy bit-identical, every output as
    tests/test_gpu_controller.py's _check requires of the host path."""
    from oracle import controller_ref as cr
    from test_gpu_controller import _check
    rng = _rng("ctl", crow.id, B)
    policy_y = _ctl_policy(crow, B)
    with _ctl_engine(crow, B, monkeypatch) as e:
        bufs = CtlBuffers(B, e.in_dim)
        for t in range(3):
            st, joy = cr.synthetic_states(rng, B, upright=t % 2 == 0), cr.synthetic_joy(rng, B)
            o0, a0 = bufs.host("obs"), bufs.host("action")
            _tick(e, bufs, st, joy)
            bufs.assert_bands(f"{crow.id} B={B} tick {t}")
            for name in ("q_des", "kp", "kd", "status"):
                ag.assert_all_written(bufs.view[name], what=name)
            ag.assert_bits_equal(bufs.view["state"], st, what="state")
            ag.assert_bits_equal(bufs.view["joy"], joy, what="joy")
            _check(st, joy, o0, a0, bufs.host("obs"), bufs.host("action"), bufs.outs(), crow.hist, policy_y)


@pytest.mark.parametrize("skip", [("q_des", "kd", "status"), ("status",)], ids=["only_kp", "all_but_status"])
@pytest.mark.parametrize("B", CTL_BATCHES)
@pytest.mark.parametrize("crow", CTL_ROWS[:3], ids=_rid)
def test_controller_tick_optional_outputs(crow, B, skip, monkeypatch):
    """Outputs individually NULL: the ones passed are bitwise those of the all-outputs call, the
    ones not passed keep their sentinel."""
    from oracle import controller_ref as cr
    rng = _rng("ctl-optional", crow.id, B)
    st, joy = cr.synthetic_states(rng, B), cr.synthetic_joy(rng, B)
    with _ctl_engine(crow, B, monkeypatch) as e:
        full, part = CtlBuffers(B, e.in_dim), CtlBuffers(B, e.in_dim)
        _tick(e, full, st, joy)
        _tick(e, part, st, joy, skip=skip)
        full.assert_bands(f"{crow.id} B={B} all outputs")
        part.assert_bands(f"{crow.id} B={B} without {skip}", skip=skip)
        for name, _, _ in CtlBuffers.SPEC:
            if name not in skip:
                ag.assert_bits_equal(part.view[name], full.view[name], what=f"{name} without {skip}")


@pytest.mark.parametrize("B", [5, 17])
@pytest.mark.parametrize("crow", CTL_ROWS[:2], ids=_rid)
def test_controller_tick_refuses_unaligned_outputs(crow, B, monkeypatch):
    """go2pi.h: action needs 16-byte alignment (one float4 store per lane), q_des / kp / kd too
    (two doubles per store). A pointer one element off is refused with GO2PI_E_INVALID and a
    message that names it, before anything is enqueued: every buffer keeps its bits. The
    aligned call that follows is served."""
    from go2_onnx_controller_amd import Go2piError
    from oracle import controller_ref as cr
    from test_gpu_controller import _check
    rng = _rng("ctl-align", crow.id, B)
    st, joy = cr.synthetic_states(rng, B), cr.synthetic_joy(rng, B)
    with _ctl_engine(crow, B, monkeypatch) as e:
        bufs = CtlBuffers(B, e.in_dim)
        bufs.view["state"].copy_(_dev(st))
        bufs.view["joy"].copy_(_dev(joy))
        before = {name: ag.bits(w) for name, w in bufs.whole.items()}
        for name in ("action", "q_des", "kp", "kd"):
            with pytest.raises(Go2piError) as ex:
                _tick(e, bufs, st, joy, shift=name)
            assert ex.value.code == -1 and name in str(ex.value) and "16" in str(ex.value), str(ex.value)
            for n, w in bufs.whole.items():
                ag.assert_bits_equal(w, before[n], what=f"{n} after the refused call ({name} + 1 element)")
        o0, a0 = bufs.host("obs"), bufs.host("action")
        _tick(e, bufs, st, joy)
        bufs.assert_bands(f"{crow.id} B={B} aligned call")
        _check(st, joy, o0, a0, bufs.host("obs"), bufs.host("action"), bufs.outs(), crow.hist, _ctl_policy(crow, B))


# --------------------------------------------------------------------------------------
# host buffers: go2pi_run and go2pi_controller_step copy back exactly `batch` rows

# every resident form the suite switches between (tests/test_gpu_resident.py,
# tests/test_gpu_resident_wide.py, tests/test_gpu_controller.py), and no resident kernel
HOST_FORMS = {
    "act1": ("shipped", {}, 500, "policy_act1_kernel"),
    "r1w": ("shipped", {"GO2PI_RES_R1W": "1"}, 500, "policy_resident1_kernel"),
    "multi": ("shipped", {"GO2PI_RES_MULTI": "1"}, 500, "policy_resident_kernel"),
    "wide": ("synth:wide_256_3", {}, 500, ("policy_wide_kernel", "policy_resident_kernel")),  # (no large BAR: the latter)
    "launch": ("shipped", {}, 0, "none"),
}


# batches 1, 3, 8 on every form, and one batched case (the resident forms serve batch <= 8 only)
HOST_CASES = [(f, B) for f in HOST_FORMS for B in (1, 3, 8)] + [("launch", 17)]


@pytest.mark.parametrize("form,B", HOST_CASES)
def test_host_run_confinement(form, B, monkeypatch):
    """run_ptr with act the middle of a larger numpy array, twice (the second call is served by
    the resident kernel the first started); B = 17: the batched launch through d_act."""
    from go2_onnx_controller_amd import Engine
    model, env, res, resident = HOST_FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with Engine(_source(model), max_batch=max(B, 8), resident_ms=res) as e:
        assert e.resident_kernel.startswith(resident), e.resident_kernel
        for k in range(2):
            x = _obs(model, B, 2)[k]
            obs_whole, obs = ag.banded_np(B, e.in_dim, np.float32)
            obs[...] = x
            uploaded = ag.bits(obs_whole)
            whole, act = ag.banded_np(B, e.out_dim, np.float32)
            e.run_ptr(obs.ctypes.data, act.ctypes.data, B)
            ag.assert_bands_intact(whole, ag.FRONT, B, what=f"{form} B={B} act")
            ag.assert_all_written(act, what=f"{form} B={B} act")
            ag.assert_bits_equal(obs_whole, uploaded, what=f"{form} B={B} obs")
            assert _err(model)(act, _want(model, B, 2)[0][k]) <= TOL


@pytest.mark.parametrize("form,B", [c for c in HOST_CASES if c[0] != "wide"])
def test_host_controller_step_confinement(form, B, monkeypatch):
    """go2pi_controller_step with every array a view of a larger one, three ticks."""
    from go2_onnx_controller_amd import Engine
    from go2_onnx_controller_amd import engine as eng
    from oracle import controller_ref as cr
    from test_gpu_controller import _check
    model, env, res, resident = HOST_FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = _rng("host-ctl", form, B)
    policy_y = _ctl_policy(CtlRow(form, model, env, 2), B)
    spec = [(n, w, np.uint32 if d == "int32" else np.dtype(d)) for n, w, d in CtlBuffers.SPEC]
    with Engine(_source(model), max_batch=max(B, 8), resident_ms=res) as e:
        whole, view = {}, {}
        for name, width, dt in spec:
            whole[name], view[name] = ag.banded_np(B, width or e.in_dim, dt)
        view["obs"][...] = 0
        view["action"][...] = 0
        for t in range(3):
            st, joy = cr.synthetic_states(rng, B, upright=t % 2 == 0), cr.synthetic_joy(rng, B)
            view["state"][...], view["joy"][...] = st, joy
            o0, a0 = view["obs"].copy(), view["action"].copy()
            eng._check(eng.lib().go2pi_controller_step(e._h, *[view[n].ctypes.data for n, _, _ in spec], B))
            for name, _, _ in spec:
                ag.assert_bands_intact(whole[name], ag.FRONT, B, what=f"{form} B={B} tick {t} {name}")
            ag.assert_bits_equal(view["state"], st, what="state")
            ag.assert_bits_equal(view["joy"], joy, what="joy")
            for name in ("q_des", "kp", "kd", "status"):
                ag.assert_all_written(view[name], what=name)
            outs = (view["q_des"], view["kp"], view["kd"], view["status"].reshape(-1))
            _check(st, joy, o0, a0, view["obs"], view["action"], outs, 2, policy_y)
