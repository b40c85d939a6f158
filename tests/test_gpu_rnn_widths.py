"""The pipelined recurrent cell (fused_impl.hpp w4_gru / w4_lstm) at every observation width
and in every instantiation that serves it, against the fp64 oracle.

The cell walks the concatenated [x | h] axis in 16-column chunks through a 4-slot register
ring (w4_cell_contract, the one chunk schedule both cells call). Which x chunks it walks, and on which slot it starts, depends on Cxe = ceil(I / 16):

* the ring starts on slot 1 when Cxe % 4 == 3 (so that the h chunks start on slot 0), else 0;
* on slot 1 the leading group of three chunks is followed by more x chunks (Cxe > 3) or by h;
* the 4-chunk x loop runs ceil((Cxe - 4 - start) / 4) times, start = 3 on slot 1 and else 0:
  not at all below Cxe = 5.

The lean recurrent tick (policy_gru_kernel / policy_lstm_kernel, w4_gru_body) stages the
observation with one direct-to-LDS load per 64-column group (nch = ceil(I / 64) of them), the
general 4-wave body (policy_fused_kernel<4, ...>) with its own loop over the same groups, and a
device-side sequence stages again on every step. The widths below were chosen to enter every
one of these paths (the older tests know I = 30 and 48 only: Cxe = 2 and 3, nch = 1):

    I       1  16  17  49  64  65  98 128 150 176 245 256 512
    Cxe     1   1   2   4   4   5   7   8  10  11  16  16  32
    x loop  0   0   0   0   0   1   0   1   2   1   3   3   7
    nch     1   1   1   1   1   2   2   2   3   3   4   4   8

I = 1 clamps every staging lane to element 0; I = 49, 65 and 245 give rows whose byte address
is not 16-aligned; I = 128 / 256 / 512 fill the LDS row of a 128- / 256- / 512-wide head.

CASES is the table: (cell, I, H, head widths, switches) and the kernel the engine must report.
tests/test_cpu_plan.py imports it and asserts the same names of the plan, without a GPU.

Tolerance: 1e-5 absolute on actions, h and c per tick, as tests/test_gpu_gru.py and
tests/test_gpu_lstm.py. test_tolerance_headroom (no GPU) shows that a straightforward float32
evaluation of these wider cells stays within a quarter of it, so the bound asks nothing of
these shapes that float32 cannot give; test_probe_sees_x_chunks (no GPU) shows that a chunk
fault (two x chunks exchanged, one dropped, an x chunk met with an h chunk's weights) moves h'
by more than 1000 times the bound on the very inputs the GPU tests use.
"""
import collections
import itertools

import numpy as np
import pytest

import probe_models as pm
from conftest import abs_err

TOL = 1e-5
BATCHES = [33, 1, 16, 17, 15]
T = 3
B0 = BATCHES[0]     # the batch of the extra tick, the sequences and the non-finite rows

Case = collections.namedtuple("Case", "cell I H head env kernel")

# the lean recurrent tick: policy_gru_kernel / policy_lstm_kernel<tiles per wave, head tiles,
# hidden tiles per wave> (head widths, H, observation widths, the template arguments)
_LEAN = [
    ((128, 128, 128, 12), 128, (1, 16, 17, 64, 65, 98, 128), "<2, 1, 2>"),
    ((128, 128, 128, 20), 128, (98,), "<2, 2, 2>"),
    ((256, 256, 256, 12), 128, (49, 150, 176, 245), "<4, 1, 2>"),
    ((256, 256, 256, 12), 256, (98, 256), "<4, 1, 4>"),
    ((256, 256, 256, 20), 256, (245,), "<4, 2, 4>"),
    ((512, 512, 512, 12), 128, (98,), "<8, 1, 2>"),
    ((512, 512, 512, 12), 256, (98, 245, 512), "<8, 1, 4>"),
]
# the general 4-wave body: policy_fused_kernel<waves, tiles per wave, head tiles, layer-0 chunks
# mod 4, cell (0 GRU, 1 LSTM), activation (1 Elu, -1 run time), hidden layers (3, 0 run time)>
_GENERAL_ENV = (("GO2PI_GRU_GENERAL", "1"),)
_GENERAL = [
    ((256, 256, 256, 12), 128, 65, _GENERAL_ENV, "policy_fused_kernel<4, 4, 1, 0, {rnn}, 1, 3>"),
    ((256, 256, 256, 12), 128, 98, _GENERAL_ENV, "policy_fused_kernel<4, 4, 1, 0, {rnn}, 1, 3>"),
    ((256, 256, 256, 12), 128, 176, _GENERAL_ENV, "policy_fused_kernel<4, 4, 1, 0, {rnn}, 1, 3>"),
    # the observation is wider than the head: an LDS row of 260 floats, so not the lean tick
    ((128, 128, 128, 12), 128, 245, (), "policy_fused_kernel<4, 2, 1, 0, {rnn}, 1, 3>"),
    # two hidden layers: the run-time forms (LSTM: the cell without the layer-0 prefill)
    ((256, 256, 12), 128, 98, (), "policy_fused_kernel<4, 4, 1, 0, {rnn}, -1, 0>"),
]

CASES = []
for _cell in ("gru", "lstm"):
    for _head, _H, _Is, _targs in _LEAN:
        CASES += [Case(_cell, _I, _H, _head, (), f"policy_{_cell}_kernel{_targs}") for _I in _Is]
    CASES += [Case(_cell, _I, _H, _head, _env, _k.format(rnn=int(_cell == "lstm")))
              for _head, _H, _I, _env, _k in _GENERAL]


def is_lean(case):
    return not case.kernel.startswith("policy_fused_kernel")


def plan_scalars(case):
    """(w4_gru_lean, lds_stride, in_pad) of the case's plan: the cell's x axis is padded to whole
    64-column groups, and the LDS row holds the widest of the observation, h and the head's
    layers, plus 4 floats."""
    in_pad = -(-case.I // 64) * 64
    return int(is_lean(case)), max(in_pad, case.H, case.head[0]) + 4, in_pad


def _id(case):
    head = f"{case.head[0]}x{len(case.head) - 1}_{case.head[-1]}"
    return f"{case.cell}_i{case.I}_h{case.H}_{head}" + ("" if is_lean(case) else "_general")


def _seed(case):
    return 4000 + case.I + 7 * case.H + 3 * case.head[0] + case.head[-1] + len(case.head)


def model_bytes(case):
    from go2_onnx_controller_amd import synth
    if case.cell == "gru":
        return synth.gru_model_bytes(I=case.I, H=case.H, head=case.head, seed=_seed(case), lbr=1)
    return synth.lstm_model_bytes(I=case.I, H=case.H, head=case.head, seed=_seed(case))


def _sw(case):
    return case.H * (2 if case.cell == "lstm" else 1)   # state floats per robot: h, or h | c


_inputs_cache = {}


def _inputs(case):
    """(one [T, B, I] float32 observation array per batch of BATCHES, the [B0, state] start of
    the extra tick, its [B0, I] observation): standard normal, the state N(0, 0.5^2). Depends on
    (I, H, cell) alone, read-only."""
    key = (case.cell, case.I, case.H)
    if key not in _inputs_cache:
        r = np.random.default_rng(9000 + case.I + 5 * case.H + (case.cell == "lstm"))
        xs = {B: r.standard_normal((T, B, case.I)).astype(np.float32) for B in BATCHES}
        s0 = (0.5 * r.standard_normal((B0, _sw(case)))).astype(np.float32)
        x1 = r.standard_normal((B0, case.I)).astype(np.float32)
        for a in list(xs.values()) + [s0, x1]:
            a.setflags(write=False)
        _inputs_cache[key] = (xs, s0, x1)
    return _inputs_cache[key]


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("rnn_widths")


_graphs = {}


def _graph(case, model_dir):
    """(onnx bytes, the oracle's graph): the file written once per case."""
    from oracle import onnx_ref
    key = case._replace(env=(), kernel="")
    if key not in _graphs:
        data = model_bytes(case)
        p = model_dir / (_id(key) + ".onnx")
        p.write_bytes(data)
        _graphs[key] = (data, onnx_ref.load(str(p)))
    return _graphs[key]


def _oracle(g, case, xs, s0=None):
    """fp64 rollout of xs [T, B, I] from state s0 [B, state] (zeros if None): the actions
    [T, B, out] and the state after every tick [T, B, state] (LSTM: h | c)."""
    from oracle import onnx_ref
    H, B = case.H, xs.shape[1]
    st = np.zeros((B, _sw(case))) if s0 is None else s0.astype(np.float64)
    ys, sts = [], []
    with np.errstate(all="ignore"):    # (the non-finite rows)
        for x in xs:
            feeds = {"observation": x.astype(np.float64), "h_in": st[None, :, :H]}
            if case.cell == "lstm":
                feeds["c_in"] = st[None, :, H:]
            r = onnx_ref.run(g, feeds)
            st = r["h_out"][0] if case.cell == "gru" else np.concatenate([r["h_out"][0], r["c_out"][0]], axis=1)
            ys.append(r["action"])
            sts.append(st)
    return np.stack(ys), np.stack(sts)


_refs = {}


def _ref(case, model_dir):
    """(per batch: the oracle's (actions, states) of the zero-state rollout; the extra tick's)."""
    key = case._replace(env=(), kernel="")
    if key not in _refs:
        _, g = _graph(case, model_dir)
        xs, s0, x1 = _inputs(case)
        roll = {B: _oracle(g, case, xs[B]) for B in BATCHES}
        extra = _oracle(g, case, x1[None], s0)
        for a in [a for pair in list(roll.values()) + [extra] for a in pair]:
            a.setflags(write=False)
        _refs[key] = (roll, extra)
    return _refs[key]


# --------------------------------------------------------------------------------------
# the cell and the head restated in numpy, from the generator's own tensors (no GPU)

def _sigmoid(x):
    return 1 / (1 + np.exp(-x))


def _params(case, dt):
    """(W [G H, I], R [G H, H], Wb + Rb per gate or (GRU) the candidate's two biases apart,
    the head's [(W, b)]) as dtype dt."""
    from go2_onnx_controller_amd import synth
    H = case.H
    W, R, Bv = (synth.gru_params if case.cell == "gru" else synth.lstm_params)(case.I, H, _seed(case))
    head = [(w.astype(dt), b.astype(dt)) for w, b in synth.mlp_layers((H,) + tuple(case.head), _seed(case), 200)]
    return W[0].astype(dt), R[0].astype(dt), Bv[0].astype(dt), head


def _cell(case, W, R, Bv, x, st):
    """One tick of the cell in the dtype of its arguments: the new state [B, state]."""
    H = case.H
    h = st[:, :H]
    if case.cell == "gru":   # gates z, r, h; linear_before_reset = 1
        gx, gh = x @ W.T + Bv[:3 * H], h @ R.T + Bv[3 * H:]
        z = _sigmoid(gx[:, :H] + gh[:, :H])
        r = _sigmoid(gx[:, H:2 * H] + gh[:, H:2 * H])
        n = np.tanh(gx[:, 2 * H:] + r * gh[:, 2 * H:])
        return (1 - z) * n + z * h
    g = x @ W.T + h @ R.T + (Bv[:4 * H] + Bv[4 * H:])   # gates i, o, f, c
    c = _sigmoid(g[:, 2 * H:3 * H]) * st[:, H:] + _sigmoid(g[:, :H]) * np.tanh(g[:, 3 * H:])
    return np.concatenate([_sigmoid(g[:, H:2 * H]) * np.tanh(c), c], axis=1)


def _head(head, h):
    for l, (w, b) in enumerate(head):
        h = h @ w.T + b
        if l + 1 < len(head):
            h = np.where(h > 0, h, np.expm1(np.minimum(h, 0)))   # Elu, alpha 1
    return h


def _restated(case, dt, xs, s0=None):
    """_oracle's rollout by the restatement, in dtype dt."""
    W, R, Bv, head = _params(case, dt)
    st = np.zeros((xs.shape[1], _sw(case)), dt) if s0 is None else s0.astype(dt)
    ys, sts = [], []
    for x in xs:
        st = _cell(case, W, R, Bv, x.astype(dt), st)
        assert st.dtype == dt
        ys.append(_head(head, st[:, :case.H]))
        sts.append(st)
    assert ys[0].dtype == dt
    return np.stack(ys), np.stack(sts)


def test_table_covers_the_schedule():
    """The widths enter every path of the chunk schedule and of the staging, in both cells."""
    for cell in ("gru", "lstm"):
        lean = [c for c in CASES if c.cell == cell and is_lean(c)]
        cxe = {-(-c.I // 16) for c in lean}
        assert cxe == {1, 2, 4, 5, 7, 8, 10, 11, 16, 32}
        assert {-(-c.I // 64) for c in lean} == {1, 2, 3, 4, 8}
        slot1 = {n for n in cxe if n % 4 == 3}
        assert slot1 == {7, 11} and all(n > 3 for n in slot1)          # K0S == 1 with Cxe > 3
        loops = {max(0, -(-(n - 4 - (3 if n % 4 == 3 else 0)) // 4)) for n in cxe}
        assert loops == {0, 1, 2, 3, 7}                                 # the x loop: 0, 1, 2 and more times
        assert {c.kernel[c.kernel.index("<"):] for c in lean} == {t for _, _, _, t in _LEAN}
        general = [c for c in CASES if c.cell == cell and not is_lean(c)]
        assert {-(-c.I // 16) for c in general} == {5, 7, 11, 16}
    assert len(set(CASES)) == len(CASES) == 48


_CXE_CASES = [next(c for c in CASES if c.cell == cell and -(-c.I // 16) == n and is_lean(c))
              for cell in ("gru", "lstm") for n in (1, 2, 4, 5, 7, 8, 10, 11, 16, 32)]


@pytest.mark.parametrize("case", _CXE_CASES, ids=_id)
def test_probe_sees_x_chunks(case):
    """No GPU: on the extra tick's inputs (non-zero h), exchanging any two 16-column x chunks of
    W, dropping any one, or exchanging an x chunk with the h chunk of the same index moves h'
    by more than 1000 times the tolerance."""
    I, H, Cxe = case.I, case.H, -(-case.I // 16)
    W, R, Bv, _ = _params(case, np.float64)
    _, s0, x1 = _inputs(case)
    xp = np.zeros((B0, 16 * Cxe))
    xp[:, :I] = x1
    Wp = np.zeros((W.shape[0], 16 * Cxe))
    Wp[:, :I] = W
    s0 = s0.astype(np.float64)
    base = _cell(case, Wp, R, Bv, xp, s0)[:, :H]
    assert abs_err(base, _cell(case, W, R, Bv, x1.astype(np.float64), s0)[:, :H]) == 0.0

    def moved(Wc, Rc=R):
        return abs_err(_cell(case, Wc, Rc, Bv, xp, s0)[:, :H], base)

    least = np.inf
    blocks = Wp.reshape(-1, Cxe, 16)
    for c1, c2 in itertools.combinations(range(Cxe), 2):
        sw = blocks.copy()
        sw[:, [c1, c2]] = sw[:, [c2, c1]]
        least = min(least, moved(sw.reshape(Wp.shape)))
    for c in range(Cxe):
        z = blocks.copy()
        z[:, c] = 0
        least = min(least, moved(z.reshape(Wp.shape)))
        Wc, Rc = Wp.copy(), R.copy()     # x chunk c's weights <-> h chunk c's (H / 16 >= 8 of them)
        if c < H // 16:
            Wc[:, 16 * c:16 * c + 16], Rc[:, 16 * c:16 * c + 16] = R[:, 16 * c:16 * c + 16], Wp[:, 16 * c:16 * c + 16]
            least = min(least, moved(Wc, Rc))
    print(f"probe {_id(case)}: least movement of h' {least:.3g}")
    assert least > 1000 * TOL


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_tolerance_headroom(case, model_dir):
    """No GPU: the restatement in float32, rolled over the GPU tests' inputs, stays within a
    quarter of the tolerance of the oracle's actions and states (and in float64 within 1e-12:
    the restatement is the oracle's function)."""
    xs, s0, x1 = _inputs(case)
    roll, extra = _ref(case, model_dir)
    worst = {np.float32: 0.0, np.float64: 0.0}
    for dt in worst:
        for B in BATCHES:
            y, st = _restated(case, dt, xs[B])
            worst[dt] = max(worst[dt], abs_err(y, roll[B][0]), abs_err(st, roll[B][1]))
        y, st = _restated(case, dt, x1[None], s0)
        worst[dt] = max(worst[dt], abs_err(y, extra[0]), abs_err(st, extra[1]))
    print(f"headroom {_id(case)}: float32 {worst[np.float32]:.3g}, float64 {worst[np.float64]:.3g}")
    assert worst[np.float64] <= 1e-12
    assert worst[np.float32] <= TOL / 4


# --------------------------------------------------------------------------------------
# GPU

def _engine(case, data, monkeypatch):
    from go2_onnx_controller_amd import Engine
    for k, v in case.env:
        monkeypatch.setenv(k, v)     # read at engine creation
    e = Engine(data, max_batch=64, small_batch=-1)
    assert e.batched_kernel == case.kernel
    assert (e.in_dim, e.hidden_dim) == (case.I, _sw(case))
    return e


def _synced(e):
    """e.sync(); a device error ends the whole session (probe_models.run_checked)."""
    from go2_onnx_controller_amd.engine import Go2piError
    try:
        e.sync()
    except Go2piError as ex:
        if ex.code == -3:
            pytest.exit(f"device error, stopping: {ex}", returncode=3)
        raise


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_ticks(case, model_dir, monkeypatch):
    """Batches 33, 1, 16, 17, 15 on one engine, three ticks each from a zero state, then one tick
    from a random state at B = 33: actions and state after every tick against the oracle."""
    data, _ = _graph(case, model_dir)
    xs, s0, x1 = _inputs(case)
    roll, extra = _ref(case, model_dir)
    worst = 0.0
    with _engine(case, data, monkeypatch) as e:
        for B in BATCHES:
            e.reset_hidden()
            for t in range(T):
                y, st = pm.run_checked(e, xs[B][t]), e.get_hidden(B)
                errs = (abs_err(y, roll[B][0][t]), abs_err(st, roll[B][1][t]))
                worst = max(worst, *errs)
                assert y.shape == roll[B][0][t].shape and max(errs) <= TOL, (B, t, errs)
            if B == B0:
                e.set_hidden(s0)
                y, st = pm.run_checked(e, x1), e.get_hidden(B)
                errs = (abs_err(y, extra[0][0]), abs_err(st, extra[1][0]))
                worst = max(worst, *errs)
                assert max(errs) <= TOL, ("extra tick", errs)
    print(f"ticks {_id(case)}: {case.kernel} worst {worst:.3g}")


_SEQ_CASES = [c for c in CASES if (is_lean(c) and c.I in (98, 245, 512)) or (not is_lean(c) and c.I == 245)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", _SEQ_CASES, ids=_id)
def test_sequence_matches_ticks(case, model_dir, monkeypatch):
    """Three ticks as one device-side sequence (the observation staged again on steps 1 and 2)
    are bitwise the three ticks launched one by one, and within the tolerance of the oracle."""
    import torch
    data, _ = _graph(case, model_dir)
    xs, _, _ = _inputs(case)
    want_y, want_st = _ref(case, model_dir)[0][B0]
    xd = torch.from_numpy(xs[B0].copy()).cuda()
    with _engine(case, data, monkeypatch) as a, _engine(case, data, monkeypatch) as b:
        a.reset_hidden()
        b.reset_hidden()
        ya = a.run_sequence_torch(xd)
        _synced(a)
        yb = torch.stack([b.run_torch(xd[t].contiguous()) for t in range(T)])
        _synced(b)
        ya, yb, ha, hb = ya.cpu().numpy(), yb.cpu().numpy(), a.get_hidden(B0), b.get_hidden(B0)
    assert ya.tobytes() == yb.tobytes() and ha.tobytes() == hb.tobytes()
    assert abs_err(ya, want_y) <= TOL and abs_err(ha, want_st[-1]) <= TOL


_NONFINITE = [c for c in CASES if (c.H, c.I) == (128, 98) and c.head == (128, 128, 128, 12)
              or (c.H, c.I) == (128, 49) and is_lean(c)
              or c.env and c.I == 98]


def _tick(e, x, s0):
    e.set_hidden(s0)
    y = pm.run_checked(e, x)
    return y, e.get_hidden(len(x))


@pytest.mark.gpu
@pytest.mark.parametrize("case", _NONFINITE, ids=_id)
def test_nonfinite_rows(case, model_dir, monkeypatch):
    """One non-finite observation element, B = 33, from the random state. A NaN (column 0 or the
    last column of row 5, the last column of the last row, which the lean tick also stages
    into the ragged tile's padding rows) makes that row's actions and state NaN and leaves
    every other row bitwise what it is without it, on this tick, and within the tolerance on
    the next. An infinity (either sign, column 0 or the last) saturates the gates: the oracle
    says which outputs are NaN, which infinite, and what the finite ones are."""
    data, g = _graph(case, model_dir)
    _, s0, x1 = _inputs(case)
    xs, _, _ = _inputs(case)
    x2 = xs[B0][0]     # the clean observation of the tick after
    I = case.I
    want_y, want_st = _oracle(g, case, np.stack([x1, x2]), s0)
    with _engine(case, data, monkeypatch) as e:
        y0, st0 = _tick(e, x1, s0)
        assert abs_err(y0, want_y[0]) <= TOL and abs_err(st0, want_st[0]) <= TOL
        for row, col in ((5, 0), (5, I - 1), (B0 - 1, I - 1)):
            x = x1.copy()
            x[row, col] = np.nan
            y, st = _tick(e, x, s0)
            others = np.arange(B0) != row
            assert np.isnan(y[row]).all() and np.isnan(st[row]).all(), (row, col)
            assert y[others].tobytes() == y0[others].tobytes() and st[others].tobytes() == st0[others].tobytes(), (row, col)
            y, st = pm.run_checked(e, x2), e.get_hidden(B0)      # the next tick, clean input
            assert abs_err(y[others], want_y[1][others]) <= TOL, (row, col)
            assert abs_err(st[others], want_st[1][others]) <= TOL, (row, col)
        row, others = 5, np.arange(B0) != 5
        for v, col in itertools.product((np.inf, -np.inf), (0, I - 1)):
            x = x1.copy()
            x[row, col] = v
            oy, ost = _oracle(g, case, x[None], s0)
            y, st = _tick(e, x, s0)
            for got, want in ((y, oy[0]), (st, ost[0])):
                assert np.array_equal(np.isnan(got), np.isnan(want)), (v, col, got[row], want[row])
                assert np.array_equal(np.isinf(got), np.isinf(want)), (v, col, got[row], want[row])
                fin = np.isfinite(want)
                assert abs_err(got[fin], want[fin]) <= TOL, (v, col)
            assert y[others].tobytes() == y0[others].tobytes() and st[others].tobytes() == st0[others].tobytes(), (v, col)
