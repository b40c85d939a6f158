"""The lean pipeline's layer hand-off (w4_step: the own phase, the flag observation, the LDS
phase's rotated chunk order and its ring tail), pinned by integer probes whose weights show
the chunk index.

A fault of the hand-off is a chunk, not a rounding: a 16-wide k-chunk of weights met with the
wrong chunk of activations (a wrong offset, another wave's rotation), a fragment of the next
layer consumed one layer early, a tile read before its wave published it. So every probe here
is exact in float32 (tests/probe_models.py: non-negative integers, Elu the identity on them,
every partial sum below 2^24) and every comparison is `np.array_equal` against the int64
reference, and the weights are built so that such a fault moves an integer:

* hidden layer l >= 1, unit n, chunk c holds ONE non-zero weight, at column
  16 c + perm_n[c % 16] with the value 1 + (c // 16 + flip_n) % 2 (perm_n a seeded permutation
  of the 16 positions and flip_n a seeded bit, per unit and layer): for a given unit the 16 or
  32 chunks carry 16 or 32 distinct (position, value) patterns. (Patterns that were an affine
  function of c and n cancelled: an exchange of two chunks moved layer 1's units by values
  that summed to zero over every unit of layer 2.)
* test_probe_sees_chunks (no GPU) swaps every pair of chunks of every hidden layer in the
  reference, rotates one wave's chunks by its tile count, and exchanges two layers' weights:
  each must change the reference's answer, or the probe could not see that fault.

Shapes: hidden widths 256 and 512 (4 and 8 tiles per wave) with 1, 2 and 3 hidden layers (no
hand-off; a hand-off without a next layer's ring tail; both), observation widths 16, 48 and
64 (layer 0 of 4, 3 and 4 chunks: the ring starts on slot 0 or 1), B = 1, 15, 16, 17, 33, each
through one launch (policy_mlp_kernel) and as two ticks of one device-side sequence (the looped
kernel). The engine must report the instantiation named here. The race check launches the
3-layer 512-wide probe 50 times back to back on one stream at B = 16 and B = 4096: a hand-off
race shows as a differing output, not as a fault.

The lean GRU tick runs the same hand-off behind its cell. A recurrent cell is not exact in
general; _gru_probe saturates a GRU-128 so that h' is exactly +-1 (checked against the fp64
oracle without a GPU), which makes the 256-wide chain behind it an integer probe again:
three ticks, launch by launch and as one sequence, `array_equal` to the int64 reference.
"""
import numpy as np
import pytest

import probe_models as pm

BATCHES = [1, 15, 16, 17, 33]
WIDTHS = [256, 512]
DEPTHS = [1, 2, 3]
OBS = [16, 48, 64]
OUT = 12
CASES = [(k, h, d) for h in WIDTHS for d in DEPTHS for k in OBS]


def _kernel(k, h, d):
    """policy_mlp_kernel<tiles per wave, head tiles, layer-0 chunks mod 4, Elu, compile-time
    hidden-layer count (3, or 0: run time), waves>"""
    c0m = 3 if -(-k // 16) % 4 == 3 else 0
    return f"policy_mlp_kernel<{h // 64}, 1, {c0m}, 1, {3 if d == 3 else 0}, 4>"


def _layers(k, h, d):
    dims = [k] + [h] * d + [OUT]
    dense = []
    n = np.arange(h)
    # layer 0: three weights of 1-2 per unit in seeded random columns and a bias of 1-3, so that
    # no two chunks of its output hold the same values (a periodic layer 0 makes chunks c and
    # c + 3 equal, and exchanging their weights in layer 1 then changes nothing)
    r = np.random.default_rng(1100 + k + h)
    W = np.zeros((h, k), np.int64)
    for j in range(3):
        W[n, r.integers(0, k, h)] = r.integers(1, 3, h)
    dense.append({"W": W, "b": r.integers(1, 4, h).astype(np.int64), "act": "Elu"})
    for l in range(1, d):
        W = np.zeros((h, h), np.int64)
        perm = np.argsort(r.random((h, 16)), axis=1)    # a permutation of the 16 positions per unit
        flip = r.integers(0, 2, h)
        for c in range(h // 16):
            W[n, 16 * c + perm[:, c % 16]] = 1 + (c // 16 + flip) % 2
        dense.append({"W": W, "b": (1 + (n + l) % 3).astype(np.int64), "act": "Elu"})
    o, kk = np.arange(OUT)[:, None], np.arange(h)[None, :]
    W = ((o * 31 + kk * 17 + (o * kk) % 13) % 4 == 0).astype(np.int64)
    dead = np.flatnonzero(W.sum(0) == 0)
    W[dead % OUT, dead] = 1                             # every hidden unit reaches an action
    dense.append({"W": W, "b": (np.arange(OUT) % 3).astype(np.int64), "act": None})
    return {"dims": dims, "signed": False, "act": "Elu", "dense": dense, "front": None, "tail": None}


def _onnx(layers):
    from go2_onnx_controller_amd import onnx_writer as ow
    dims, nodes, inits, cur = layers["dims"], [], [], "obs"
    for l, d in enumerate(layers["dense"]):
        inits += [(f"W{l}", d["W"].astype(np.float32)), (f"b{l}", d["b"].astype(np.float32))]
        nodes.append(ow.node("Gemm", [cur, f"W{l}", f"b{l}"], [f"g{l}"], "", [ow.attr_int("transB", 1)]))
        cur = f"g{l}"
        if d["act"]:
            nodes.append(ow.node("Elu", [cur], [f"a{l}"], "", [ow.attr_float("alpha", 1.0)]))
            cur = f"a{l}"
    nodes.append(ow.node("Identity", [cur], ["act"]))
    return ow.model(nodes, inits, [("obs", ["N", dims[0]])], [("act", ["N", dims[-1]])])


_cases = {}


def _case(k, h, d):
    """(onnx bytes, layers, one observation array per batch of BATCHES, their exact answers): once."""
    if (k, h, d) not in _cases:
        layers = _layers(k, h, d)
        xs = pm.int_inputs(layers, BATCHES)
        assert pm.abs_sum_bound(layers, np.concatenate(xs)) < 2 ** 24   # exact in float32, any order
        refs = [pm.int_ref(layers, x) for x in xs]
        for a in xs + refs:
            a.setflags(write=False)
        _cases[(k, h, d)] = (_onnx(layers), layers, xs, refs)
    return _cases[(k, h, d)]


def _id(c):
    return f"{c[0]}_{c[1]}x{c[2]}"


def _with(layers, l, W):
    dense = list(layers["dense"])
    dense[l] = dict(dense[l], W=W)
    return dict(layers, dense=dense)


@pytest.mark.parametrize("h,d", [(h, d) for h in WIDTHS for d in (2, 3)], ids=lambda v: str(v))
def test_probe_sees_chunks(h, d):
    """No GPU: every chunk fault the probe is meant to catch changes the exact answer."""
    _, layers, xs, refs = _case(48, h, d)
    x, base = xs[-1], refs[-1]
    C, tpw = h // 16, h // 64
    dense = layers["dense"]
    ins = [x.astype(np.float64)]    # the input rows of every layer (float64: exact, and a BLAS product)
    for dl in dense[:-1]:
        ins.append(ins[-1] @ dl["W"].T.astype(np.float64) + dl["b"])

    def changed(l, Wl):
        """Does the answer change with Wl as layer l's weights?"""
        y = ins[l]
        for m in range(l, len(dense)):
            y = y @ (Wl if m == l else dense[m]["W"]).T.astype(np.float64) + dense[m]["b"]
        return not np.array_equal(y, base)

    assert not changed(1, dense[1]["W"])   # (the float64 forward is the int64 reference)
    for l in range(1, d):
        W = dense[l]["W"]
        for unit in (0, h - 1):     # the patterns of a unit's chunks are distinct
            pat = {(int(np.flatnonzero(W[unit, 16 * c:16 * c + 16])[0]), int(W[unit, 16 * c:16 * c + 16].max()))
                   for c in range(C)}
            assert len(pat) == C
        blocks = W.reshape(h, C, 16)
        for c1 in range(C):
            for c2 in range(c1 + 1, C):
                sw = blocks.copy()
                sw[:, [c1, c2]] = sw[:, [c2, c1]]
                assert changed(l, sw.reshape(h, h)), (l, c1, c2)
        for w in range(4):          # one wave's units with their chunks rotated by its tile count
            rot = blocks.copy()
            u = slice(16 * tpw * w, 16 * tpw * (w + 1))
            rot[u] = np.roll(rot[u], tpw, axis=1)
            assert changed(l, rot.reshape(h, h)), (l, w)
    if d == 3:                      # layer 2's fragments consumed as layer 1's and the reverse
        ex = _with(_with(layers, 1, layers["dense"][2]["W"]), 2, layers["dense"][1]["W"])
        assert not np.array_equal(pm.int_ref(ex, x), base)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_one_launch_exact(case):
    from go2_onnx_controller_amd import Engine
    data, _, xs, refs = _case(*case)
    bad = []
    with Engine(data, max_batch=64, small_batch=-1) as e:
        kern = e.batched_kernel
        for x, ref in zip(xs, refs):
            y = pm.run_checked(e, x)
            if not (y.shape == ref.shape and np.array_equal(y, ref)):
                bad.append((len(x), int((y != ref).sum()) if y.shape == ref.shape else y.shape))
    print(f"lean handoff {_id(case)}: {kern!r} bad={bad}")
    assert kern == _kernel(*case)
    assert not bad, f"(rows, differing outputs): {bad}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_two_tick_sequence_exact(case):
    """Two ticks in one launch (the looped kernel), tick 1 the batch's rows in reverse order."""
    import torch
    from go2_onnx_controller_amd import Engine
    data, _, xs, refs = _case(*case)
    bad = []
    with Engine(data, max_batch=64, small_batch=-1) as e:
        assert e.batched_kernel == _kernel(*case)
        for x, ref in zip(xs, refs):
            x2, want = np.stack([x, x[::-1]]), np.stack([ref, ref[::-1]])
            y = e.run_sequence_torch(torch.from_numpy(x2.copy()).cuda()).cpu().numpy()
            if not (y.shape == want.shape and np.array_equal(y, want)):
                bad.append((len(x), int((y != want).sum()) if y.shape == want.shape else y.shape))
    assert not bad, f"(rows, differing outputs): {bad}"


@pytest.mark.gpu
@pytest.mark.parametrize("B", [16, 4096])
def test_back_to_back_launches_agree(B):
    """50 launches on one stream, each into rows of its own: 50 times the exact answer."""
    import torch
    from go2_onnx_controller_amd import Engine
    data, layers, _, _ = _case(48, 512, 3)
    x = pm.int_inputs(layers, [B], seed=5)[0]
    assert pm.abs_sum_bound(layers, x) < 2 ** 24
    ref = pm.int_ref(layers, x)
    with Engine(data, max_batch=B, small_batch=-1) as e:
        assert e.batched_kernel == _kernel(48, 512, 3)
        xd = torch.from_numpy(x).cuda()
        out = torch.full((50, B, OUT), -1.0, dtype=torch.float32, device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        for i in range(50):
            e.run_torch(xd, out=out[i], stream=s)
        s.synchronize()
        y = out.cpu().numpy()
    differ = [i for i in range(50) if y[i].tobytes() != y[0].tobytes()]
    assert not differ, f"launches that differ from the first: {differ}"
    assert np.array_equal(y[0], ref)


# --------------------------------------------------------------------------------------
# the lean GRU tick shares the hand-off: a saturated cell makes its dense chain exact

GRU_H, GRU_I, GRU_B, GRU_T = 128, 48, 33, 3


def _gru_probe():
    """(onnx bytes, layers of the dense chain, x [T, B, I], exact actions [T, B, OUT]): a GRU-128
    (linear_before_reset = 1) in front of the 256-wide 3-layer chain of the probes above. The
    cell is saturated so that h' is exactly +-1 in float32 and in float64, whatever h was:
    no recurrent weights; update gate z = sigmoid(-60) = 8.8e-27, so (1 - z) n + z h and
    n + z (h - n) both round to n; candidate n = tanh(40 x[j % I] - 20) = tanh(-20) or tanh(>= 20),
    where 1 -+ 8e-18 rounds to +-1 (as 2 sigmoid(2 a) - 1: sigmoid is 1 / (1 + 4e-18) = 1 or
    4e-18). The chain's layer 0 has biases 7-9 over three weights of 1-2, so its pre-activations
    stay >= 1 on +-1 inputs and Elu is the identity from there on."""
    from go2_onnx_controller_amd import onnx_writer as ow
    H, I = GRU_H, GRU_I
    layers = _layers(H, 256, 3)
    layers["dense"][0] = dict(layers["dense"][0], b=layers["dense"][0]["b"] + 6)
    W = np.zeros((1, 3 * H, I), np.float32)              # gates z, r, h
    W[0, 2 * H + np.arange(H), np.arange(H) % I] = 40.0
    R = np.zeros((1, 3 * H, H), np.float32)
    B = np.zeros((1, 6 * H), np.float32)
    B[0, :H] = -60.0
    B[0, 2 * H:3 * H] = -20.0
    axes = np.array([0], np.int64)
    inits = [("gru.W", W), ("gru.R", R), ("gru.B", B), ("axes0", axes)]
    nodes = [ow.node("Unsqueeze", ["observation", "axes0"], ["x_seq"]),
             ow.node("GRU", ["x_seq", "gru.W", "gru.R", "gru.B", "", "h_in"], ["gru_Y", "h_out"], "",
                     [ow.attr_int("hidden_size", H), ow.attr_int("linear_before_reset", 1)]),
             ow.node("Squeeze", ["h_out", "axes0"], ["h_t"])]
    cur = "h_t"
    for l, d in enumerate(layers["dense"]):
        last = l + 1 == len(layers["dense"])
        inits += [(f"W{l}", d["W"].astype(np.float32)), (f"b{l}", d["b"].astype(np.float32))]
        nodes.append(ow.node("Gemm", [cur, f"W{l}", f"b{l}"], ["action" if last else f"g{l}"], "",
                             [ow.attr_int("transB", 1)]))
        cur = f"g{l}"
        if not last:
            nodes.append(ow.node("Elu", [cur], [f"a{l}"], "", [ow.attr_float("alpha", 1.0)]))
            cur = f"a{l}"
    data = ow.model(nodes, inits, [("observation", ["batch", I]), ("h_in", [1, "batch", H])],
                    [("action", ["batch", OUT]), ("h_out", [1, "batch", H])])
    x = np.random.default_rng(77).integers(0, 4, (GRU_T, GRU_B, I)).astype(np.float32)
    s = np.where(x[:, :, np.arange(H) % I] >= 1, 1, -1).astype(np.int64)     # h' of every tick
    h, zmin = s, None
    for d in layers["dense"]:
        z = h @ d["W"].T + d["b"]
        zmin = int(z.min()) if zmin is None else zmin
        h = z
    assert zmin >= 1 and np.abs(h).max() < 2 ** 24
    return data, layers, x, h, s


def test_gru_probe_is_exact_in_the_oracle(tmp_path):
    """No GPU: the fp64 oracle gives the integer answer and h' = +-1 exactly, tick after tick."""
    from oracle import onnx_ref
    data, _, x, want, s = _gru_probe()
    p = tmp_path / "gru_probe.onnx"
    p.write_bytes(data)
    g = onnx_ref.load(str(p))
    h = np.full((1, GRU_B, GRU_H), 0.25)     # a state the saturated cell must forget
    for t in range(GRU_T):
        r = onnx_ref.run(g, {"observation": x[t].astype(np.float64), "h_in": h})
        h = r["h_out"]
        assert np.array_equal(h[0], s[t]) and np.array_equal(r["action"], want[t]), t


@pytest.mark.gpu
def test_gru_tick_exact():
    """Three ticks, one launch each, then the same three as one device-side sequence."""
    import torch
    from go2_onnx_controller_amd import Engine
    data, _, x, want, s = _gru_probe()
    with Engine(data, max_batch=64) as e:
        assert e.batched_kernel == "policy_gru_kernel<4, 1, 2>"
        e.reset_hidden()
        for t in range(GRU_T):
            y = pm.run_checked(e, x[t])
            assert np.array_equal(y, want[t]), (t, int((y != want[t]).sum()))
        assert np.array_equal(e.get_hidden(GRU_B), s[-1])
        e.reset_hidden()
        y = e.run_sequence_torch(torch.from_numpy(x).cuda()).cpu().numpy()
        assert np.array_equal(y, want), int((y != want).sum())
