"""The one-tick form of the lean pipeline kernel (policy_mlp_kernel: no step loop, the
ring's fragments requested first, an identity head) and the looped form it was split
from (policy_mlp_seq_kernel: device-side sequences, and a head with an activation).

Every shape the lean kernel is instantiated for, at batches around the 16-row tile (a
partial tile, an exact one, one row past it, several tiles), against the fp64 oracle at
the project's 1e-5 absolute (the synthetic models' outputs are O(0.1-1)); the two forms
against each other to the bit (the same fma chains in the same order); and a Tanh head,
which the one-tick form does not serve.
"""
import numpy as np
import pytest

from conftest import SHIPPED, abs_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
BATCHES = (1, 15, 16, 17, 33, 300)

# the one-tick kernel of each policy: <tiles per wave, head tiles, layer-0 chunks mod 4, act,
# hidden layers, waves>
SHAPES = {
    "go2_mlp_512": "policy_mlp_kernel<8, 1, 3, 1, 3, 4>",        # 8 tiles per wave, 3 layer-0 chunks
    "pipe_512_relu": "policy_mlp_kernel<8, 1, 0, -1, 0, 4>",     # 8 chunks of layer 0: two 64-column staging chunks
    "pipe_256_h2": "policy_mlp_kernel<4, 2, 3, 1, 0, 4>",        # 4 tiles per wave, two head tiles
    "pipe_128_tanh_h2": "policy_mlp_kernel<2, 2, 3, -1, 0, 4>",  # 2 tiles per wave, the barrier form
    "shipped": "policy_mlp_kernel<2, 1, 3, 1, 3, 4>",
}

_cache = {}


def _case(synth_path, name):
    """(model path, inputs [300, in_dim], fp64 oracle outputs of those rows): computed once."""
    if name not in _cache:
        from oracle import onnx_ref
        p = SHIPPED if name == "shipped" else synth_path(name)
        g = onnx_ref.load(p)
        x = np.random.default_rng(23).standard_normal((max(BATCHES), g.inputs[0][1][1])).astype(np.float32)
        want = onnx_ref.act(g, x)
        x.setflags(write=False)
        want.setflags(write=False)
        _cache[name] = (p, x, want)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_one_tick_shapes(synth_path, name):
    from go2_onnx_controller_amd import Engine
    p, x, want = _case(synth_path, name)
    with Engine(p, max_batch=512, small_batch=-1) as e:
        assert e.batched_kernel == SHAPES[name]
        for B in BATCHES:  # (a row's action does not depend on the other rows: the oracle's first B rows)
            err = abs_err(e.run(x[:B]), want[:B])
            print(name, B, err)
            assert err <= TOL, (name, B, err)


@pytest.mark.parametrize("name", ["go2_mlp_512", "shipped"])
def test_one_tick_and_looped_forms_agree_bitwise(synth_path, name):
    """T = 3 ticks of the same 33 rows in one launch (the looped kernel) against one-tick
    launches of those rows: every tick the same bits."""
    import torch
    from go2_onnx_controller_amd import Engine
    p, x, want = _case(synth_path, name)
    B, T = 33, 3
    with Engine(p, max_batch=64, small_batch=-1) as e:
        xd = torch.from_numpy(x[:B].copy()).cuda()
        one = e.run_torch(xd).cpu().numpy()
        seq = e.run_sequence_torch(xd.unsqueeze(0).repeat(T, 1, 1).contiguous()).cpu().numpy()
        again = e.run_torch(xd).cpu().numpy()
    assert abs_err(one, want[:B]) <= TOL
    assert np.array_equal(one, again)
    for t in range(T):
        assert np.array_equal(seq[t], one), (name, t, abs_err(seq[t], one))


def _tanh_head_bytes(dims=(48, 256, 256, 256, 12), seed=31):
    """Gemm -> Elu per hidden layer, Tanh after the last Gemm: the lean kernel's shape (no
    observation front-end, no action tail) with an activation on the head. The head's
    weights are scaled so that Tanh leaves its linear range."""
    from go2_onnx_controller_amd import onnx_writer as ow
    from go2_onnx_controller_amd import synth
    layers = synth.mlp_layers(dims, seed)
    layers[-1] = ((layers[-1][0] * np.float32(8)).astype(np.float32), (layers[-1][1] * np.float32(8)).astype(np.float32))
    nodes, inits, cur = [], [], "observation"
    for l, (W, b) in enumerate(layers):
        inits += [(f"W{l}", W), (f"b{l}", b)]
        nodes.append(ow.node("Gemm", [cur, f"W{l}", f"b{l}"], [f"g{l}"], "", [ow.attr_int("transB", 1)]))
        op = "Elu" if l + 1 < len(layers) else "Tanh"
        out = f"a{l}" if l + 1 < len(layers) else "action"
        nodes.append(ow.node(op, [f"g{l}"], [out]))
        cur = out
    return ow.model(nodes, inits, [("observation", ["batch", dims[0]])], [("action", ["batch", dims[-1]])])


def test_head_with_activation_takes_the_looped_form(tmp_path):
    """A Tanh head: one-tick launches run the looped kernel (its run-time head
    activation), and a sequence launch gives the same bits."""
    import torch
    from go2_onnx_controller_amd import Engine
    from oracle import onnx_ref
    p = tmp_path / "tanh_head.onnx"
    p.write_bytes(_tanh_head_bytes())
    g = onnx_ref.load(str(p))
    x = np.random.default_rng(29).standard_normal((17, 48)).astype(np.float32)
    want = onnx_ref.act(g, x)
    assert np.max(np.abs(want)) > 0.9  # the activation is not the identity on these outputs
    with Engine(str(p), max_batch=64, small_batch=-1) as e:
        assert e.batched_kernel == "policy_mlp_seq_kernel<4, 1, 3, 1, 3, 4>"
        for B in (1, 17):
            err = abs_err(e.run(x[:B]), want[:B])
            print("tanh head", B, err)
            assert err <= TOL, (B, err)
        xd = torch.from_numpy(x).cuda()
        seq = e.run_sequence_torch(xd.unsqueeze(0).repeat(2, 1, 1).contiguous()).cpu().numpy()
        assert np.array_equal(seq[0], e.run(x)) and np.array_equal(seq[1], seq[0])
