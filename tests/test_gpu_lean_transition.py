"""GPU: the lean one-tick kernel's layer hand-off, head and tail (policy_mlp_kernel with the
compile-time Elu: w4_step's own phase, w4_epi_elu1, the fused head, the partial sums).

What a change to the transition can break is a term, not a rounding: a tile whose first MFMA
does not start from its bias, a tile published or read one layer early, a head partial left
out of the sum, a row of a ragged tile stored or skipped. So:

* integer probes (tests/probe_models.py: non-negative weights, biases 1..3 and observations,
  where Elu is the identity and every partial sum is an integer below 2^24, exact in float32
  in any order) at 4 and 8 tiles per wave (256- and 512-wide), with 1, 2 and 3 hidden layers
  (no transition, one, and the unrolled three-layer form), at B = 1, 15, 16, 17, 33 (one row,
  a partial tile, a full one, one row into the second workgroup, a third ragged workgroup):
  every answer equals the int64 reference, and the engine reports the instantiation named here;
* the same probes as two ticks of one device-side sequence, which runs the looped kernel
  (policy_mlp_seq_kernel) that shares the code;
* an Elu policy with hidden biases of magnitude 0.75-2 and both signs, so that both branches
  of the activation are taken and a tile started from zero (or from another tile's bias)
  moves an action by far more than the tolerance (checked below in float64 for every tile of
  every hidden layer), against the fp64 oracle at the project's 1e-5 absolute.
"""
import numpy as np
import pytest

import probe_models as pm
from conftest import abs_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
BATCHES = [1, 15, 16, 17, 33]

# probe dims -> the one-tick kernel <tiles per wave, head tiles, layer-0 chunks mod 4, act,
# compile-time hidden-layer count (3, or 0: run time), waves>
PROBES = {
    (48, 256, 12): "policy_mlp_kernel<4, 1, 3, 1, 0, 4>",
    (48, 256, 256, 12): "policy_mlp_kernel<4, 1, 3, 1, 0, 4>",
    (33, 256, 256, 256, 12): "policy_mlp_kernel<4, 1, 3, 1, 3, 4>",
    (70, 512, 16): "policy_mlp_kernel<8, 1, 0, 1, 0, 4>",
    (48, 512, 512, 12): "policy_mlp_kernel<8, 1, 3, 1, 0, 4>",
    (48, 512, 512, 512, 12): "policy_mlp_kernel<8, 1, 3, 1, 3, 4>",
}

_cases = {}


def _case(dims):
    """(onnx bytes, one observation array per batch of BATCHES, their exact answers): once."""
    if dims not in _cases:
        data, layers = pm.int_policy(dims, "Elu", False)
        xs = pm.int_inputs(layers, BATCHES)
        assert pm.abs_sum_bound(layers, np.concatenate(xs)) < 2 ** 24   # exact in float32, any order
        refs = [pm.int_ref(layers, x) for x in xs]
        for a in xs + refs:
            a.setflags(write=False)
        _cases[dims] = (data, xs, refs)
    return _cases[dims]


def _id(dims):
    return "_".join(str(d) for d in dims)


@pytest.mark.parametrize("dims", list(PROBES), ids=_id)
def test_one_tick_exact(dims):
    from go2_onnx_controller_amd import Engine
    data, xs, refs = _case(dims)
    bad = []
    with Engine(data, max_batch=64, small_batch=-1) as e:
        kern = e.batched_kernel
        for x, ref in zip(xs, refs):
            y = pm.run_checked(e, x)
            if not (y.shape == ref.shape and np.array_equal(y, ref)):
                bad.append((len(x), int((y != ref).sum()) if y.shape == ref.shape else y.shape))
    print(f"lean transition {_id(dims)}: {kern!r} bad={bad}")
    assert kern == PROBES[dims]
    assert not bad, f"(rows, differing outputs): {bad}"


@pytest.mark.parametrize("dims", list(PROBES), ids=_id)
def test_two_tick_sequence_exact(dims):
    """Two ticks in one launch (the looped kernel), each with observations of its own: the
    17- and the 33-row requests (tick 1 of the 33-row one is its rows in reverse order)."""
    import torch
    from go2_onnx_controller_amd import Engine
    data, xs, refs = _case(dims)
    with Engine(data, max_batch=64, small_batch=-1) as e:
        for i in (BATCHES.index(17), BATCHES.index(33)):
            x2 = np.stack([xs[i], xs[i][::-1]])
            want = np.stack([refs[i], refs[i][::-1]])
            y = e.run_sequence_torch(torch.from_numpy(x2.copy()).cuda()).cpu().numpy()
            assert y.shape == want.shape and np.array_equal(y, want), (len(xs[i]), int((y != want).sum()))


# --------------------------------------------------------------------------------------
# Elu with biases that matter

def _bias_layers(dims, seed=41):
    """synth's uniform weights; hidden biases +-(0.75 + 0.25 * ((n + l) % 6)), the sign
    alternating every third unit: within every 16-unit tile both signs and six magnitudes."""
    from go2_onnx_controller_amd import synth
    layers = synth.mlp_layers(dims, seed)
    for l in range(len(layers) - 1):
        n = np.arange(layers[l][1].shape[0])
        b = (0.75 + 0.25 * ((n + l) % 6)) * np.where((n // 3 + l) % 2, -1.0, 1.0)
        layers[l] = (layers[l][0], b.astype(np.float32))
    return layers


def _bytes(layers, dims):
    from go2_onnx_controller_amd import onnx_writer as ow
    nodes, inits, cur = [], [], "observation"
    for l, (W, b) in enumerate(layers):
        last = l + 1 == len(layers)
        inits += [(f"W{l}", W), (f"b{l}", b)]
        nodes.append(ow.node("Gemm", [cur, f"W{l}", f"b{l}"], ["action" if last else f"g{l}"], "",
                             [ow.attr_int("transB", 1)]))
        if not last:
            nodes.append(ow.node("Elu", [f"g{l}"], [f"a{l}"]))
            cur = f"a{l}"
    return ow.model(nodes, inits, [("observation", ["batch", dims[0]])], [("action", ["batch", dims[-1]])])


def _fwd64(layers, x, drop=None):
    """float64 forward; drop = (layer, tile): that tile's 16 biases of that layer are zero."""
    h = x.astype(np.float64)
    for l, (W, b) in enumerate(layers):
        b = b.astype(np.float64)
        if drop is not None and drop[0] == l:
            b = b.copy()
            b[16 * drop[1]:16 * drop[1] + 16] = 0
        z = h @ W.astype(np.float64).T + b
        h = z if l + 1 == len(layers) else np.where(z > 0, z, np.expm1(np.minimum(z, 0)))
    return h


@pytest.mark.parametrize("dims,kernel", [((48, 256, 256, 256, 12), "policy_mlp_kernel<4, 1, 3, 1, 3, 4>"),
                                         ((48, 512, 512, 512, 12), "policy_mlp_kernel<8, 1, 3, 1, 3, 4>")],
                         ids=["256x3", "512x3"])
def test_elu_biases_matter(tmp_path, dims, kernel):
    from go2_onnx_controller_amd import Engine
    from oracle import onnx_ref
    layers = _bias_layers(dims)
    p = tmp_path / "bias.onnx"
    p.write_bytes(_bytes(layers, dims))
    x = np.random.default_rng(43).standard_normal((max(BATCHES), dims[0])).astype(np.float32)
    want = onnx_ref.act(onnx_ref.load(str(p)), x)
    mine = _fwd64(layers, x)
    assert abs_err(mine, want) <= 1e-9   # the sensitivity check below speaks of the oracle's function
    # every tile of every hidden layer: without its biases some action moves by >= 100 tolerances
    least = min(float(np.max(np.abs(_fwd64(layers, x, (l, t)) - mine)))
                for l in range(len(dims) - 2) for t in range(dims[1] // 16))
    print(f"elu biases {_id(dims)}: least action change without one tile's biases {least:.3g}")
    assert least >= 100 * TOL
    # both Elu branches are taken in every hidden layer
    h = x.astype(np.float64)
    for W, b in layers[:-1]:
        z = h @ W.astype(np.float64).T + b
        assert 0.2 < float((z > 0).mean()) < 0.8
        h = np.where(z > 0, z, np.expm1(np.minimum(z, 0)))
    with Engine(str(p), max_batch=64, small_batch=-1) as e:
        assert e.batched_kernel == kernel
        for B in BATCHES:
            err = abs_err(pm.run_checked(e, x[:B]), want[:B])
            print(f"elu biases {_id(dims)} B={B}: {err:.3g}")
            assert err <= TOL, (B, err)
