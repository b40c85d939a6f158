"""Residual MLP policies (x + f(x)) for the tests: SimBa blocks, whose carried value is the
un-normalised sum in front of a LayerNormalization, and ResNet-v1 blocks, whose carried value
is an activated layer output.

Every model is described once, as a list of layers (skip_models.L's fields plus res: the index
of the layer whose carried value is added to this layer's Gemm + bias output, in front of its
LayerNormalization and activation), and three things are derived from that description: the
ONNX bytes (onnx_writer), the view the loader must report (K, N, act, ln, skip, res), and, for
the integer probes, an int64 evaluation that owes nothing to the loader or to the oracle.

The carried value of layer j is the input of its LayerNormalization where it has one (the sum
s_j of a pre-LN layer, act(s_j) of a post-LN one), else its output.

Weights are uniform in +-1 / sqrt(K) from a seeded generator, observations N(0, 1) from a
seeded generator. None of these models is in synth.MODELS (the golden hashes stay as they are).
"""
from __future__ import annotations

import os

import numpy as np

from go2_onnx_controller_amd import onnx_writer as ow

ACT_CODE = {None: 0, "Elu": 1, "Relu": 2, "Tanh": 3, "Sigmoid": 4}
RUN = "run"


def L(n, act=None, inp=(RUN,), ln=None, res=None):
    """One dense layer: n outputs, activation, input parts ("run" / (b, e) observation columns),
    LayerNormalization ("pre" / "post"), res: the source layer of the carried value it adds."""
    return dict(n=n, act=act, inp=tuple(inp), ln=ln, res=res)


# name -> (observation width, layers)
SPECS = {
    # SimBa: h = Linear(obs); h = h + Linear(Relu(Linear(LN(h)))) twice; out = Linear(LN(h)).
    # Chained taps of raw sums; 64 wide: four tiles on eight waves (the split-K store)
    "simba_64": (48, [L(64, ln="pre"), L(128, "Relu"), L(64, ln="pre", res=0), L(128, "Relu"),
                      L(64, ln="pre", res=2), L(12)]),
    # sixteen tiles on eight waves (two per wave)
    "simba_256": (48, [L(256, ln="pre"), L(256, "Relu"), L(256, ln="pre", res=0), L(12)]),
    # ResNet v1: the tap is an activated output, the width no multiple of 16, and the layer in
    # front of the 5-wide head carries the sum
    "res_v1": (33, [L(100, "Tanh"), L(100, "Tanh"), L(100, "Tanh", res=0), L(5)]),
    # one-layer blocks: each layer both consumer and source
    "res_adjacent": (48, [L(64, "Elu"), L(64, "Elu", res=0), L(64, "Elu", res=1), L(12)]),
    # the padded columns [20, 64) accumulate Sigmoid(0) = 0.5 per layer
    "res_sig": (48, [L(20, "Sigmoid"), L(20, "Sigmoid", res=0), L(20, "Sigmoid", res=1), L(12)]),
    # an estimator-actor with a residual block: the consumer (layer 4) is padded to its skip
    # successor's K_pad = 128, its source (layer 2) to 64
    "res_skip": (98, [L(64, "Elu", [(0, 98)]), L(19), L(64, "Elu", [RUN, (0, 49)]), L(64, "Elu"),
                      L(64, "Elu", res=2), L(64, "Elu", [RUN, (49, 98)]), L(12)]),
    # post-LN: the carried value is the activated value in front of the LN
    "res_post": (48, [L(64, "Relu", ln="post"), L(64, "Relu"), L(64, "Relu", ln="post", res=0), L(12)]),
}
NAMES = tuple(SPECS)
SEED = {n: 9300 + i for i, n in enumerate(NAMES)}

PROBE_SPECS = {
    "probe_v1": (40, [L(48, "Relu"), L(48, "Relu"), L(48, "Relu", res=0), L(8)]),
    "probe_adjacent": (30, [L(32, "Relu"), L(32, "Relu", res=0), L(32, "Relu", res=1), L(6)]),
}
PROBES = tuple(PROBE_SPECS)
PROBE_SEED = {"probe_v1": 31, "probe_adjacent": 32}

PARITY_BATCHES = (1, 5, 8, 9, 16, 17, 33)


def spec(name):
    return SPECS[name] if name in SPECS else PROBE_SPECS[name]


def in_dim(name: str) -> int:
    return spec(name)[0]


def _part_width(p, prev_n):
    return prev_n if p == RUN else p[1] - p[0]


def layer_k(layers, l):
    prev_n = layers[l - 1]["n"] if l else 0
    if l == 0 and layers[0]["inp"] == (RUN,):
        return None  # (the observation: filled in by the caller)
    return sum(_part_width(p, prev_n) for p in layers[l]["inp"])


def _k(name, l):
    F, layers = spec(name)
    k = layer_k(layers, l)
    return F if k is None else k


def weights(name: str):
    """[(W [N, K] in ONNX (Concat) column order, b [N], LN scale, LN bias)] per layer."""
    _, layers = spec(name)
    if name in PROBE_SPECS:
        return _probe_weights(name)
    rng = np.random.default_rng(SEED[name])
    out = []
    for l, ly in enumerate(layers):
        K, N = _k(name, l), ly["n"]
        a = 1.0 / np.sqrt(K)
        W = rng.uniform(-a, a, (N, K)).astype(np.float32)
        b = rng.uniform(-a, a, N).astype(np.float32)
        g = rng.uniform(0.75, 1.25, N).astype(np.float32) if ly["ln"] else None
        c = rng.uniform(-0.25, 0.25, N).astype(np.float32) if ly["ln"] else None
        out.append((W, b, g, c))
    return out


def model_bytes(name: str) -> bytes:
    F, layers = spec(name)
    nodes, inits = [], [("ax1", np.array([1], np.int64))]
    x0 = "observation"
    cur, n_slice = x0, 0
    tap = {}  # layer -> the tensor that holds its carried value
    for l, (ly, (W, b, g, c)) in enumerate(zip(layers, weights(name))):
        names = []
        for p in ly["inp"]:
            if p == RUN or p == (0, F):
                names.append(cur if p == RUN else x0)
            else:
                out = f"part{n_slice}"
                inits += [(f"st{n_slice}", np.array([p[0]], np.int64)), (f"en{n_slice}", np.array([p[1]], np.int64))]
                nodes.append(ow.node("Slice", [x0, f"st{n_slice}", f"en{n_slice}", "ax1"], [out], f"slice{n_slice}"))
                n_slice += 1
                names.append(out)
        if len(names) > 1:
            nodes.append(ow.node("Concat", names, [f"cat{l}"], f"cat{l}", [ow.attr_int("axis", 1 if l % 2 else -1)]))
            x = f"cat{l}"
        else:
            x = names[0]
        last = l == len(layers) - 1
        inits += [(f"w{l}", W), (f"b{l}", b)]
        y = "action" if last and not ly["act"] else f"g{l}"
        nodes.append(ow.node("Gemm", [x, f"w{l}", f"b{l}"], [y], f"gemm{l}", [ow.attr_int("transB", 1)]))
        if ly["res"] is not None:
            src = tap[ly["res"]]
            if l % 4 == 2:  # some of them through an Identity on the carried side
                nodes.append(ow.node("Identity", [src], [f"carry{l}"], f"carry{l}"))
                src = f"carry{l}"
            # both operand orders
            nodes.append(ow.node("Add", [y, src] if l % 2 else [src, y], [f"s{l}"], f"res{l}"))
            y = f"s{l}"

        def ln_node(src, dst):
            inits.extend([(f"lng{l}", g), (f"lnb{l}", c)])
            nodes.append(ow.node("LayerNormalization", [src, f"lng{l}", f"lnb{l}"], [dst], f"ln{l}",
                                 [ow.attr_int("axis", -1), ow.attr_float("epsilon", 1e-5)]))

        if ly["ln"] == "pre":
            tap[l] = y
            ln_node(y, f"n{l}")
            y = f"n{l}"
        if ly["act"]:
            out = "action" if last else f"a{l}"
            nodes.append(ow.node(ly["act"], [y], [out], f"act{l}"))
            y = out
        if ly["ln"] == "post":
            tap[l] = y
            ln_node(y, f"n{l}")
            y = f"n{l}"
        if not ly["ln"]:
            tap[l] = y
        cur = y
    return ow.model(nodes, inits, [("observation", ["batch", F])], [("action", ["batch", layers[-1]["n"]])])


def model_path(name: str, directory) -> str:
    path = os.path.join(str(directory), name + ".onnx")
    if not os.path.exists(path):
        with open(path, "wb") as fh:
            fh.write(model_bytes(name))
    return path


def expected_view(name: str):
    """What inspect_model must report per layer: K, N, act, ln, skip (device order), res."""
    F, layers = spec(name)
    out = []
    for l, ly in enumerate(layers):
        skip = [] if l == 0 else [c for p in ly["inp"] if p != RUN for c in range(p[0], p[1])]
        out.append(dict(K=_k(name, l), N=ly["n"], act=ACT_CODE[ly["act"]], ln={None: 0, "pre": 1, "post": 2}[ly["ln"]],
                        skip=skip, res=-1 if ly["res"] is None else ly["res"]))
    return out


def seed_of(name: str, B: int, k: int = 0) -> int:
    names = NAMES + PROBES
    return 63000 + 1000 * names.index(name) + 50 * k + B


def obs(name: str, B: int, k: int = 0) -> np.ndarray:
    """N(0, 1) observations [B, in_dim] float32, a fixed function of (model, B, k)."""
    rng = np.random.default_rng(seed_of(name, B, k))
    return rng.standard_normal((B, in_dim(name))).astype(np.float32)


# ---------------------------------------------------------------------------
# integer probes: integer weights, biases and observations, Relu: every partial sum, the
# carried value included, is an integer below 2^24, so float32 arithmetic is exact in any
# summation order and a kernel must return the int64 answer bit for bit.
PROBE_OBS_MAX = 2


def _probe_weights(name: str):
    _, layers = PROBE_SPECS[name]
    rng = np.random.default_rng(PROBE_SEED[name])
    out = []
    for l, ly in enumerate(layers):
        K, N = _k(name, l), ly["n"]
        W = rng.integers(-1, 2, (N, K))  # (keeps the sums below 2^24)
        W[W == 0] = 1  # every input column is read by every unit
        b = rng.integers(-4, 5, N)
        out.append((W.astype(np.float32), b.astype(np.float32), None, None))
    return out


def probe_obs(name: str, B: int) -> np.ndarray:
    rng = np.random.default_rng(seed_of(name, B))
    return rng.integers(-PROBE_OBS_MAX, PROBE_OBS_MAX + 1, (B, in_dim(name))).astype(np.float32)


def probe_forward(name: str, x, zero=None) -> np.ndarray:
    """The probe's answer in int64. zero = (l, j): unit j of the carried value that layer l
    adds is replaced by 0 on its way to the Add (the main chain keeps the unit)."""
    _, layers = PROBE_SPECS[name]
    cur = np.asarray(x).astype(np.int64)
    outs = []
    for l, (ly, (W, b, _, _)) in enumerate(zip(layers, weights(name))):
        assert ly["inp"] == (RUN,) and ly["ln"] is None
        y = cur @ W.astype(np.int64).T + b.astype(np.int64)
        if ly["res"] is not None:
            c = outs[ly["res"]]
            if zero and zero[0] == l:
                c = c.copy()
                c[:, zero[1]] = 0
            y = y + c
        if ly["act"] == "Relu":
            y = np.maximum(y, 0)
        else:
            assert ly["act"] is None
        outs.append(y)
        cur = y
    return cur


def probe_bound(name: str) -> int:
    """The largest sum |w| |h| + |b| + |carried| any unit of the probe can reach, from
    |obs| <= PROBE_OBS_MAX: an upper bound of every partial sum in any order."""
    F, layers = PROBE_SPECS[name]
    worst, cur, outs = 0, np.full(F, PROBE_OBS_MAX, np.int64), []
    for ly, (W, b, _, _) in zip(layers, weights(name)):
        cur = np.abs(W.astype(np.int64)) @ cur + np.abs(b.astype(np.int64))
        if ly["res"] is not None:
            cur = cur + outs[ly["res"]]
        outs.append(cur)
        worst = max(worst, int(cur.max()))
    return worst
