"""Estimator-actor policies (observation skip inputs) for the tests: an encoder MLP reads the
observation, and a later dense layer reads Concat(encoder output, parts of the observation).

Every model is described once, as a list of layers whose input is a list of parts
("run": the previous layer's output; (b, e): columns [b, e) of x0, the observation as layer 0
sees it), and three things are derived from that description: the ONNX bytes (onnx_writer;
Slice / Concat / Gemm nodes), the view the loader must report (K, N, act, ln and the skip
columns in device order: running value first, then the parts in Concat order), and, for the
integer probes, an int64 evaluation that owes nothing to the loader or to the oracle.

Weights are uniform in +-1 / sqrt(K) from a seeded generator, observations N(0, 1) from a
seeded generator. None of these models is in synth.MODELS (the golden hashes stay as they are).
"""
from __future__ import annotations

import os

import numpy as np

from go2_onnx_controller_amd import onnx_writer as ow

ACT_CODE = {None: 0, "Elu": 1, "Relu": 2, "Tanh": 3, "Sigmoid": 4}
RUN = "run"


def L(n, act=None, inp=(RUN,), ln=None):
    """One dense layer: n outputs, activation, input parts, LayerNormalization ("pre" / "post")."""
    return dict(n=n, act=act, inp=tuple(inp), ln=ln)


# name -> (observation width, front ("norm": Sub, Div, Clip(+-5) on the observation), layers)
SPECS = {
    # running value first; prev.N = 19 (no multiple of 4); K = 68 -> K_pad 128
    "ea_98": (98, None, [L(64, "Elu", [(0, 98)]), L(32, "Elu"), L(19), L(128, "Elu", [RUN, (0, 49)]),
                         L(64, "Elu"), L(12)]),
    # observation first: the weight columns are permuted; K = 64 exactly
    "ea_k64": (270, None, [L(128, "Elu", [(0, 270)]), L(64, "Elu"), L(19), L(512, "Elu", [(0, 45), RUN]),
                           L(256, "Elu"), L(128, "Elu"), L(12)]),
    # two parts out of order; K = 114; non-uniform widths; a 5-wide head
    "ea_two": (98, None, [L(100, "Tanh", [(0, 98)]), L(16, "Tanh"), L(200, "Tanh", [(49, 98), (0, 49), RUN]),
                          L(33, "Tanh"), L(5)]),
    # the whole normalised observation as the part: the prologue on the skip path
    "ea_front": (98, "norm", [L(256, "Elu", [(0, 98)]), L(128, "Elu"), L(35, "Elu"),
                              L(256, "Elu", [RUN, (0, 98)]), L(256, "Elu"), L(12)]),
    # the skip columns land where the previous layer's store wrote Sigmoid(0) = 0.5
    "ea_sig": (48, None, [L(64, "Sigmoid", [(0, 48)]), L(20, "Sigmoid"), L(64, "Sigmoid", [RUN, (0, 48)]), L(12)]),
    # layer 0 reads obs[49:98] only: a gather
    "ea_l0slice": (98, None, [L(64, "Elu", [(49, 98)]), L(16, "Elu"), L(64, "Elu", [(0, 49), RUN]), L(12)]),
    # the skip on the head
    "ea_head": (48, None, [L(64, "Elu", [(0, 48)]), L(8, "Elu"), L(12, None, [RUN, (0, 12)])]),
    # ea_98 with a post-LN on the encoder's 32-wide layer and a pre-LN on the 128-wide skip layer
    "ea_ln": (98, None, [L(64, "Elu", [(0, 98)]), L(32, "Elu", ln="post"), L(19),
                         L(128, "Elu", [RUN, (0, 49)], ln="pre"), L(64, "Elu"), L(12)]),
}
NAMES = tuple(SPECS)
SEED = {n: 9100 + i for i, n in enumerate(NAMES)}

# integer probes (below): one shaped like ea_k64's Concat (observation first), one with a
# layer-0 gather, two skip layers and a skip on the head
PROBE_SPECS = {
    "probe_k64": (60, None, [L(32, "Relu", [(0, 60)]), L(19, "Relu"), L(64, "Relu", [(0, 45), RUN]), L(8)]),
    "probe_gather": (60, None, [L(24, "Relu", [(20, 50)]), L(32, "Relu", [(0, 20), RUN, (50, 60)]),
                                L(6, None, [RUN, (5, 9)])]),
}
PROBES = tuple(PROBE_SPECS)

PARITY_BATCHES = (1, 5, 8, 9, 16, 17, 33)


def spec(name):
    return SPECS[name] if name in SPECS else PROBE_SPECS[name]


def in_dim(name: str) -> int:
    return spec(name)[0]


def _part_width(p, prev_n):
    return prev_n if p == RUN else p[1] - p[0]


def layer_k(layers, l):
    prev_n = layers[l - 1]["n"] if l else 0
    return sum(_part_width(p, prev_n) for p in layers[l]["inp"])


def weights(name: str):
    """[(W [N, K] in ONNX (Concat) column order, b [N], LN scale, LN bias)] per layer."""
    _, _, layers = spec(name)
    if name in PROBE_SPECS:
        return _probe_weights(name)
    rng = np.random.default_rng(SEED[name])
    out = []
    for l, ly in enumerate(layers):
        K, N = layer_k(layers, l), ly["n"]
        a = 1.0 / np.sqrt(K)
        W = rng.uniform(-a, a, (N, K)).astype(np.float32)
        b = rng.uniform(-a, a, N).astype(np.float32)
        g = rng.uniform(0.75, 1.25, N).astype(np.float32) if ly["ln"] else None
        c = rng.uniform(-0.25, 0.25, N).astype(np.float32) if ly["ln"] else None
        out.append((W, b, g, c))
    return out


def front_constants(name: str):
    """(mean, std, clip) of a "norm" front, else None."""
    F, front, _ = spec(name)
    if front != "norm":
        return None
    rng = np.random.default_rng(SEED[name] + 50)
    return (rng.uniform(-0.5, 0.5, F).astype(np.float32), rng.uniform(0.5, 2.0, F).astype(np.float32), 5.0)


def model_bytes(name: str) -> bytes:
    F, front, layers = spec(name)
    nodes, inits = [], [("ax1", np.array([1], np.int64))]
    x0 = "observation"
    if front == "norm":
        mean, std, clip = front_constants(name)
        inits += [("obs_mean", mean), ("obs_std", std), ("clip_lo", np.array(-clip, np.float32)),
                  ("clip_hi", np.array(clip, np.float32))]
        nodes += [ow.node("Sub", ["observation", "obs_mean"], ["centred"], "sub"),
                  ow.node("Div", ["centred", "obs_std"], ["scaled"], "div"),
                  ow.node("Clip", ["scaled", "clip_lo", "clip_hi"], ["x0"], "clip")]
        x0 = "x0"
    cur = None
    n_slice = 0
    for l, (ly, (W, b, g, c)) in enumerate(zip(layers, weights(name))):
        names = []
        for p in ly["inp"]:
            if p == RUN:
                names.append(cur)
            elif p == (0, F):
                names.append(x0)
            else:
                out = f"part{n_slice}"
                if n_slice % 3 == 2:  # one in three in the opset 1-9 attribute form
                    nodes.append(ow.node("Slice", [x0], [out], f"slice{n_slice}",
                                         [ow.attr_ints("starts", [p[0]]), ow.attr_ints("ends", [p[1]]),
                                          ow.attr_ints("axes", [1])]))
                else:
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

        def ln_node(src, dst):
            inits.extend([(f"lng{l}", g), (f"lnb{l}", c)])
            nodes.append(ow.node("LayerNormalization", [src, f"lng{l}", f"lnb{l}"], [dst], f"ln{l}",
                                 [ow.attr_int("axis", -1), ow.attr_float("epsilon", 1e-5)]))

        if ly["ln"] == "pre":
            ln_node(y, f"n{l}")
            y = f"n{l}"
        if ly["act"]:
            out = "action" if last else f"a{l}"
            nodes.append(ow.node(ly["act"], [y], [out], f"act{l}"))
            y = out
        if ly["ln"] == "post":
            ln_node(y, f"n{l}")
            y = f"n{l}"
        cur = y
    return ow.model(nodes, inits, [("observation", ["batch", F])], [("action", ["batch", layers[-1]["n"]])])


def model_path(name: str, directory) -> str:
    path = os.path.join(str(directory), name + ".onnx")
    if not os.path.exists(path):
        with open(path, "wb") as fh:
            fh.write(model_bytes(name))
    return path


def expected_view(name: str):
    """What inspect_model must report per layer: K, N, act, ln, skip (device order)."""
    F, _, layers = spec(name)
    out = []
    for l, ly in enumerate(layers):
        if l == 0:
            (b, e), = ly["inp"]
            skip = [] if (b, e) == (0, F) else list(range(b, e))
        else:
            skip = [c for p in ly["inp"] if p != RUN for c in range(p[0], p[1])]
        out.append(dict(K=layer_k(layers, l), N=ly["n"], act=ACT_CODE[ly["act"]],
                        ln={None: 0, "pre": 1, "post": 2}[ly["ln"]], skip=skip))
    return out


def device_weights(name: str):
    """Each layer's W with its columns in device order (running value first, then the parts in
    Concat order): what the loader's w_sum is taken of, and what the kernels multiply."""
    _, _, layers = spec(name)
    out = []
    for l, (ly, (W, _, _, _)) in enumerate(zip(layers, weights(name))):
        prev_n = layers[l - 1]["n"] if l else 0
        at, run_cols, part_cols = 0, [], []
        for p in ly["inp"]:
            w = _part_width(p, prev_n)
            (run_cols if p == RUN else part_cols).extend(range(at, at + w))
            at += w
        out.append(W[:, run_cols + part_cols])
    return out


def seed_of(name: str, B: int, k: int = 0) -> int:
    names = NAMES + PROBES
    return 52000 + 1000 * names.index(name) + 50 * k + B


def obs(name: str, B: int, k: int = 0) -> np.ndarray:
    """N(0, 1) observations [B, in_dim] float32, a fixed function of (model, B, k); a "norm"
    front's model gets 3 N(0, 1) so that its Clip binds on some elements."""
    rng = np.random.default_rng(seed_of(name, B, k))
    scale = 3.0 if spec(name)[1] == "norm" else 1.0
    return (rng.standard_normal((B, in_dim(name))) * scale).astype(np.float32)


# ---------------------------------------------------------------------------
# integer probes: integer weights, biases and observations, Relu: every partial sum is an
# integer below 2^24, so float32 arithmetic is exact in any summation order and a kernel
# must return the int64 answer bit for bit.
PROBE_OBS_MAX = 3


def _probe_weights(name: str):
    _, _, layers = PROBE_SPECS[name]
    # (seeds at which no hidden unit is dead on every row of the B = 33 input: tests/test_cpu_skip.py)
    rng = np.random.default_rng({"probe_k64": 80, "probe_gather": 77}[name])
    out = []
    for l, ly in enumerate(layers):
        K, N = layer_k(layers, l), ly["n"]
        W = rng.integers(-2, 3, (N, K)) if l == 0 else rng.integers(-1, 2, (N, K))  # (keeps the sums below 2^24)
        W[W == 0] = 1  # every input column is read by every unit
        b = rng.integers(-4, 5, N)
        out.append((W.astype(np.float32), b.astype(np.float32), None, None))
    return out


def probe_obs(name: str, B: int) -> np.ndarray:
    rng = np.random.default_rng(seed_of(name, B))
    return rng.integers(-PROBE_OBS_MAX, PROBE_OBS_MAX + 1, (B, in_dim(name))).astype(np.float32)


def probe_forward(name: str, x, zero=None) -> np.ndarray:
    """The probe's answer in int64. zero = (l, j): unit j of layer l's output (l = -1:
    observation column j) is replaced by 0."""
    _, _, layers = PROBE_SPECS[name]
    x0 = np.asarray(x).astype(np.int64)
    if zero and zero[0] == -1:
        x0 = x0.copy()
        x0[:, zero[1]] = 0
    cur = None
    for l, (ly, (W, b, _, _)) in enumerate(zip(layers, weights(name))):
        xin = np.concatenate([cur if p == RUN else x0[:, p[0]:p[1]] for p in ly["inp"]], axis=1)
        y = xin @ W.astype(np.int64).T + b.astype(np.int64)
        if ly["act"] == "Relu":
            y = np.maximum(y, 0)
        else:
            assert ly["act"] is None
        if zero and zero[0] == l:
            y[:, zero[1]] = 0
        cur = y
    return cur


def probe_bound(name: str) -> int:
    """The largest sum |w| |h| + |b| any unit of the probe can reach, from |obs| <= 3: an upper
    bound of every partial sum in any order."""
    _, _, layers = PROBE_SPECS[name]
    worst, cur = 0, None
    for l, (ly, (W, b, _, _)) in enumerate(zip(layers, weights(name))):
        prev_n = layers[l - 1]["n"] if l else 0
        h = np.concatenate([cur if p == RUN else np.full(_part_width(p, prev_n), PROBE_OBS_MAX, np.int64)
                            for p in ly["inp"]])
        cur = np.abs(W.astype(np.int64)) @ h + np.abs(b.astype(np.int64))
        worst = max(worst, int(cur.max()))
    return worst
