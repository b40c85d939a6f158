"""Estimator-actor policies for the small-batch kernels (GO2PI_SKIP_SMALL): the models of
tests/skip_models.py, and three more at the smallest shapes where the single launch and the
multi-workgroup resident kernel can go wrong with a skip input and the GEMV chain cannot.

The new models are described and built as skip_models builds its own (a list of layers whose
input is a list of parts; ONNX bytes, the loader's view and, for the integer probes, an int64
evaluation all derive from that description); every function here takes any name, of either
module. None of these models is in synth.MODELS.
"""
from __future__ import annotations

import os

import numpy as np

import skip_models as sm
from go2_onnx_controller_amd import onnx_writer as ow
from skip_models import RUN, L

SPECS = {
    # the skip layer's K = 598 -> K_pad 640 > 512: at batch 5 and up its rows pass the 4096
    # granules of one sweep round, and the skip columns sit past them
    "ea_round2": (98, None, [L(64, "Elu", [(0, 98)]), L(500, "Elu"), L(64, "Elu", [RUN, (0, 98)]), L(12)]),
}
PROBE_SPECS = {
    # layer 0: K_pad 128 (8 chunks), N_pad = ceil64(max(100, 120)) = 128 -> 4 slices of 2
    # chunks: the resident kernel's local layer 0 (NF = 8), a skip on the layer behind it
    "probe_local0": (98, None, [L(100, "Relu", [(0, 98)]), L(64, "Relu", [RUN, (10, 30)]), L(8)]),
    # a layer-0 gather of the same geometry (K_pad 128, N_pad 128): must run tiled; parts in
    # front of and behind the running value; a skip on the head
    "probe_gather0": (100, None, [L(120, "Relu", [(2, 98)]), L(32, "Relu", [(98, 100), RUN, (0, 2)]),
                                  L(6, None, [RUN, (5, 9)])]),
}
NEW_NAMES = tuple(SPECS)
NEW_PROBES = tuple(PROBE_SPECS)
NAMES = sm.NAMES + NEW_NAMES          # float parity
PROBES = sm.PROBES + NEW_PROBES       # exact
SEED = {"ea_round2": 9300}
# (seeds at which no hidden unit is dead on every row of the B = 33 input and every column
# read changes an output: tests/test_cpu_skip_small.py)
PROBE_SEED = {"probe_local0": 1, "probe_gather0": 1}

SMALL_BATCHES = (1, 5, 8)
PROBE_BATCHES = (8, 1, 5, 7, 4, 8)  # tests/test_gpu_probe_shapes.py's order: stale rows of a larger request


def _new(name):
    return name in SPECS or name in PROBE_SPECS


def spec(name):
    return SPECS[name] if name in SPECS else PROBE_SPECS[name] if name in PROBE_SPECS else sm.spec(name)


def in_dim(name):
    return spec(name)[0]


def weights(name):
    """[(W [N, K] in ONNX (Concat) column order, b [N], None, None)] per layer (skip_models.weights)."""
    if not _new(name):
        return sm.weights(name)
    _, _, layers = spec(name)
    out = []
    if name in PROBE_SPECS:
        rng = np.random.default_rng(PROBE_SEED[name])
        for l, ly in enumerate(layers):
            K, N = sm.layer_k(layers, l), ly["n"]
            W = rng.integers(-2, 3, (N, K)) if l == 0 else rng.integers(-1, 2, (N, K))  # (keeps the sums below 2^24)
            W[W == 0] = 1  # every input column is read by every unit
            b = rng.integers(-4, 5, N)
            out.append((W.astype(np.float32), b.astype(np.float32), None, None))
        return out
    rng = np.random.default_rng(SEED[name])
    for l, ly in enumerate(layers):
        K, N = sm.layer_k(layers, l), ly["n"]
        a = 1.0 / np.sqrt(K)
        out.append((rng.uniform(-a, a, (N, K)).astype(np.float32), rng.uniform(-a, a, N).astype(np.float32), None, None))
    return out


def model_bytes(name):
    if not _new(name):
        return sm.model_bytes(name)
    F, _, layers = spec(name)
    nodes, inits = [], [("ax1", np.array([1], np.int64))]
    cur, n_slice = None, 0
    for l, (ly, (W, b, _, _)) in enumerate(zip(layers, weights(name))):
        names = []
        for p in ly["inp"]:
            if p == RUN:
                names.append(cur)
            elif p == (0, F):
                names.append("observation")
            else:
                out = f"part{n_slice}"
                inits += [(f"st{n_slice}", np.array([p[0]], np.int64)), (f"en{n_slice}", np.array([p[1]], np.int64))]
                nodes.append(ow.node("Slice", ["observation", f"st{n_slice}", f"en{n_slice}", "ax1"], [out], f"slice{n_slice}"))
                n_slice += 1
                names.append(out)
        x = names[0]
        if len(names) > 1:
            x = f"cat{l}"
            nodes.append(ow.node("Concat", names, [x], x, [ow.attr_int("axis", 1)]))
        last = l == len(layers) - 1
        inits += [(f"w{l}", W), (f"b{l}", b)]
        y = "action" if last and not ly["act"] else f"g{l}"
        nodes.append(ow.node("Gemm", [x, f"w{l}", f"b{l}"], [y], f"gemm{l}", [ow.attr_int("transB", 1)]))
        if ly["act"]:
            out = "action" if last else f"a{l}"
            nodes.append(ow.node(ly["act"], [y], [out], f"act{l}"))
            y = out
        cur = y
    return ow.model(nodes, inits, [("observation", ["batch", F])], [("action", ["batch", layers[-1]["n"]])])


def model_path(name, directory):
    path = os.path.join(str(directory), name + ".onnx")
    if not os.path.exists(path):
        with open(path, "wb") as fh:
            fh.write(model_bytes(name))
    return path


def expected_view(name):
    """What inspect_model must report per layer (skip_models.expected_view)."""
    if not _new(name):
        return sm.expected_view(name)
    F, _, layers = spec(name)
    out = []
    for l, ly in enumerate(layers):
        if l == 0:
            (b, e), = ly["inp"]
            skip = [] if (b, e) == (0, F) else list(range(b, e))
        else:
            skip = [c for p in ly["inp"] if p != RUN for c in range(p[0], p[1])]
        out.append(dict(K=sm.layer_k(layers, l), N=ly["n"], act=sm.ACT_CODE[ly["act"]], ln=0, skip=skip))
    return out


def seed_of(name, B, k=0):
    if not _new(name):
        return sm.seed_of(name, B, k)
    return 62000 + 1000 * (NEW_NAMES + NEW_PROBES).index(name) + 50 * k + B


def obs(name, B, k=0):
    """N(0, 1) observations [B, in_dim] float32, a fixed function of (model, B, k)."""
    if not _new(name):
        return sm.obs(name, B, k)
    return np.random.default_rng(seed_of(name, B, k)).standard_normal((B, in_dim(name))).astype(np.float32)


def probe_obs(name, B):
    if not _new(name):
        return sm.probe_obs(name, B)
    rng = np.random.default_rng(seed_of(name, B))
    return rng.integers(-sm.PROBE_OBS_MAX, sm.PROBE_OBS_MAX + 1, (B, in_dim(name))).astype(np.float32)


def probe_forward(name, x, zero=None):
    """The probe's answer in int64 (skip_models.probe_forward). zero = (l, j): unit j of layer
    l's output (l = -1: observation column j) is replaced by 0."""
    if not _new(name):
        return sm.probe_forward(name, x, zero)
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


def probe_bound(name):
    """The largest sum |w| |h| + |b| any unit of the probe can reach, from |obs| <= 3."""
    if not _new(name):
        return sm.probe_bound(name)
    _, _, layers = PROBE_SPECS[name]
    worst, cur = 0, None
    for l, (ly, (W, b, _, _)) in enumerate(zip(layers, weights(name))):
        h = np.concatenate([cur if p == RUN else np.full(p[1] - p[0], sm.PROBE_OBS_MAX, np.int64) for p in ly["inp"]])
        cur = np.abs(W.astype(np.int64)) @ h + np.abs(b.astype(np.int64))
        worst = max(worst, int(cur.max()))
    return worst


def read_columns(name):
    """The observation columns any layer of the model reads."""
    F, _, layers = spec(name)
    return sorted({c for ly in layers for p in ly["inp"] if p != RUN for c in range(p[0], p[1])})
