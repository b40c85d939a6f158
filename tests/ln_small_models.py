"""The models and inputs of the LayerNormalization small-batch tests (Engine(ln_small=True):
the single-launch kernel and the resident kernels at batch <= 8).

Six models come from the registry (synth.MODELS, through tests/ln_ref.py); three more are
built here with synth.mlp_model_bytes and written under a test's tmp_path, so that the
registry, and the golden hashes made from it, stay as they are. The three cover the
act1 shapes the registry's models do not: hidden width 64, the two-layer program (the
shortest barrier chain of policy_act1_kernel) and four layer-0 float4s per lane.

cases() lists every (model, batch, seed) the GPU tests feed; tests/test_cpu_layernorm_small.py
checks on exactly those that fp32 arithmetic alone stays under a third of the tolerance.
"""
from __future__ import annotations

import os

import numpy as np

import ln_ref

REGISTRY_MODELS = ("ln_pre_small", "ln_post_small", "ln_mixed", "ln_512_pre", "ln_ctl_post", "ln_wide_pre")

# name -> (mlp_model_bytes keyword arguments, the LN mode inspect_model reports per layer)
NEW_MODELS = {
    # act1 <3, 64, F0 = 1>: statistics over 40 of 64 columns on the second layer
    "ln_a1_64": (dict(dims=(24, 40, 64, 6), seed=40, act="Tanh", layer_norm=("pre", "post")), [1, 2, 0]),
    # act1 <2, 64, 1>: one wide layer, the shortest barrier chain
    "ln_a1_nl2": (dict(dims=(20, 50, 5), seed=41, layer_norm="pre"), [1, 0]),
    # act1 <3, 64, 4>: layer 0 reads four float4s per lane
    "ln_a1_f4": (dict(dims=(200, 64, 64, 12), seed=42, act="Relu", layer_norm="post"), [2, 2, 0]),
}
ALL_MODELS = REGISTRY_MODELS + tuple(NEW_MODELS)

# what serves go2pi_run at batch <= 8 with ln_small = 1 and resident_ms > 0, read from
# plan.cpp's selection and resident.hip's act1_shape / launch_resident
RESIDENT_FORM = {
    "ln_pre_small": "policy_act1_kernel",    # <3, 128, 1>: 100 and 72 of 128 columns
    "ln_ctl_post": "policy_act1_kernel",     # <4, 128, 2>, generic (not the Elu specialisation)
    "ln_post_small": "policy_resident_kernel",  # multi-workgroup, tiled layer 0
    "ln_mixed": "policy_resident_kernel",
    "ln_wide_pre": "policy_resident_kernel",    # ... and ln_rows' > 512-column path
    "ln_512_pre": "policy_resident_kernel",     # multi-workgroup LOCAL0, NF = 16 (not the wide kernel)
    "ln_a1_64": "policy_act1_kernel",
    "ln_a1_nl2": "policy_act1_kernel",
    "ln_a1_f4": "policy_act1_kernel",
}
ACT1_MODELS = tuple(n for n in ALL_MODELS if RESIDENT_FORM[n] == "policy_act1_kernel")
MULTI_MODELS = tuple(n for n in ALL_MODELS if RESIDENT_FORM[n] == "policy_resident_kernel")

LAUNCH_BATCHES = (1, 2, 5, 8, 9, 40)   # single launch (<= 8) and the hand-over to the batched body
RESIDENT_REQUESTS = 40                 # requests per resident run, batches cycling through 1 .. 8
BITWISE_MODELS = ("ln_ctl_post", "ln_512_pre")
BITWISE_BATCHES = (1, 8)


def model_bytes(name: str) -> bytes:
    from go2_onnx_controller_amd import synth
    if name in NEW_MODELS:
        return synth.mlp_model_bytes(**NEW_MODELS[name][0])
    return synth.MODELS[name]()


def model_path(name: str, directory) -> str:
    """The .onnx file of `name`: the registry's own for its models, else written under
    `directory` (a test's tmp_path)."""
    from go2_onnx_controller_amd import synth
    if name not in NEW_MODELS:
        return synth.ensure_model(name)
    path = os.path.join(str(directory), name + ".onnx")
    if not os.path.exists(path):
        with open(path, "wb") as fh:
            fh.write(model_bytes(name))
    return path


def in_dim(name: str) -> int:
    if name in NEW_MODELS:
        return NEW_MODELS[name][0]["dims"][0]
    return {"ln_pre_small": 40, "ln_post_small": 33, "ln_mixed": 30, "ln_512_pre": 48, "ln_ctl_post": 98,
            "ln_wide_pre": 24}[name]


def _base(name: str) -> int:
    return 7000 + 100 * ALL_MODELS.index(name)


def launch_seed(name: str, B: int) -> int:
    return _base(name) + B


def resident_batches():
    """The batch of each request of a resident run: 1 .. 8 mixed, every size five times."""
    return [1 + (3 * i + i // 8) % 8 for i in range(RESIDENT_REQUESTS)]


def resident_seed(name: str, i: int) -> int:
    return _base(name) + 50 + i  # a fresh observation each request


def bitwise_seed(name: str, B: int) -> int:
    return _base(name) + 90 + B


def obs(name: str, B: int, seed: int) -> np.ndarray:
    return ln_ref.obs_for(name, B, in_dim(name), 1.0, seed)


def cases():
    """Every (model, batch, seed) the GPU tests feed, each once."""
    out = set()
    for name in ALL_MODELS:
        for B in LAUNCH_BATCHES:
            out.add((name, B, launch_seed(name, B)))
        for i, B in enumerate(resident_batches()):
            out.add((name, B, resident_seed(name, i)))
    for name in BITWISE_MODELS:
        for B in BITWISE_BATCHES:
            out.add((name, B, bitwise_seed(name, B)))
    return sorted(out)


DROPIN_TICKS = 200


def dropin_observations(ticks: int = DROPIN_TICKS) -> np.ndarray:
    """The observation of each tick of tests/cpp/controller_shape.cpp's "ticks" mode: the
    same float32 in-place updates as its loop (observation[t % 98] += 0.001f)."""
    o, seq = np.zeros(98, np.float32), np.empty((ticks, 98), np.float32)
    for t in range(ticks):
        o[t % 98] += np.float32(0.001)
        seq[t] = o
    return seq


def zero_variance_model():
    """(model bytes, the action every observation gives): layer 0 has zero weights and a
    constant bias, then a pre-LN, so the variance is exactly 0, the layer's output is its
    LN bias and the action is W2 . b_ln + b2 (tests/test_gpu_layernorm.py's known answer).
    10 -> 72 -> 5: the act1 shape <2, 128, 1>."""
    from go2_onnx_controller_amd import onnx_writer as ow
    rng = np.random.default_rng(3)
    N = 72
    g = rng.uniform(0.75, 1.25, N).astype(np.float32)
    b_ln = rng.uniform(-0.25, 0.25, N).astype(np.float32)
    W2 = (rng.standard_normal((5, N)) / 8).astype(np.float32)
    b2 = rng.standard_normal(5).astype(np.float32)
    inits = [("w0", np.zeros((N, 10), np.float32)), ("b0", np.full(N, 0.625, np.float32)), ("g", g), ("c", b_ln),
             ("w2", W2), ("b2", b2)]
    nodes = [ow.node("Gemm", ["observation", "w0", "b0"], ["a"], "g0", [ow.attr_int("transB", 1)]),
             ow.node("LayerNormalization", ["a", "g", "c"], ["n"], "ln", [ow.attr_int("axis", -1)]),
             ow.node("Gemm", ["n", "w2", "b2"], ["action"], "g1", [ow.attr_int("transB", 1)])]
    model = ow.model(nodes, inits, [("observation", ["batch", 10])], [("action", ["batch", 5])])
    return model, W2.astype(np.float64) @ b_ln.astype(np.float64) + b2


# A layer wider than 512 without LayerNormalization: at batch 7 and 8 its input rows are
# more than the 4096 granules the eight sweeping waves of policy_latency_kernel /
# policy_resident_kernel take in one round (the rows past them were left unswept before
# the sweep looped; ln_wide_pre is the LN model of the same width).
PLAIN_WIDE = dict(dims=(24, 600, 8), seed=44, act="Tanh")
PLAIN_WIDE_SEED = 7990


def plain_wide_obs(B: int) -> np.ndarray:
    return ln_ref.obs_for("plain_wide", B, 24, 1.0, PLAIN_WIDE_SEED + B)
