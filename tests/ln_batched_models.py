"""The models and inputs of the batched LayerNormalization pipeline tests
(Engine(ln_batched=True): policy_mlp_ln_kernel<tiles per wave, head tiles>), in one place for
tests/test_cpu_layernorm_batched.py (the plan, the input condition) and
tests/test_gpu_layernorm_batched.py.

Three models come from the registry (synth.MODELS); five are built here with
synth.mlp_model_bytes and written under a test's tmp_path, so that the registry, and the
golden hashes made from it, stay as they are.

cases() lists every (model, batch, seed, scale) the GPU tests feed; the CPU test checks on
exactly those that fp32 arithmetic alone stays under a third of the tolerance.
"""
from __future__ import annotations

import os

import numpy as np

import ln_ref

TOL = 1e-5
GENERAL = "policy_fused_kernel<8, 0, 0, 0, 0,"  # the general body's name starts so

# (ln_pre_small: 100 and 72 columns, both under the 128 pad, so the planner's shape rule,
# every hidden layer's ceil64(N) the same 64 * TPW, serves it as it serves lnb_t4_mask)
REGISTRY_MODELS = ("ln_512_pre", "ln_ctl_post", "ln_pre_small")

# name -> (mlp_model_bytes keyword arguments, the LN mode inspect_model reports per layer)
NEW_MODELS = {
    # two true widths under one 256 pad; the columns a Sigmoid + post-LN excludes hold 0.5
    "lnb_t4_mask": (dict(dims=(20, 200, 250, 9), seed=50, act="Sigmoid", layer_norm="post"), [2, 2, 0]),
    # LN and LN-free layers in one policy: the register hand-off on both
    "lnb_t4_some": (dict(dims=(48, 256, 256, 256, 12), seed=51, act="Tanh", layer_norm=("pre", None, "pre")),
                    [1, 0, 1, 0]),
    # a two-tile head, an LN without B
    "lnb_t2_h2": (dict(dims=(33, 128, 128, 20), seed=52, act="Relu", layer_norm="pre", ln_bias=(True, False)),
                  [1, 1, 0]),
    # one hidden layer: LN straight into the head, 500 of 512 columns
    "lnb_t8_nl2": (dict(dims=(64, 500, 12), seed=53, act="Elu", layer_norm="post"), [2, 0]),
    # both modes in one policy, an epsilon per layer
    "lnb_t8_eps": (dict(dims=(48, 512, 512, 12), seed=54, act="LeakyRelu", layer_norm=("post", "pre"),
                        ln_eps=(1e-5, 1e-3)), [2, 1, 0]),
}
LN_MODES = dict({"ln_512_pre": [1, 1, 1, 0], "ln_ctl_post": [2, 2, 2, 0], "ln_pre_small": [1, 1, 0]}, **{k: v[1] for k, v in NEW_MODELS.items()})
ALL_MODELS = REGISTRY_MODELS + tuple(NEW_MODELS)

# the kernel Engine(ln_batched=True).batched_kernel names
KERNEL = {
    "ln_512_pre": "policy_mlp_ln_kernel<8, 1>",
    "ln_ctl_post": "policy_mlp_ln_kernel<2, 1>",
    "ln_pre_small": "policy_mlp_ln_kernel<2, 1>",
    "lnb_t4_mask": "policy_mlp_ln_kernel<4, 1>",
    "lnb_t4_some": "policy_mlp_ln_kernel<4, 1>",
    "lnb_t2_h2": "policy_mlp_ln_kernel<2, 2>",
    "lnb_t8_nl2": "policy_mlp_ln_kernel<8, 1>",
    "lnb_t8_eps": "policy_mlp_ln_kernel<8, 1>",
}

PARITY_BATCHES = (1, 15, 16, 17, 33)   # the tile edge and a partial tile
HANDOVER_MODELS = ("ln_ctl_post", "ln_512_pre")
HANDOVER_BATCHES = (3, 8, 9)           # 8 / 9: the single launch and the hand-over; 3: run_torch
WORKLOAD_ROWS = 4097                   # one workgroup per CU ... and one row more
SHARD_MODELS = ("ln_512_pre", "lnb_t4_mask")
SHARD_ROWS = 1024
SHARDS = ((0, 512), (17, 530), (1000, 1024))
SEQ_MODEL, SEQ_STEPS, SEQ_ROWS = "lnb_t4_some", 3, 100
EPS_MODEL, EPS_ROWS, EPS_SEED, EPS_SCALE = "lnb_t8_eps", 20, 77, 1e-2
NAN_MODEL, NAN_ROWS, NAN_ROW = "lnb_t4_mask", 33, 5


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


def dims(name: str):
    if name in NEW_MODELS:
        return NEW_MODELS[name][0]["dims"]
    return {"ln_512_pre": (48, 512, 512, 512, 12), "ln_ctl_post": (98, 128, 128, 128, 12),
            "ln_pre_small": (40, 100, 72, 12)}[name]


def seed_of(name: str, B: int) -> int:
    return 90000 + 10000 * ALL_MODELS.index(name) + B


def obs(name: str, B: int, seed: int | None = None, scale: float = 1.0) -> np.ndarray:
    """N(0, 1) * scale observations [B, in_dim] float32, a fixed function of (model, B)."""
    return ln_ref.obs_for(name, B, dims(name)[0], scale, seed_of(name, B) if seed is None else seed)


def cases():
    """Every (model, batch, seed, scale) the GPU tests feed, each once."""
    out = set()
    for name in ALL_MODELS:
        for B in PARITY_BATCHES:
            out.add((name, B, seed_of(name, B), 1.0))
    for name in HANDOVER_MODELS:
        for B in HANDOVER_BATCHES:
            out.add((name, B, seed_of(name, B), 1.0))
    out.add(("ln_512_pre", WORKLOAD_ROWS, seed_of("ln_512_pre", WORKLOAD_ROWS), 1.0))
    for name in SHARD_MODELS:
        out.add((name, SHARD_ROWS, seed_of(name, SHARD_ROWS), 1.0))
    out.add((SEQ_MODEL, SEQ_STEPS * SEQ_ROWS, seed_of(SEQ_MODEL, SEQ_STEPS * SEQ_ROWS), 1.0))
    out.add((EPS_MODEL, EPS_ROWS, EPS_SEED, EPS_SCALE))
    out.add((NAN_MODEL, NAN_ROWS, seed_of(NAN_MODEL, NAN_ROWS), 1.0))
    return sorted(out)


def zero_variance_model():
    """(model bytes, the action every observation gives): 10 -> 100 -> 5, layer 0 with zero
    weights and the bias 0.625, then a pre-LN over N = 100 columns under a 128 pad
    (tests/test_gpu_layernorm.py's construction). 0.625 * 100 / 100 is exact in fp32, so the
    variance is exactly 0, the layer's output is its LN bias and the action is W2 . b_ln + b2."""
    from go2_onnx_controller_amd import onnx_writer as ow
    rng = np.random.default_rng(3)
    N = 100
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
