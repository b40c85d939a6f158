"""Reference for policies with ONNX LayerNormalization (opset 17), for the tests.

oracle/onnx_ref.py has no LayerNormalization, so the graph is evaluated here: node by
node from the .onnx file's own nodes and initialisers (parsed by oracle.onnx_ref.load),
LayerNormalization in numpy below, every other operator through oracle.onnx_ref.run on
a single-node graph. dtype float64 is the reference; float32 shows what the number
format alone costs (the input condition of tests/test_cpu_layernorm.py).
"""
from __future__ import annotations

import numpy as np

from oracle import onnx_ref


def layer_norm(x, scale, bias=None, eps=1e-5, dtype=np.float64):
    """ONNX LayerNormalization over the last axis: biased variance of x - mean (two
    passes), y = (x - mean) / sqrt(var + eps) * scale + bias, all in `dtype`."""
    dt = np.dtype(dtype)
    x = np.asarray(x, dt)
    mean = x.mean(axis=-1, keepdims=True, dtype=dt)
    d = x - mean
    var = (d * d).mean(axis=-1, keepdims=True, dtype=dt)
    y = d / np.sqrt(var + dt.type(eps)) * np.asarray(scale, dt)
    if bias is not None:
        y = y + np.asarray(bias, dt)
    return y.astype(dt)


def _ln_node(nd, env, dt):
    x = env[nd.inputs[0]]
    axis = int(nd.attrs.get("axis", -1))
    if axis not in (-1, x.ndim - 1):
        raise NotImplementedError(f"ln_ref: LayerNormalization axis {axis} of a rank-{x.ndim} value")
    if int(nd.attrs.get("stash_type", 1)) != 1:
        raise NotImplementedError("ln_ref: stash_type != 1")
    if any(o for o in nd.outputs[1:]):
        raise NotImplementedError("ln_ref: Mean / InvStdDev outputs")
    bias = env[nd.inputs[2]] if len(nd.inputs) > 2 and nd.inputs[2] else None
    # the attribute is a float32 in the file; the engine reads that same value
    eps = float(np.float32(nd.attrs.get("epsilon", 1e-5)))
    return {nd.outputs[0]: layer_norm(x, env[nd.inputs[1]], bias, eps, dt)}


def run(g, feeds: dict, dtype=np.float64) -> dict:
    """Evaluate graph `g` (oracle.onnx_ref.Graph) in `dtype`: {output name: array}."""
    dt = np.dtype(dtype)
    env = {k: (v.astype(dt) if v.dtype != np.int64 else v) for k, v in g.inits.items()}
    env.update({k: np.asarray(v, dtype=dt) for k, v in feeds.items()})
    for nd in g.nodes:
        if nd.op_type == "LayerNormalization":
            env.update(_ln_node(nd, env, dt))
            continue
        one = onnx_ref.Graph([nd], {k: env[k] for k in nd.inputs if k and env[k].dtype == np.int64}, [],
                             [(o, None) for o in nd.outputs if o])
        env.update(onnx_ref.run(one, {k: env[k] for k in nd.inputs if k and env[k].dtype != np.int64}, dt))
    return {name: env[name] for name, _ in g.outputs}


class LnRef:
    """A loaded policy: f64(obs) / f32(obs) -> action [B, out]; a recurrent one is stepped
    with step(obs, h) -> (action, h'), h [B, H]."""

    def __init__(self, path_or_bytes):
        self.g = onnx_ref.load(path_or_bytes)
        self.obs_name = self.g.inputs[0][0]
        self.act_name = self.g.outputs[0][0]
        self.recurrent = len(self.g.inputs) > 1

    def _act(self, x, dtype):
        x = np.asarray(x, np.float32)
        return run(self.g, {self.obs_name: x}, dtype)[self.act_name]

    def f64(self, x):
        return self._act(x, np.float64)

    def f32(self, x):
        return self._act(x, np.float32)

    def step(self, x, h, dtype=np.float64):
        out = run(self.g, {self.obs_name: np.asarray(x, np.float32), self.g.inputs[1][0]: np.asarray(h)[None]}, dtype)
        return out[self.act_name], out[self.g.outputs[1][0]][0]

    def rollout(self, xs, h0, dtype=np.float64):
        """xs [T, B, I], h0 [B, H] -> (actions [T, B, out], h_T)."""
        h, ys = np.asarray(h0, dtype), []
        for x in xs:
            y, h = self.step(x, h, dtype)
            ys.append(y)
        return np.stack(ys), h


# The (model, batch, seed, scale) inputs of the GPU tests, in one place so that
# tests/test_cpu_layernorm.py checks the input condition on exactly what the GPU sees.
MLP_MODELS = ("ln_pre_small", "ln_post_small", "ln_mixed", "ln_512_pre", "ln_ctl_post", "ln_wide_pre")
ALL_MODELS = MLP_MODELS + ("gru_ln",)
PARITY_BATCHES = (1, 5, 8, 9, 16, 17, 33, 100)


def seed_of(name: str, B: int) -> int:
    return 1000 * ALL_MODELS.index(name) + B


def obs_for(name: str, B: int, in_dim: int, scale: float = 1.0, seed: int | None = None) -> np.ndarray:
    """N(0, 1) * scale observations [B, in_dim] float32, a fixed function of (model, B)."""
    rng = np.random.default_rng(seed_of(name, B) if seed is None else seed)
    return (rng.standard_normal((B, in_dim)) * scale).astype(np.float32)


def ctl_inputs(B: int, T: int):
    """The controller-tick test's raw inputs: T ticks of (state [B, 36], joystick [B, 5])."""
    from oracle import controller_ref as cr
    rng = np.random.default_rng(4000 + B)
    return [(cr.synthetic_states(rng, B, upright=t % 2 == 0), cr.synthetic_joy(rng, B)) for t in range(T)]
