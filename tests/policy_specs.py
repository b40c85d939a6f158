"""Test policies with observation skip inputs and residual connections, described once.

Every model is a list of layers. A layer's input is a list of parts (RUN: the previous layer's
output; (b, e): columns [b, e) of x0, the observation as layer 0 sees it; RUN at layer 0 is the
whole x0, as (0, F) is), and it may add a carried value (res: the index of the source layer,
whose carried value is added to this layer's Gemm + bias output, in front of its
LayerNormalization and activation). The carried value of layer j is the input of its
LayerNormalization where it has one (the sum s_j of a pre-LN layer, act(s_j) of a post-LN one),
else its output.

Four things are derived from that description: the ONNX bytes (onnx_writer: Slice / Concat /
Gemm / Add nodes), the view the loader must report (K, N, act, ln, the skip columns in device
order: running value first, then the parts in Concat order, and res), the weights in device
column order and, for the integer probes, an int64 evaluation that owes nothing to the loader
or to the oracle.

The models come in three families (Family below), one per feature that brought them. A family
holds its tables, its seeds, the batches its tests run and the dialect its ONNX is written in;
model names are unique across the families, so every function takes a name alone.
tests/golden/policy_specs.json pins the bytes, weights and inputs of every model.

Weights are uniform in +-1 / sqrt(K) from a seeded generator, observations N(0, 1) from a
seeded generator. None of these models is in synth.MODELS (the golden hashes stay as they are).
"""
from __future__ import annotations

import dataclasses
import functools
import os

import numpy as np

from go2_onnx_controller_amd import onnx_writer as ow

ACT_CODE = {None: 0, "Elu": 1, "Relu": 2, "Tanh": 3, "Sigmoid": 4}
LN_CODE = {None: 0, "pre": 1, "post": 2}
RUN = "run"


def L(n, act=None, inp=(RUN,), ln=None, res=None):
    """One dense layer: n outputs, activation, input parts (RUN / (b, e) observation columns),
    LayerNormalization ("pre" / "post"), res: the source layer of the carried value it adds."""
    return dict(n=n, act=act, inp=tuple(inp), ln=ln, res=res)


@dataclasses.dataclass(frozen=True)
class Family:
    """specs, probe_specs: name -> (observation width, front, layers); front "norm": Sub, Div,
    Clip(+-5) on the observation, None: nothing."""
    specs: dict
    probe_specs: dict
    weight_seed_base: int      # a float model's weights: base + its index among names (+ 50: its front's constants)
    probe_seed: dict           # probe -> the seed of its integer weights
    obs_seed_base: int         # seed_of = base + 1000 * (index among names + probes) + 50 * k + B
    probe_obs_max: int         # probe observations are integers in [-max, max]
    probe_w0_max: int          # a probe's layer-0 weights are in [-max, max] (later layers: +-1)
    parity_batches: tuple = ()
    small_batches: tuple = ()
    probe_batches: tuple = ()
    # the dialect model_bytes writes
    attr_slice_every_third: bool = False   # every third Slice in the opset 1-9 attribute form
    alternate_concat_axis: bool = False    # Concat axis 1 on odd layers, -1 on even (else 1)
    norm_front: bool = False               # a spec may ask for the "norm" front
    identity_on_carried: bool = False      # layers 2, 6, ..: the carried operand through an Identity
    alternate_add_order: bool = False      # Add(y, carried) on odd layers, Add(carried, y) on even

    @property
    def names(self):
        return tuple(self.specs)

    @property
    def probes(self):
        return tuple(self.probe_specs)


# estimator-actor policies: an encoder MLP reads the observation, and a later dense layer reads
# Concat(encoder output, parts of the observation)
SKIP = Family(
    specs={
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
    },
    # one shaped like ea_k64's Concat (observation first), one with a layer-0 gather, two skip
    # layers and a skip on the head
    probe_specs={
        "probe_k64": (60, None, [L(32, "Relu", [(0, 60)]), L(19, "Relu"), L(64, "Relu", [(0, 45), RUN]), L(8)]),
        "probe_gather": (60, None, [L(24, "Relu", [(20, 50)]), L(32, "Relu", [(0, 20), RUN, (50, 60)]),
                                    L(6, None, [RUN, (5, 9)])]),
    },
    weight_seed_base=9100,
    # (seeds at which no hidden unit is dead on every row of the B = 33 input: tests/test_cpu_skip.py)
    probe_seed={"probe_k64": 80, "probe_gather": 77},
    obs_seed_base=52000, probe_obs_max=3, probe_w0_max=2,
    parity_batches=(1, 5, 8, 9, 16, 17, 33),
    attr_slice_every_third=True, alternate_concat_axis=True, norm_front=True,
)

# three more estimator-actor policies, at the smallest shapes where the single launch and the
# multi-workgroup resident kernel (GO2PI_SKIP_SMALL) can go wrong with a skip input and the GEMV
# chain cannot
SKIP_SMALL = Family(
    specs={
        # the skip layer's K = 598 -> K_pad 640 > 512: at batch 5 and up its rows pass the 4096
        # granules of one sweep round, and the skip columns sit past them
        "ea_round2": (98, None, [L(64, "Elu", [(0, 98)]), L(500, "Elu"), L(64, "Elu", [RUN, (0, 98)]), L(12)]),
    },
    probe_specs={
        # layer 0: K_pad 128 (8 chunks), N_pad = ceil64(max(100, 120)) = 128 -> 4 slices of 2
        # chunks: the resident kernel's local layer 0 (NF = 8), a skip on the layer behind it
        "probe_local0": (98, None, [L(100, "Relu", [(0, 98)]), L(64, "Relu", [RUN, (10, 30)]), L(8)]),
        # a layer-0 gather of the same geometry (K_pad 128, N_pad 128): must run tiled; parts in
        # front of and behind the running value; a skip on the head
        "probe_gather0": (100, None, [L(120, "Relu", [(2, 98)]), L(32, "Relu", [(98, 100), RUN, (0, 2)]),
                                      L(6, None, [RUN, (5, 9)])]),
    },
    weight_seed_base=9300,
    # (seeds at which no hidden unit is dead on every row of the B = 33 input and every column
    # read changes an output: tests/test_cpu_skip_small.py)
    probe_seed={"probe_local0": 1, "probe_gather0": 1},
    obs_seed_base=62000, probe_obs_max=3, probe_w0_max=2,
    small_batches=(1, 5, 8),
    probe_batches=(8, 1, 5, 7, 4, 8),  # tests/test_gpu_probe_shapes.py's order: stale rows of a larger request
)

# residual MLP policies (x + f(x)): SimBa blocks, whose carried value is the un-normalised sum
# in front of a LayerNormalization, and ResNet-v1 blocks, whose carried value is an activated
# layer output
RES = Family(
    specs={
        # SimBa: h = Linear(obs); h = h + Linear(Relu(Linear(LN(h)))) twice; out = Linear(LN(h)).
        # Chained taps of raw sums; 64 wide: four tiles on eight waves (the split-K store)
        "simba_64": (48, None, [L(64, ln="pre"), L(128, "Relu"), L(64, ln="pre", res=0), L(128, "Relu"),
                                L(64, ln="pre", res=2), L(12)]),
        # sixteen tiles on eight waves (two per wave)
        "simba_256": (48, None, [L(256, ln="pre"), L(256, "Relu"), L(256, ln="pre", res=0), L(12)]),
        # ResNet v1: the tap is an activated output, the width no multiple of 16, and the layer in
        # front of the 5-wide head carries the sum
        "res_v1": (33, None, [L(100, "Tanh"), L(100, "Tanh"), L(100, "Tanh", res=0), L(5)]),
        # one-layer blocks: each layer both consumer and source
        "res_adjacent": (48, None, [L(64, "Elu"), L(64, "Elu", res=0), L(64, "Elu", res=1), L(12)]),
        # the padded columns [20, 64) accumulate Sigmoid(0) = 0.5 per layer
        "res_sig": (48, None, [L(20, "Sigmoid"), L(20, "Sigmoid", res=0), L(20, "Sigmoid", res=1), L(12)]),
        # an estimator-actor with a residual block: the consumer (layer 4) is padded to its skip
        # successor's K_pad = 128, its source (layer 2) to 64
        "res_skip": (98, None, [L(64, "Elu", [(0, 98)]), L(19), L(64, "Elu", [RUN, (0, 49)]), L(64, "Elu"),
                                L(64, "Elu", res=2), L(64, "Elu", [RUN, (49, 98)]), L(12)]),
        # post-LN: the carried value is the activated value in front of the LN
        "res_post": (48, None, [L(64, "Relu", ln="post"), L(64, "Relu"), L(64, "Relu", ln="post", res=0), L(12)]),
    },
    probe_specs={
        "probe_v1": (40, None, [L(48, "Relu"), L(48, "Relu"), L(48, "Relu", res=0), L(8)]),
        "probe_adjacent": (30, None, [L(32, "Relu"), L(32, "Relu", res=0), L(32, "Relu", res=1), L(6)]),
    },
    weight_seed_base=9300,
    probe_seed={"probe_v1": 31, "probe_adjacent": 32},
    obs_seed_base=63000, probe_obs_max=2, probe_w0_max=1,
    parity_batches=(1, 5, 8, 9, 16, 17, 33),
    alternate_concat_axis=True, identity_on_carried=True, alternate_add_order=True,
)

FAMILIES = {"skip": SKIP, "skip_small": SKIP_SMALL, "res": RES}
_FAMILY_OF = {n: f for f in FAMILIES.values() for n in f.names + f.probes}
assert len(_FAMILY_OF) == sum(len(f.names + f.probes) for f in FAMILIES.values())  # names are unique

# what the small-batch kernels run under GO2PI_SKIP_SMALL: both skip families
SMALL_NAMES = SKIP.names + SKIP_SMALL.names      # float parity
SMALL_PROBES = SKIP.probes + SKIP_SMALL.probes   # exact


def family(name: str) -> Family:
    return _FAMILY_OF[name]


def is_probe(name: str) -> bool:
    return name in family(name).probe_specs


def spec(name: str):
    """(observation width, front, layers)"""
    fam = family(name)
    return fam.probe_specs[name] if is_probe(name) else fam.specs[name]


def weight_seed(name: str) -> int:
    fam = family(name)
    return fam.probe_seed[name] if is_probe(name) else fam.weight_seed_base + fam.names.index(name)


def in_dim(name: str) -> int:
    return spec(name)[0]


def parts(name: str, l: int):
    """Layer l's input parts, layer 0's RUN spelled (0, F)."""
    F, _, layers = spec(name)
    return tuple((0, F) if l == 0 and p == RUN else p for p in layers[l]["inp"])


def _widths(name, l):
    layers = spec(name)[2]
    return [layers[l - 1]["n"] if p == RUN else p[1] - p[0] for p in parts(name, l)]


def layer_k(name: str, l: int) -> int:
    return sum(_widths(name, l))


def weights(name: str):
    """[(W [N, K] in ONNX (Concat) column order, b [N], LN scale, LN bias)] per layer."""
    fam, layers = family(name), spec(name)[2]
    probe = is_probe(name)
    rng = np.random.default_rng(weight_seed(name))
    out = []
    for l, ly in enumerate(layers):
        K, N = layer_k(name, l), ly["n"]
        if probe:
            m = fam.probe_w0_max if l == 0 else 1  # (keeps the sums below 2^24)
            W = rng.integers(-m, m + 1, (N, K))
            W[W == 0] = 1  # every input column is read by every unit
            b = rng.integers(-4, 5, N)
            out.append((W.astype(np.float32), b.astype(np.float32), None, None))
            continue
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
    assert family(name).norm_front, name
    rng = np.random.default_rng(weight_seed(name) + 50)
    return (rng.uniform(-0.5, 0.5, F).astype(np.float32), rng.uniform(0.5, 2.0, F).astype(np.float32), 5.0)


def model_bytes(name: str) -> bytes:
    fam = family(name)
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
    cur, n_slice = None, 0
    tap = {}  # layer -> the tensor that holds its carried value
    for l, (ly, (W, b, g, c)) in enumerate(zip(layers, weights(name))):
        names = []
        for p in parts(name, l):
            if p == RUN:
                names.append(cur)
            elif p == (0, F):
                names.append(x0)
            else:
                out = f"part{n_slice}"
                if fam.attr_slice_every_third and n_slice % 3 == 2:
                    nodes.append(ow.node("Slice", [x0], [out], f"slice{n_slice}",
                                         [ow.attr_ints("starts", [p[0]]), ow.attr_ints("ends", [p[1]]),
                                          ow.attr_ints("axes", [1])]))
                else:
                    inits += [(f"st{n_slice}", np.array([p[0]], np.int64)), (f"en{n_slice}", np.array([p[1]], np.int64))]
                    nodes.append(ow.node("Slice", [x0, f"st{n_slice}", f"en{n_slice}", "ax1"], [out], f"slice{n_slice}"))
                n_slice += 1
                names.append(out)
        x = names[0]
        if len(names) > 1:
            x = f"cat{l}"
            axis = -1 if fam.alternate_concat_axis and l % 2 == 0 else 1
            nodes.append(ow.node("Concat", names, [x], x, [ow.attr_int("axis", axis)]))
        last = l == len(layers) - 1
        inits += [(f"w{l}", W), (f"b{l}", b)]
        y = "action" if last and not ly["act"] else f"g{l}"
        nodes.append(ow.node("Gemm", [x, f"w{l}", f"b{l}"], [y], f"gemm{l}", [ow.attr_int("transB", 1)]))
        if ly["res"] is not None:
            src = tap[ly["res"]]
            if fam.identity_on_carried and l % 4 == 2:
                nodes.append(ow.node("Identity", [src], [f"carry{l}"], f"carry{l}"))
                src = f"carry{l}"
            swap = fam.alternate_add_order and l % 2 == 0
            nodes.append(ow.node("Add", [src, y] if swap else [y, src], [f"s{l}"], f"res{l}"))
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


def expected_view(name: str):
    """What inspect_model must report per layer: K, N, act, ln, skip (device order), res (-1: none)."""
    F, _, layers = spec(name)
    out = []
    for l, ly in enumerate(layers):
        # (layer 0 reading every column is no skip: it is the plain input)
        skip = [c for p in parts(name, l) if p != RUN and not (l == 0 and p == (0, F)) for c in range(p[0], p[1])]
        out.append(dict(K=layer_k(name, l), N=ly["n"], act=ACT_CODE[ly["act"]], ln=LN_CODE[ly["ln"]], skip=skip,
                        res=-1 if ly["res"] is None else ly["res"]))
    return out


def device_weights(name: str):
    """Each layer's W with its columns in device order (running value first, then the parts in
    Concat order): what the loader's w_sum is taken of, and what the kernels multiply."""
    out = []
    for l, (W, _, _, _) in enumerate(weights(name)):
        at, run_cols, part_cols = 0, [], []
        for p, w in zip(parts(name, l), _widths(name, l)):
            (run_cols if p == RUN else part_cols).extend(range(at, at + w))
            at += w
        out.append(W[:, run_cols + part_cols])
    return out


def read_columns(name: str):
    """The observation columns any layer of the model reads."""
    layers = spec(name)[2]
    return sorted({c for l in range(len(layers)) for p in parts(name, l) if p != RUN for c in range(p[0], p[1])})


def seed_of(name: str, B: int, k: int = 0) -> int:
    fam = family(name)
    return fam.obs_seed_base + 1000 * (fam.names + fam.probes).index(name) + 50 * k + B


def obs(name: str, B: int, k: int = 0) -> np.ndarray:
    """N(0, 1) observations [B, in_dim] float32, a fixed function of (model, B, k); a "norm"
    front's model gets 3 N(0, 1) so that its Clip binds on some elements."""
    rng = np.random.default_rng(seed_of(name, B, k))
    x = rng.standard_normal((B, in_dim(name)))
    if spec(name)[1] == "norm":
        x = x * 3.0
    return x.astype(np.float32)


# ---------------------------------------------------------------------------
# integer probes: integer weights, biases and observations, Relu: every partial sum, the
# carried value included, is an integer below 2^24, so float32 arithmetic is exact in any
# summation order and a kernel must return the int64 answer bit for bit.
def probe_obs(name: str, B: int) -> np.ndarray:
    m = family(name).probe_obs_max
    rng = np.random.default_rng(seed_of(name, B))
    return rng.integers(-m, m + 1, (B, in_dim(name))).astype(np.float32)


def probe_forward(name: str, x, zero_unit=None, zero_carried=None) -> np.ndarray:
    """The probe's answer in int64. zero_unit = (l, j): unit j of layer l's output (l = -1:
    observation column j) is replaced by 0, for every reader. zero_carried = (l, j): unit j of
    the carried value that layer l adds is replaced by 0 on its way to the Add (the main chain
    keeps the unit)."""
    assert is_probe(name)
    x0 = np.asarray(x).astype(np.int64)
    if zero_unit and zero_unit[0] == -1:
        x0 = x0.copy()
        x0[:, zero_unit[1]] = 0
    outs = []
    for l, (ly, (W, b, _, _)) in enumerate(zip(spec(name)[2], weights(name))):
        assert ly["ln"] is None and ly["act"] in (None, "Relu")
        xin = np.concatenate([outs[-1] if p == RUN else x0[:, p[0]:p[1]] for p in parts(name, l)], axis=1)
        y = xin @ W.astype(np.int64).T + b.astype(np.int64)
        if ly["res"] is not None:
            c = outs[ly["res"]]
            if zero_carried and zero_carried[0] == l:
                c = c.copy()
                c[:, zero_carried[1]] = 0
            y = y + c
        if ly["act"] == "Relu":
            y = np.maximum(y, 0)
        if zero_unit and zero_unit[0] == l:
            y[:, zero_unit[1]] = 0
        outs.append(y)
    return outs[-1]


def probe_bound(name: str) -> int:
    """The largest sum |w| |h| + |b| + |carried| any unit of the probe can reach, from
    |obs| <= probe_obs_max: an upper bound of every partial sum in any order."""
    assert is_probe(name)
    obs_max = family(name).probe_obs_max
    outs = []
    for l, (ly, (W, b, _, _)) in enumerate(zip(spec(name)[2], weights(name))):
        h = np.concatenate([outs[-1] if p == RUN else np.full(w, obs_max, np.int64)
                            for p, w in zip(parts(name, l), _widths(name, l))])
        cur = np.abs(W.astype(np.int64)) @ h + np.abs(b.astype(np.int64))
        if ly["res"] is not None:
            cur = cur + outs[ly["res"]]
        outs.append(cur)
    return max(int(o.max()) for o in outs)


# ---------------------------------------------------------------------------
# what the test files share: the models on disk, the oracle and its answers, computed once
def model_path(name: str, directory) -> str:
    path = os.path.join(str(directory), name + ".onnx")
    if not os.path.exists(path):
        with open(path, "wb") as fh:
            fh.write(model_bytes(name))
    return path


@functools.lru_cache(maxsize=None)
def model_dir() -> str:
    """One directory for the session."""
    import tempfile
    return tempfile.mkdtemp(prefix="policy_specs_")


def path(name: str) -> str:
    return model_path(name, model_dir())


@functools.lru_cache(maxsize=None)
def ref(name: str):
    import ln_ref
    return ln_ref.LnRef(path(name))


@functools.lru_cache(maxsize=None)
def want(name: str, B: int, k: int = 0) -> np.ndarray:
    """The fp64 answer on obs(name, B, k), read-only."""
    y = ref(name).f64(obs(name, B, k))
    y.setflags(write=False)
    return y


def inspect(path):
    from go2_onnx_controller_amd.engine import inspect_model
    return inspect_model(str(path))
