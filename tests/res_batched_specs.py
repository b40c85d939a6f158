"""Residual MLP policies of the 4-wave pipeline's shape (GO2PI_RESIDUAL_BATCHED:
policy_mlp_res_kernel<tiles per wave, head tiles>), at the smallest shapes where that kernel can
go wrong and the general body cannot: there the carried value lives in each lane's registers
from the source layer's epilogue to the consumer's, through both epilogue sites (inside the
layer loop and in front of the head), the register hand-off (4 / 8 tiles per wave) and the
barrier path (2 tiles per wave), with each hidden layer's own activation.

One policy_specs.Family in the res family's dialect (and a second, EXTRA, of two models that
only the selection tests use). Their names are added to policy_specs' name
table at import, so the name-keyed helpers (model_path, probe_forward, expected_view, obs, ..)
serve them; they are not in policy_specs.FAMILIES, whose models tests/golden/policy_specs.json
pins.
"""
import dataclasses

import policy_specs as ps
from policy_specs import L

RES_BATCHED = dataclasses.replace(
    ps.RES,
    specs={
        # fewest layers; the consumer is the last hidden layer (the site in front of the head); barrier path
        "resb_t2_min": (20, None, [L(128, "Relu"), L(128, "Relu", res=0), L(6)]),
        # consumer and source at once, at the site inside the layer loop
        "resb_t2_adjacent": (48, None, [L(128, "Elu"), L(128, "Elu", res=0), L(128, "Elu", res=1), L(12)]),
        # a post-LN source, masked columns, two true widths under one pad, a 2-tile head
        "resb_t2_post_h2": (33, None, [L(100, "Relu", ln="post"), L(72, "Relu"), L(100, "Relu", ln="post", res=0),
                                       L(20)]),
        # chained raw-sum taps on the register hand-off, an activation per layer
        "resb_t4_simba2": (48, None, [L(250, ln="pre"), L(200, "Relu"), L(250, ln="pre", res=0), L(256, "Relu"),
                                      L(250, ln="pre", res=2), L(12)]),
        # carried across two layers, a layer behind the consumer, a 2-tile head
        "resb_t4_far": (40, None, [L(256, "Tanh"), L(256, "Tanh"), L(256, "Tanh"), L(256, "Tanh", res=0),
                                   L(256, "Tanh"), L(17)]),
        # the workload's width
        "resb_t8_simba": (48, None, [L(512, ln="pre"), L(512, "Relu"), L(512, ln="pre", res=0), L(12)]),
        # no LN at 8 tiles per wave, 500 of 512 columns
        "resb_t8_v1": (48, None, [L(500, "Elu"), L(500, "Elu"), L(500, "Elu", res=0), L(500, "Elu"), L(12)]),
    },
    # wider or deeper probes pass 2^24 (three 193-wide layers do), so exactness inside the layer
    # loop at 4 tiles per wave and up rests on the float models
    probe_specs={
        "probe_t2": (12, None, [L(70, "Relu"), L(70, "Relu"), L(70, "Relu", res=0), L(8)]),
        "probe_t2_adjacent": (16, None, [L(65, "Relu"), L(65, "Relu", res=0), L(65, "Relu", res=1), L(6)]),
        "probe_t4": (30, None, [L(200, "Relu"), L(200, "Relu", res=0), L(6)]),
        "probe_t8": (24, None, [L(450, "Relu"), L(450, "Relu", res=0), L(6)]),
    },
    weight_seed_base=9500,
    # (the first seeds at which the bound stays below 2^24, no hidden unit is dead on every row
    # of the B = 33 input, and every observation column and carried unit changes an output:
    # tests/test_cpu_res_batched.py)
    probe_seed={"probe_t2": 2, "probe_t2_adjacent": 2, "probe_t4": 1, "probe_t8": 1},
    obs_seed_base=66000, probe_obs_max=1, probe_w0_max=1,
    parity_batches=(1, 15, 16, 17, 33),   # small_batch = -1: every batch on the pipeline
    small_batches=(9, 100),               # the default small_batch: the first batch past the chain, and 7 tiles
    probe_batches=(33, 1, 16, 17, 8, 5),  # a smaller batch behind a larger one
)

# two more for the selection alone (a family of their own, so the table above keeps its
# positions and seeds): the pipeline's shape behind a "norm" front (Sub, Div, Clip), which the
# pipeline's kernels do not take, and with a Go2 controller's I/O (98 observations, 12 actions),
# whose tick stays refused
EXTRA = dataclasses.replace(
    RES_BATCHED,
    specs={"resb_front": (20, "norm", [L(128, "Relu"), L(128, "Relu", res=0), L(6)]),
           "resb_ctl": (98, None, [L(128, "Elu"), L(128, "Elu", res=0), L(12)])},
    probe_specs={}, probe_seed={}, weight_seed_base=9550, obs_seed_base=67000, norm_front=True)

for _f in (RES_BATCHED, EXTRA):
    for _n in _f.names + _f.probes:
        assert ps._FAMILY_OF.get(_n, _f) is _f, _n  # names are unique across the families
        ps._FAMILY_OF[_n] = _f

SW = "GO2PI_RESIDUAL_BATCHED"
GENERAL = "policy_fused_res_kernel<8>"
# <tiles per wave, head tiles> of every model the switch moves to the pipeline
TPW_HT = {"resb_t2_min": (2, 1), "resb_t2_adjacent": (2, 1), "resb_t2_post_h2": (2, 2), "resb_t4_simba2": (4, 1),
          "resb_t4_far": (4, 2), "resb_t8_simba": (8, 1), "resb_t8_v1": (8, 1),
          "simba_256": (4, 1), "res_v1": (2, 1),  # (policy_specs.RES)
          "resb_ctl": (2, 1),  # (EXTRA)
          "probe_t2": (2, 1), "probe_t2_adjacent": (2, 1), "probe_t4": (4, 1), "probe_t8": (8, 1)}
KERNEL = {n: "policy_mlp_res_kernel<%d, %d>" % t for n, t in TPW_HT.items()}
NAMES = RES_BATCHED.names + ("simba_256", "res_v1")  # float parity
PROBES = RES_BATCHED.probes                           # exact
# residual models the switch leaves on the general body: 64-wide hidden layers (one tile per
# wave), non-uniform widths, a skip input
INELIGIBLE = ("simba_64", "res_adjacent", "res_skip")


def inputs(name):
    """Every (B, k) whose ps.obs(name, B, k) a GPU test of these models feeds."""
    out = [(B, 0) for B in RES_BATCHED.parity_batches + RES_BATCHED.small_batches + (8,)]
    if name == "resb_t8_simba":
        out.append((4097, 0))
    if name in ("resb_t4_simba2", "resb_t2_post_h2"):
        out.append((1024, 0))
    if name == "resb_t4_far":
        out += [(100, k) for k in range(3)]
    return out
