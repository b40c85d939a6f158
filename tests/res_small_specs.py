"""Four more residual MLP policies, at the smallest shapes where the single launch and the
multi-workgroup resident kernel (GO2PI_RESIDUAL_SMALL) can go wrong with a carried value and the
GEMV chain cannot: there the carried value lives in the publishing lanes of the workgroup that
owns its tile, across the layers between source and consumer.

One policy_specs.Family in the res family's dialect. Its names are added to policy_specs' name
table at import, so the name-keyed helpers (model_path, probe_forward, expected_view, obs, ..)
serve them; they are not in policy_specs.FAMILIES, whose models tests/golden/policy_specs.json
pins.
"""
import dataclasses

import policy_specs as ps
from policy_specs import RUN, L

RES_SMALL = dataclasses.replace(
    ps.RES,
    specs={
        # a bottleneck block: workgroups 1-3 own no tile of the 16-wide middle layer and hold
        # layer 0's carried columns across it
        "res_neck": (48, None, [L(64, "Elu"), L(16, "Elu"), L(64, "Elu", res=0), L(12)]),
        # SimBa, 600 wide: K_pad 640 > 512, so batch 5 and 8 take the second sweep round in the
        # residual instantiations; 40 workgroups
        "simba_round2": (24, None, [L(600, ln="pre"), L(600, "Relu"), L(600, ln="pre", res=0), L(8)]),
    },
    probe_specs={
        "probe_neck": (30, None, [L(64, "Relu"), L(16, "Relu"), L(64, "Relu", res=0), L(6)]),
        # the consumer (layer 1) is padded to its skip successor's K_pad = 128, its source to 64:
        # workgroups 4-7 add a carried value that no layer wrote
        "probe_wide_consumer": (40, None, [L(60, "Relu"), L(60, "Relu", res=0), L(40, "Relu", [RUN, (0, 16)]), L(6)]),
    },
    weight_seed_base=9400,
    # (seeds at which no hidden unit is dead on every row of the B = 33 input and every carried
    # unit changes an output: tests/test_cpu_res_small.py; at 41, probe_neck's unit (2, 42) is dead)
    probe_seed={"probe_neck": 45, "probe_wide_consumer": 40},
    obs_seed_base=64000,
    small_batches=(1, 5, 8),
    probe_batches=(8, 1, 5, 7, 4, 8),  # stale rows of a larger request
)

for _n in RES_SMALL.names + RES_SMALL.probes:
    assert ps._FAMILY_OF.get(_n, RES_SMALL) is RES_SMALL, _n  # names are unique across the families
    ps._FAMILY_OF[_n] = RES_SMALL

# what the small-batch kernels run under GO2PI_RESIDUAL_SMALL: both residual families
NAMES = ps.RES.names + RES_SMALL.names      # float parity
PROBES = ps.RES.probes + RES_SMALL.probes   # exact
SW = "GO2PI_RESIDUAL_SMALL"


def has_ln(name):
    return any(ly["ln"] for ly in ps.spec(name)[2])


def has_skip(name):
    return any(ly["skip"] for ly in ps.expected_view(name))


def switches(name):
    """The environment switches that put the model on the small-batch kernels."""
    return (SW,) + (("GO2PI_SKIP_SMALL",) if has_skip(name) else ())


def opts(name):
    """... and the engine option (ln_small's GO2PI_LN_SMALL bit) an LN model needs beside them."""
    return {"ln_small": 1} if has_ln(name) else {}
