"""Generate tests/golden/policy_specs.json (run from the repo root:
`python tests/golden/make_policy_specs.py`).

One record per test policy with skip inputs or residual connections: digests of everything
the tests derive from its description: the ONNX bytes, the weights, the loader's expected
view, the observations and, for the integer probes, the int64 answers and the exactness
bound. tests/test_cpu_policy_specs.py recomputes each record and compares.

The committed file was written by this script on the three per-feature modules
(tests/skip_models.py, tests/skip_small_models.py, tests/res_models.py) before one builder
replaced them, so it pins that no model, weight or input moved. A record that moves on purpose
is regenerated here; one that moves by accident is a bug in the builder.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import policy_specs as ps  # noqa: E402

OUT = os.path.join(HERE, "policy_specs.json")
BATCHES = range(1, 34)
# the view's keys as each family's tests compared them when the file was written
VIEW_KEYS = ("K", "N", "act", "ln", "skip")
# where the probes are zeroed on the B = 33 input. The skip probes: a unit (l, j) of a layer's
# output (l = -1: an observation column). The residual probes: unit j of the carried value on
# its way to an Add, the three units dealt in turn to the probe's residual layers.
ZERO_UNIT = ((-1, 3), (0, 5), (1, 2))
ZERO_CARRIED = (0, 7, 31)


def names():
    """[(family, name, is a probe)] in the families' own order."""
    return [(f, n, ps.is_probe(n)) for f, fam in ps.FAMILIES.items() for n in fam.names + fam.probes]


def _sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def record(family, name, probe):
    keys = VIEW_KEYS + (("res",) if family == "res" else ())
    r = {"family": family,
         "model": hashlib.sha256(ps.model_bytes(name)).hexdigest(),
         "weights": _sha(a for layer in ps.weights(name) for a in layer if a is not None),
         "view": [{k: ly[k] for k in keys} for ly in ps.expected_view(name)],
         "obs": _sha(ps.obs(name, B, k) for B in BATCHES for k in range(3))}
    if family != "res":
        r["device_weights"] = _sha(ps.device_weights(name))
    if probe:
        xs = [ps.probe_obs(name, B) for B in BATCHES]
        r["probe_obs"] = _sha(xs)
        r["probe_forward"] = _sha(ps.probe_forward(name, x) for x in xs)
        if family == "res":
            at = [l for l, ly in enumerate(ps.spec(name)[2]) if ly["res"] is not None]
            r["probe_zero_carried"] = _sha(ps.probe_forward(name, xs[-1], zero_carried=(at[i % len(at)], j))
                                           for i, j in enumerate(ZERO_CARRIED))
        else:
            r["probe_zero_unit"] = _sha(ps.probe_forward(name, xs[-1], zero_unit=z) for z in ZERO_UNIT)
        r["probe_bound"] = int(ps.probe_bound(name))
    return r


def records():
    return {name: record(family, name, probe) for family, name, probe in names()}


def main():
    with open(OUT, "w") as fh:  # one line per model
        fh.write("{\n" + ",\n".join(f' "{n}": {json.dumps(r, sort_keys=True)}' for n, r in records().items()) + "\n}\n")
    print(f"{OUT}: {len(names())} models")


if __name__ == "__main__":
    main()
