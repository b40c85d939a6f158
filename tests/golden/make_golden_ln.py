"""Generate tests/golden/golden_ln.npz (run from the repo root:
`python tests/golden/make_golden_ln.py`).

Inputs and fp64 outputs of two LayerNormalization policies (synth.py: ln_pre_small,
ln_mixed) from the tests' own reference (tests/ln_ref.py: numpy fp64 on the .onnx
file's nodes). tests/test_cpu_layernorm.py checks the fixture against ln_ref, and
tests/test_gpu_layernorm.py checks the engine against the fixture.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ln_ref  # noqa: E402
from go2_onnx_controller_amd import synth  # noqa: E402

NAMES = ("ln_pre_small", "ln_mixed")
ROWS = 24  # one full 16-row tile and a partial one


def main():
    out = {}
    for i, name in enumerate(NAMES):
        ref = ln_ref.LnRef(synth.MODELS[name]())
        in_dim = ref.g.inputs[0][1][1]
        x = np.random.default_rng(700 + i).standard_normal((ROWS, in_dim)).astype(np.float32)
        out[f"{name}_x"] = x
        out[f"{name}_y"] = ref.f64(x)
    np.savez(os.path.join(HERE, "golden_ln.npz"), **out)
    print("golden_ln.npz written")


if __name__ == "__main__":
    main()
