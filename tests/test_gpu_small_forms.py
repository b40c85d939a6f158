"""GPU: the three small-batch forms return the same bits on fractional weights.

gemv_layer_kernel (the chain, GO2PI_SMALL_CHAIN=1), policy_latency_kernel (the single launch)
and policy_resident_kernel with layer 0 tiled (GO2PI_RES_TILED0=1, and GO2PI_RES_MULTI=1 so
that no other resident form takes the shape) run one tiled layer body with one summation
order per output (stated in csrc/tile_layer.hpp; the chain calls it, the other two keep their
own text of it), so their answers are equal bit for bit, not only within the tolerance. The
probe suites pin that on integer policies, where any order gives the same sum; this pins it
where a different order would show.

Each form is also held to the fp64 reference at the project's 1e-5, so that three identical
wrong answers do not pass. Models: pre- and post-LN with non-uniform widths (ln_mixed under
ln_small), a skip layer of K_pad 640 whose rows at batch 5 and 8 take the second sweep round
with the skip columns behind it (ea_round2 under GO2PI_SKIP_SMALL), and the plain
instantiation's widest input (24 -> 600 -> 8). The switches are read when an engine is
created, so each is set first.
"""
import functools

import numpy as np
import pytest

import ln_ref
import ln_small_models as lm
import policy_specs as ps
from conftest import abs_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
RES_MS = 5000
BATCHES = (1, 5, 8)
CHAIN = "gemv_layer_kernel graph"
LATENCY = "policy_latency_kernel"
MULTI = "policy_resident_kernel"
# form -> (switches beside the model's own, resident_ms)
FORMS = {"chain": (("GO2PI_SMALL_CHAIN",), 0), "launch": ((), 0),
         "resident": (("GO2PI_RES_TILED0", "GO2PI_RES_MULTI"), RES_MS)}
# model -> (the switch that opts it into the small-batch kernels, Engine keywords)
MODELS = {"ln_mixed": (None, dict(ln_small=True)), "ea_round2": ("GO2PI_SKIP_SMALL", {}), "plain_600": (None, {})}


@functools.lru_cache(maxsize=None)
def _model(name):
    """The model as Engine and LnRef take it: a path, or the bytes."""
    from go2_onnx_controller_amd import synth
    if name == "ln_mixed":
        return synth.ensure_model(name)
    if name == "ea_round2":
        return ps.path(name)
    return synth.mlp_model_bytes(**lm.PLAIN_WIDE)


@functools.lru_cache(maxsize=None)
def _case(name, B):
    """(a fresh observation of this batch, its fp64 answer): computed once, never written."""
    if name == "ln_mixed":
        x = lm.obs(name, B, lm.bitwise_seed(name, B))
    elif name == "ea_round2":
        x = ps.obs(name, B, 2)
    else:
        x = lm.plain_wide_obs(B)
    y = ln_ref.LnRef(_model(name)).f64(x)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def _run(name, form, monkeypatch):
    from go2_onnx_controller_amd import Engine
    own, kw = MODELS[name]
    switches, res_ms = FORMS[form]
    for sw in ("GO2PI_SMALL_CHAIN", "GO2PI_RES_TILED0", "GO2PI_RES_MULTI", "GO2PI_SKIP_SMALL"):
        monkeypatch.delenv(sw, raising=False)
    for sw in switches + ((own,) if own else ()):
        monkeypatch.setenv(sw, "1")
    with Engine(_model(name), max_batch=8, resident_ms=res_ms, **kw) as e:
        assert e.small_kernel == (CHAIN if form == "chain" else LATENCY), (name, form, e.small_kernel)
        if form == "resident":
            assert e.resident_kernel.startswith(MULTI + " ring="), (name, e.resident_kernel)
        else:
            assert e.resident_kernel.startswith("none"), (name, form, e.resident_kernel)
        out = {B: e.run(_case(name, B)[0]) for B in BATCHES}
        assert e.resident_launches == (1 if form == "resident" else 0), (name, form, e.resident_launches)
    return out


@pytest.mark.parametrize("name", list(MODELS))
def test_three_forms_bitwise_equal(name, monkeypatch):
    got = {form: _run(name, form, monkeypatch) for form in FORMS}
    for B in BATCHES:
        want = _case(name, B)[1]
        for form in FORMS:
            y = got[form][B]
            err = abs_err(y, want)
            print(f"{name} {form} B={B}: abs err {err:.3g}")
            assert np.isfinite(y).all() and err <= TOL, (name, form, B, err)
        for form in ("launch", "resident"):
            diff = int(np.count_nonzero(got[form][B].view(np.uint32) != got["chain"][B].view(np.uint32)))
            print(f"{name} {form} vs chain B={B}: {diff} of {got[form][B].size} words differ")
            assert np.array_equal(got[form][B], got["chain"][B]), (name, form, B)
