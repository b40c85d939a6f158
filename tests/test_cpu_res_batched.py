"""CPU: residual MLP policies on the 4-wave pipeline (GO2PI_RESIDUAL_BATCHED:
policy_mlp_res_kernel<tiles per wave, head tiles>), through the planner
(tests/cpp/plan_probe.cpp), the loader and the oracle; no device is touched.

1. with the switch every model of tests/res_batched_specs.py plans the pipeline's residual
   kernel of its shape; without it policy_fused_res_kernel<8>, and every other plan key is the
   same either way;
2. residual models outside the pipeline's shape, a "norm" front and waves = 8 keep the general
   residual kernel; waves = 4 / 16 stay refused;
3. the switch beside GO2PI_RESIDUAL_SMALL, ln_small 0..3 and small_batch = -1;
4. a model without a residual plans what it planned, switch or not;
5. the probes: exactness bound, float32 / float64 oracle equal to the int64 answer, every
   column, hidden unit and carried unit matters;
6. the float models' input condition on exactly the inputs tests/test_gpu_res_batched.py feeds;
7. the loader's view of the new models.
"""
import numpy as np
import pytest

import ln_ref
import policy_specs as ps
import res_batched_specs as rb
from conftest import SHIPPED, abs_err
from test_cpu_plan import plan

SW = rb.SW
TOL = 1e-5
CHAIN = "gemv_layer_kernel graph"
LATENCY = "policy_latency_kernel"
# what the switch may change of a plan: the batched selection (small_kernel names the batched
# kernel only where there is no small-batch path)
SELECTION = ("batched_kernel",)


# ---- 1. the selection
@pytest.mark.parametrize("name", rb.NAMES + rb.PROBES + ("resb_ctl",))
def test_selection_with_and_without_the_switch(tmp_path, name):
    path = ps.model_path(name, tmp_path)
    got, off = plan(path, SW), plan(path)
    assert got["batched_kernel"] == rb.KERNEL[name], got["batched_kernel"]
    assert off["batched_kernel"].startswith(rb.GENERAL), off["batched_kernel"]
    assert got["small_kernel"] == off["small_kernel"] == CHAIN
    for k in got:
        if k not in SELECTION:
            assert got[k] == off[k], k
    # no small-batch path: every batch on the batched kernel
    got1, off1 = plan(path, SW, small_batch=-1), plan(path, small_batch=-1)
    assert got1["batched_kernel"] == got1["small_kernel"] == rb.KERNEL[name]
    assert off1["batched_kernel"].startswith(rb.GENERAL) and off1["small_kernel"] == off1["batched_kernel"]
    for k in got1:
        if k not in SELECTION + ("small_kernel",):
            assert got1[k] == off1[k], k
    # the switch needs no LN bit beside it, and any ln_small leaves the choice alone
    for bits in (0, 1, 2, 3):
        assert plan(path, SW, ln_small=bits)["batched_kernel"] == rb.KERNEL[name], bits
        assert plan(path, ln_small=bits)["batched_kernel"].startswith(rb.GENERAL), bits


# ---- 2. what keeps the general residual kernel
@pytest.mark.parametrize("name", rb.INELIGIBLE + ("resb_front",))
def test_ineligible_models_keep_the_general_kernel(tmp_path, name):
    path = ps.model_path(name, tmp_path)
    for opts in ({}, {"small_batch": -1}, {"ln_small": 3}):
        got = plan(path, SW, **opts)
        assert got["batched_kernel"].startswith(rb.GENERAL), (name, opts, got["batched_kernel"])
        assert got == plan(path, **opts), (name, opts)


@pytest.mark.parametrize("name", ["resb_t2_min", "resb_t4_simba2", "resb_t8_simba"])
def test_explicit_waves(tmp_path, name):
    path = ps.model_path(name, tmp_path)
    assert plan(path, SW, waves=8)["batched_kernel"].startswith(rb.GENERAL)
    assert plan(path, SW, waves=8) == plan(path, waves=8)
    for waves in (4, 16):  # still refused
        got = plan(path, SW, waves=waves)
        assert got["code"] == -1 and "residual connections" in got["error"]
    for sw2 in ("GO2PI_NO_W4", "GO2PI_NO_HEAD_FUSE"):  # the pipeline's A/B switches hold for it too
        assert plan(path, SW, sw2)["batched_kernel"].startswith(rb.GENERAL), sw2


# ---- 3. beside other switches
@pytest.mark.parametrize("name", ["resb_t2_min", "resb_t4_simba2", "simba_256", "res_v1"])
def test_beside_the_small_batch_switches(tmp_path, name):
    path = ps.model_path(name, tmp_path)
    ln = any(ly["ln"] for ly in ps.spec(name)[2])
    for bits in (0, 1, 2, 3):
        # GO2PI_RESIDUAL_SMALL: the single launch (an LN model with the GO2PI_LN_SMALL bit), else the chain
        want_small = LATENCY if (not ln or bits & 1) else CHAIN
        for res_ms in (0, 100):
            got = plan(path, SW, "GO2PI_RESIDUAL_SMALL", ln_small=bits, resident_ms=res_ms)
            off = plan(path, "GO2PI_RESIDUAL_SMALL", ln_small=bits, resident_ms=res_ms)
            assert got["batched_kernel"] == rb.KERNEL[name]
            assert got["small_kernel"] == want_small, (name, bits, got["small_kernel"])
            for k in got:
                if k not in SELECTION:
                    assert got[k] == off[k], (k, bits, res_ms)
        assert plan(path, SW, ln_small=bits)["small_kernel"] == CHAIN
        got = plan(path, SW, "GO2PI_RESIDUAL_SMALL", ln_small=bits, small_batch=-1)
        assert got["small_kernel"] == got["batched_kernel"] == rb.KERNEL[name]


# ---- 4. models without a residual
@pytest.mark.parametrize("name", ["shipped", "go2_mlp_512", "ln_512_pre", "go2_gru_256", "ea_98"])
def test_models_without_a_residual_plan_what_they_planned(synth_path, tmp_path, name):
    p = SHIPPED if name == "shipped" else ps.model_path(name, tmp_path) if name == "ea_98" else synth_path(name)
    for opts in ({}, {"ln_small": 3}, {"ln_small": 2}, {"small_batch": -1}, {"resident_ms": 100}):
        assert plan(p, SW, **opts) == plan(p, **opts), (name, opts)
    if name == "ln_512_pre":  # the LN pipeline's kernel stays the LN pipeline's
        assert plan(p, SW, ln_small=3)["batched_kernel"] == "policy_mlp_ln_kernel<8, 1>"


# ---- 5. the probes
@pytest.mark.parametrize("name", rb.PROBES)
def test_probe_is_exact_and_every_unit_matters(tmp_path, name):
    bound = ps.probe_bound(name)
    print(f"{name}: largest sum |w||h| + |b| + |carried| = {bound} (2^24 = {1 << 24})")
    assert bound < 1 << 24
    ref = ln_ref.LnRef(ps.model_path(name, tmp_path))
    for B in sorted(set(rb.RES_BATCHED.probe_batches)):
        x = ps.probe_obs(name, B)
        want = ps.probe_forward(name, x)
        for dt in (np.float64, np.float32):  # the oracle agrees with the int64 answer, exactly
            assert np.array_equal(ref._act(x, dt), want.astype(dt)), (B, dt)
        assert np.abs(want).max() <= bound
    x = ps.probe_obs(name, 33)
    want = ps.probe_forward(name, x)
    _, _, layers = ps.spec(name)
    assert ps.read_columns(name) == list(range(ps.in_dim(name)))
    for j in range(ps.in_dim(name)):
        assert not np.array_equal(ps.probe_forward(name, x, zero_unit=(-1, j)), want), ("obs", j)
    for l, ly in enumerate(layers[:-1]):
        for j in range(ly["n"]):
            assert not np.array_equal(ps.probe_forward(name, x, zero_unit=(l, j)), want), (l, j)
    for l, ly in enumerate(layers):
        if ly["res"] is not None:
            for j in range(ly["n"]):
                assert not np.array_equal(ps.probe_forward(name, x, zero_carried=(l, j)), want), ("carried", l, j)


# ---- 6. the float models' input condition
@pytest.mark.parametrize("name", rb.NAMES + ("resb_ctl",))
def test_input_condition_of_the_float_models(tmp_path, name):
    """On the inputs tests/test_gpu_res_batched.py uses, float32 arithmetic alone stays under a
    third of the tolerance."""
    ref = ln_ref.LnRef(ps.model_path(name, tmp_path))
    worst = 0.0
    for B, k in rb.inputs(name):
        x = ps.obs(name, B, k)
        worst = max(worst, abs_err(ref.f32(x), ref.f64(x)))
    print(f"{name}: worst fp32-vs-fp64 error {worst:.3g}")
    assert worst <= TOL / 3


# ---- 7. loader view
@pytest.mark.parametrize("name", rb.RES_BATCHED.names + rb.PROBES)
def test_loader_view(tmp_path, name):
    v = ps.inspect(ps.model_path(name, tmp_path))
    assert v["in_dim"] == ps.in_dim(name)
    got = [{k: ly[k] for k in ("K", "N", "act", "ln", "skip", "res")} for ly in v["layers"]]
    assert got == ps.expected_view(name)
