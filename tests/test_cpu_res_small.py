"""CPU: residual MLP policies on the small-batch kernels (GO2PI_RESIDUAL_SMALL), through the
planner (tests/cpp/plan_probe.cpp), the loader and the oracle; no device is touched.

1. with the switch (and the GO2PI_LN_SMALL bit / GO2PI_SKIP_SMALL where the model needs them)
   every residual model plans policy_latency_kernel and, with resident_ms > 0, the
   multi-workgroup resident kernel with a tiled layer 0 for act() alone; the batched kernel,
   every program scalar and every buffer hash are the plan's without the switch;
2. the prerequisite switches: without them, the chain;
3. the switch beside GO2PI_SMALL_CHAIN, small_batch = -1, both ring placements and the
   resident A/B switches;
4. a model without a residual plans what it planned, switch or not;
5. the LDS regions of the latency and multi-workgroup forms of residual programs;
6. the new probes: exactness bound, float32 / float64 oracle equal to the int64 answer, every
   column, hidden unit and carried unit matters;
7. the new float models' input condition;
8. the loader's view of the new models.
"""
import numpy as np
import pytest

import ln_ref
import policy_specs as ps
import res_small_specs as rs
from conftest import SHIPPED, abs_err
from test_cpu_lds_layout import check_regions
from test_cpu_plan import plan

SW = rs.SW
MULTI = "policy_resident_kernel"
LATENCY = "policy_latency_kernel"
CHAIN = "gemv_layer_kernel graph"
# what the switch may change of a plan: the small-batch selection and the layouts it brings in
SELECTION = ("small_kernel", "resident_kernel", "controller_kernel", "latency_ok", "done_ok", "lds")
LN_MODELS = [n for n in rs.NAMES if rs.has_ln(n)]


def _chain(got):
    return got["small_kernel"] == CHAIN and got["resident_kernel"] == "none" and got["latency_ok"] == 0


# ---- 1. with the switch
@pytest.mark.parametrize("name", rs.NAMES + rs.PROBES)
def test_selection_with_the_switch(tmp_path, name):
    path = ps.model_path(name, tmp_path)
    others = [s for s in rs.switches(name) if s != SW]
    got = plan(path, *rs.switches(name), resident_ms=100, **rs.opts(name))
    off = plan(path, *others, resident_ms=100, **rs.opts(name))
    assert got["small_kernel"] == LATENCY
    assert got["latency_ok"] == 1 and got["done_ok"] == 1
    assert got["resident_kernel"].startswith(MULTI + " ring="), got["resident_kernel"]
    assert got["controller_kernel"].startswith("none")
    assert got["lds"]["act"]["form"] == "multi" and got["lds"]["act"]["nf"] == 0 and "ctl" not in got["lds"]
    # without the switch: the chain, as tests/test_cpu_res.py pins it
    assert _chain(off) and off["done_ok"] == 0, off["small_kernel"]
    # the batched kernel, the program's scalars and every buffer are untouched by the switch
    assert got["batched_kernel"].startswith("policy_fused_res_kernel<8>")
    for k in got:
        if k not in SELECTION:
            assert got[k] == off[k], k
    assert got["lds"]["gemv"] == off["lds"]["gemv"] and got["lds"]["lds_stride"] == off["lds"]["lds_stride"]
    # no resident path asked for: the single launch alone
    got0 = plan(path, *rs.switches(name), **rs.opts(name))
    assert got0["small_kernel"] == LATENCY and got0["resident_kernel"] == "none"


def test_local_layer0_geometry_is_tiled(tmp_path):
    """simba_256's layer 0 (K_pad 64, N_pad 256: two slices of two chunks, NF = 8) would run as
    the local layer 0; a residual program tiles it, so that a publishing lane owns the
    source's columns. The same layer shapes without the Add keep the local form."""
    from go2_onnx_controller_amd import synth
    lds = plan(ps.model_path("simba_256", tmp_path), SW, resident_ms=100, ln_small=1)["lds"]
    assert (lds["k0_pad"], lds["n0_pad"], lds["act"]["nf"], lds["act"]["tiled0"]) == (64, 256, 0, 0)
    p = tmp_path / "plain_256.onnx"
    p.write_bytes(synth.mlp_model_bytes(dims=(48, 256, 256, 256, 12), seed=3, act="Relu", layer_norm="pre"))
    lds = plan(p, SW, "GO2PI_RES_MULTI", resident_ms=100, ln_small=1)["lds"]
    assert (lds["k0_pad"], lds["n0_pad"], lds["act"]["nf"]) == (64, 256, 8)
    r2 = plan(ps.model_path("simba_round2", tmp_path), SW, resident_ms=100, ln_small=1)
    assert r2["one_round"] == 0 and max(g["k_pad"] for g in r2["lds"]["gemv"][1:]) == 640


# ---- 2. the prerequisite switches
@pytest.mark.parametrize("name", LN_MODELS)
def test_ln_residual_needs_the_ln_small_bit_too(tmp_path, name):
    path = ps.model_path(name, tmp_path)
    for extra in ({}, {"ln_small": 0}, {"ln_small": 2}):
        assert _chain(plan(path, SW, resident_ms=100, **extra)), (name, extra)
    for bits in (1, 3):
        got = plan(path, SW, resident_ms=100, ln_small=bits)
        assert got["small_kernel"] == LATENCY and got["resident_kernel"].startswith(MULTI)


@pytest.mark.parametrize("name", ["res_skip", "probe_wide_consumer"])
def test_skip_residual_needs_skip_small_too(tmp_path, name):
    path = ps.model_path(name, tmp_path)
    assert _chain(plan(path, SW, resident_ms=100))
    assert _chain(plan(path, "GO2PI_SKIP_SMALL", resident_ms=100))
    got = plan(path, SW, "GO2PI_SKIP_SMALL", resident_ms=100)
    assert got["small_kernel"] == LATENCY and got["resident_kernel"].startswith(MULTI)


# ---- 3. the switch beside other settings
@pytest.mark.parametrize("name", ["simba_64", "res_v1", "res_skip", "probe_neck"])
def test_switch_with_other_settings(tmp_path, name):
    path = ps.model_path(name, tmp_path)
    sws, kw = rs.switches(name), rs.opts(name)
    others = [s for s in sws if s != SW]
    assert _chain(plan(path, *sws, "GO2PI_SMALL_CHAIN", resident_ms=100, **kw))
    assert plan(path, *sws, small_batch=-1, resident_ms=100, **kw) == plan(path, *others, small_batch=-1,
                                                                           resident_ms=100, **kw)
    assert plan(path, *sws, small_batch=-1, **kw)["small_kernel"].startswith("policy_fused_res_kernel<8>")
    for ring in ("vram", "host"):
        got = plan(path, *sws, "ring=" + ring, resident_ms=100, **kw)
        assert got["resident_kernel"] == f"{MULTI} ring={ring}"
    for sw2 in ("GO2PI_RES_MULTI", "GO2PI_RES_R1W", "GO2PI_REQ_HOST"):
        assert plan(path, *sws, sw2, resident_ms=100, **kw)["resident_kernel"].startswith(MULTI + " ring=")
    for waves in (4, 16):  # still refused
        got = plan(path, *sws, waves=waves, **kw)
        assert got["code"] == -1 and "residual connections" in got["error"]


# ---- 4. models without a residual
@pytest.mark.parametrize("name", ["shipped", "go2_mlp_512", "go2_gru_256", "go2_lstm_256", "mlp_small_relu", "ctl_h3",
                                  "wide_256_3", "ln_512_pre", "ln_wide_pre", "ln_ctl_post"])
def test_models_without_a_residual_plan_what_they_planned(synth_path, name):
    p = SHIPPED if name == "shipped" else synth_path(name)
    for opts in ({}, {"resident_ms": 100}, {"resident_ms": 100, "ln_small": 1}, {"small_batch": -1}):
        for ring in ("ring=vram", "ring=host"):
            assert plan(p, SW, ring, **opts) == plan(p, ring, **opts), (name, opts, ring)


@pytest.mark.parametrize("name", ["ea_98", "ea_ln"])
def test_skip_models_plan_what_they_planned(tmp_path, name):
    p = ps.model_path(name, tmp_path)
    for opts in ({}, {"resident_ms": 100}, {"resident_ms": 100, "ln_small": 1}, {"small_batch": -1}):
        for ring in ("ring=vram", "ring=host"):
            assert plan(p, SW, "GO2PI_SKIP_SMALL", ring, **opts) == plan(p, "GO2PI_SKIP_SMALL", ring, **opts), \
                (name, opts, ring)


# ---- 5. LDS regions
@pytest.mark.parametrize("name", rs.NAMES + rs.PROBES)
def test_lds_regions(tmp_path, name):
    lds = plan(ps.model_path(name, tmp_path), *rs.switches(name), resident_ms=100, **rs.opts(name))["lds"]
    kmax = max((ly["K"] + 63) // 64 * 64 for ly in ps.expected_view(name))
    for key in ("latency", "act"):
        f = lds[key]
        assert f["total_bytes"] % 4 == 0 and f["total_bytes"] <= 160 * 1024
        check_regions(f["regions"], f["total_bytes"] // 4)
        size = {n: s for n, _, s in f["regions"]}
        assert size["xs"] >= 8 * kmax  # eight rows of the widest layer input
        if key == "act":
            assert size["obsv"] >= 8 * ps.in_dim(name)


# ---- 6. the probes
@pytest.mark.parametrize("name", rs.RES_SMALL.probes)
def test_probe_is_exact_and_every_unit_matters(tmp_path, name):
    bound = ps.probe_bound(name)
    print(f"{name}: largest sum |w||h| + |b| + |carried| = {bound} (2^24 = {1 << 24})")
    assert bound < 1 << 24
    ref = ln_ref.LnRef(ps.model_path(name, tmp_path))
    for B in (33,) + tuple(sorted(set(rs.RES_SMALL.probe_batches))):
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


# ---- 7. the float models' input condition
@pytest.mark.parametrize("name", rs.RES_SMALL.names)
def test_input_condition_of_the_new_float_models(tmp_path, name):
    """On the inputs tests/test_gpu_res_small.py uses, float32 arithmetic alone stays under a
    third of the tolerance."""
    ref = ln_ref.LnRef(ps.model_path(name, tmp_path))
    worst = 0.0
    for B in rs.RES_SMALL.small_batches:
        for k in (0, 1, 2):
            x = ps.obs(name, B, k)
            worst = max(worst, abs_err(ref.f32(x), ref.f64(x)))
    print(f"{name}: worst fp32-vs-fp64 error {worst:.3g}")
    assert worst <= 1e-5 / 3


# ---- 8. loader view
@pytest.mark.parametrize("name", rs.RES_SMALL.names + rs.RES_SMALL.probes)
def test_loader_view(tmp_path, name):
    v = ps.inspect(ps.model_path(name, tmp_path))
    assert v["in_dim"] == ps.in_dim(name)
    got = [{k: ly[k] for k in ("K", "N", "act", "ln", "skip", "res")} for ly in v["layers"]]
    assert got == ps.expected_view(name)
