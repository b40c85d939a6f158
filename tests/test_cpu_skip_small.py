"""CPU: policies with observation skip inputs on the small-batch kernels (GO2PI_SKIP_SMALL),
through the planner (tests/cpp/plan_probe.cpp), the loader and the oracle; no device is touched.

1. with the switch every skip model plans policy_latency_kernel and, with resident_ms > 0,
   the multi-workgroup resident kernel for act() alone; the batched kernel, every program
   scalar and every buffer hash are the plan's without the switch;
2. the switch beside GO2PI_SMALL_CHAIN, small_batch = -1 and both ring placements;
3. a model without a skip input plans what it planned, switch or not;
4. the LDS regions of the latency and multi-workgroup forms of skip programs;
5. the new probes: exactness bound, float32 / float64 oracle equal to the int64 answer,
   every column read and every hidden unit matters; ea_round2's input condition;
6. the loader's view of the new models.
"""
import numpy as np
import pytest

import ln_ref
import ln_small_models as lm
import policy_specs as ps
from conftest import SHIPPED, abs_err
from test_cpu_lds_layout import check_regions
from test_cpu_plan import plan

SW = "GO2PI_SKIP_SMALL"
MULTI = "policy_resident_kernel"
CHAIN = "gemv_layer_kernel graph"
# what the switch may change of a plan: the small-batch selection and the layouts it brings in
SELECTION = ("small_kernel", "resident_kernel", "controller_kernel", "latency_ok", "done_ok", "lds")


def _opts(name):
    return {"ln_small": 1} if name == "ea_ln" else {}


# ---- 1. with the switch
@pytest.mark.parametrize("name", ps.SMALL_NAMES + ps.SMALL_PROBES)
def test_selection_with_the_switch(tmp_path, name):
    path = ps.model_path(name, tmp_path)
    got = plan(path, SW, resident_ms=100, **_opts(name))
    off = plan(path, resident_ms=100, **_opts(name))
    assert got["small_kernel"] == "policy_latency_kernel"
    assert got["latency_ok"] == 1
    assert got["resident_kernel"].startswith(MULTI + " ring="), got["resident_kernel"]
    assert got["controller_kernel"].startswith("none")
    assert got["lds"]["act"]["form"] == "multi" and "ctl" not in got["lds"]
    # without the switch: the chain, as tests/test_cpu_skip.py pins it
    assert off["small_kernel"] == CHAIN and off["resident_kernel"].startswith("none") and off["latency_ok"] == 0
    # the batched kernel, the program's scalars and every buffer are untouched by the switch
    for k in got:
        if k not in SELECTION:
            assert got[k] == off[k], k
    assert got["lds"]["gemv"] == off["lds"]["gemv"] and got["lds"]["lds_stride"] == off["lds"]["lds_stride"]
    # no resident path asked for: the single launch alone
    got0 = plan(path, SW, **_opts(name))
    assert got0["small_kernel"] == "policy_latency_kernel" and got0["resident_kernel"] == "none"


def test_ln_skip_needs_the_ln_small_bit_too(tmp_path):
    path = ps.model_path("ea_ln", tmp_path)
    for extra in ({}, {"ln_small": 2}):
        got = plan(path, SW, resident_ms=100, **extra)
        assert got["small_kernel"] == CHAIN and got["resident_kernel"] == "none" and got["latency_ok"] == 0
    for bits in (1, 3):
        got = plan(path, SW, resident_ms=100, ln_small=bits)
        assert got["small_kernel"] == "policy_latency_kernel" and got["resident_kernel"].startswith(MULTI)


def test_local_layer0_and_gather_geometry(tmp_path):
    """probe_local0 runs the local layer 0 with NF = 8; probe_gather0 has the same layer-0
    geometry and a gather, so it is tiled; GO2PI_RES_TILED0 tiles both."""
    a = plan(ps.model_path("probe_local0", tmp_path), SW, resident_ms=100)["lds"]
    b = plan(ps.model_path("probe_gather0", tmp_path), SW, resident_ms=100)["lds"]
    assert (a["k0_pad"], a["n0_pad"], a["act"]["nf"]) == (128, 128, 8)
    assert (b["k0_pad"], b["n0_pad"], b["act"]["nf"]) == (128, 128, 0)
    assert plan(ps.model_path("probe_local0", tmp_path), SW, "GO2PI_RES_TILED0", resident_ms=100)["lds"]["act"]["nf"] == 0
    r2 = plan(ps.model_path("ea_round2", tmp_path), SW, resident_ms=100)
    assert r2["one_round"] == 0 and max(g["k_pad"] for g in r2["lds"]["gemv"][1:]) == 640


# ---- 2. the switch beside other settings
@pytest.mark.parametrize("name", ["ea_98", "ea_k64", "probe_gather0"])
def test_switch_with_other_settings(tmp_path, name):
    path = ps.model_path(name, tmp_path)
    got = plan(path, SW, "GO2PI_SMALL_CHAIN", resident_ms=100)
    assert got["small_kernel"] == CHAIN and got["resident_kernel"] == "none" and got["latency_ok"] == 0
    assert plan(path, SW, small_batch=-1, resident_ms=100) == plan(path, small_batch=-1, resident_ms=100)
    assert plan(path, SW, small_batch=-1)["small_kernel"].startswith("policy_fused_kernel<8, 0, 0, 0, 0,")
    for ring in ("vram", "host"):
        got = plan(path, SW, "ring=" + ring, resident_ms=100)
        assert got["resident_kernel"] == f"{MULTI} ring={ring}"
    for sw2 in ("GO2PI_RES_MULTI", "GO2PI_RES_R1W", "GO2PI_REQ_HOST"):
        assert plan(path, SW, sw2, resident_ms=100)["resident_kernel"].startswith(MULTI + " ring=")


# ---- 3. models without a skip input
@pytest.mark.parametrize("name", ["shipped", "go2_mlp_512", "go2_gru_256", "go2_lstm_256", "mlp_small_relu", "ctl_h3",
                                  "wide_256_3", "ln_512_pre", "ln_wide_pre", "ln_ctl_post"])
def test_models_without_a_skip_plan_what_they_planned(synth_path, name):
    p = SHIPPED if name == "shipped" else synth_path(name)
    for opts in ({}, {"resident_ms": 100}, {"resident_ms": 100, "ln_small": 1}, {"small_batch": -1}):
        for ring in ("ring=vram", "ring=host"):
            assert plan(p, SW, ring, **opts) == plan(p, ring, **opts), (name, opts, ring)


def test_plain_wide_layer_keeps_its_plan(tmp_path):
    from go2_onnx_controller_amd import synth
    p = tmp_path / "plain_wide.onnx"
    p.write_bytes(synth.mlp_model_bytes(**lm.PLAIN_WIDE))
    assert plan(p, SW, resident_ms=100) == plan(p, resident_ms=100)


# ---- 4. LDS regions
@pytest.mark.parametrize("tiled0", [False, True])
@pytest.mark.parametrize("name", ps.SMALL_NAMES + ps.SMALL_PROBES)
def test_lds_regions(tmp_path, name, tiled0):
    sw = [SW] + (["GO2PI_RES_TILED0"] if tiled0 else [])
    lds = plan(ps.model_path(name, tmp_path), *sw, resident_ms=100, **_opts(name))["lds"]
    view = ps.expected_view(name)
    kmax = max((ly["K"] + 63) // 64 * 64 for ly in view)
    for key in ("latency", "act"):
        f = lds[key]
        assert f["total_bytes"] % 4 == 0 and f["total_bytes"] <= 160 * 1024
        check_regions(f["regions"], f["total_bytes"] // 4)
        size = {n: s for n, _, s in f["regions"]}
        assert size["xs"] >= 8 * kmax  # eight rows of the widest layer input, skip columns included
        if key == "act":
            assert size["obsv"] >= 8 * ps.in_dim(name)  # the raw rows a skip layer reads


# ---- 5. the probes and the float model's input condition
@pytest.mark.parametrize("name", ps.SKIP_SMALL.probes)
def test_probe_is_exact_and_every_unit_matters(tmp_path, name):
    bound = ps.probe_bound(name)
    print(f"{name}: largest sum |w||h| + |b| = {bound} (2^24 = {1 << 24})")
    assert bound < 1 << 24
    ref = ln_ref.LnRef(ps.model_path(name, tmp_path))
    for B in (33,) + tuple(sorted(set(ps.SKIP_SMALL.probe_batches))):
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


def test_input_condition_of_the_new_float_model(tmp_path):
    """ea_round2 on the inputs tests/test_gpu_skip_small.py uses: float32 arithmetic alone
    stays under a third of the tolerance."""
    name = "ea_round2"
    ref = ln_ref.LnRef(ps.model_path(name, tmp_path))
    worst = 0.0
    for B in ps.SKIP_SMALL.small_batches:
        for k in (0, 1):
            x = ps.obs(name, B, k)
            worst = max(worst, abs_err(ref.f32(x), ref.f64(x)))
    print(f"{name}: worst fp32-vs-fp64 error {worst:.3g}")
    assert worst <= 1e-5 / 3


# ---- 6. loader view
@pytest.mark.parametrize("name", ps.SKIP_SMALL.names + ps.SKIP_SMALL.probes)
def test_loader_view(tmp_path, name):
    v = ps.inspect(ps.model_path(name, tmp_path))
    assert v["in_dim"] == ps.in_dim(name)
    got = [{k: ly[k] for k in ("K", "N", "act", "ln", "skip", "res")} for ly in v["layers"]]
    assert got == ps.expected_view(name)
