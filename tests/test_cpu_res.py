"""CPU: residual MLP policies (the res family of tests/policy_specs.py): what the loader reports (Dense::res), the
forms it refuses, the integer probes' own arithmetic, the input condition of the GPU tests
(float32 alone stays under a third of the tolerance) and the plan (policy_fused_res_kernel<8>
and the GEMV chain, nothing else), with the plan of policies without a residual pinned to the
parent commit's (tests/golden/res_plan_parent.json).
"""
import json
import os

import numpy as np
import pytest

import graphs
import ln_ref
import ln_small_models as lm
import policy_specs as ps
from conftest import GOLDEN, SHIPPED, abs_err
from go2_onnx_controller_amd import onnx_writer as ow

TOL = 1e-5
E_INVALID, E_MODEL = -1, -2  # include/go2pi.h
KEYS = ("K", "N", "act", "ln", "skip", "res")


# ---- 1. the loader's view
@pytest.mark.parametrize("name", ps.RES.names + ps.RES.probes)
def test_inspect(name):
    v = ps.inspect(ps.path(name))
    assert v["in_dim"] == ps.in_dim(name)
    assert [{k: ly[k] for k in KEYS} for ly in v["layers"]] == ps.expected_view(name)


@pytest.mark.parametrize("kind", ["matmul_add_sigmoid", "relu_deep"])
def test_plain_model_reports_no_residual(tmp_path, kind):
    from go2_onnx_controller_amd import engine
    p = tmp_path / "plain.onnx"
    p.write_bytes(graphs.variant_bytes(kind))
    layers = engine.inspect_model(str(p))["layers"]
    assert len(layers) >= 2 and all(ly["res"] == -1 for ly in layers)
    assert all(ly["res"] == -1 for ly in engine.inspect_model(SHIPPED)["layers"])


# ---- 2. refusals
def _refusal(kind):
    """obs[8] -> Gemm(6) g0 -> Relu -> z; then the refused construct; -> act."""
    r = np.random.default_rng(23)
    f32 = lambda *s: (r.standard_normal(s) * 0.5).astype(np.float32)  # noqa: E731
    tb = [ow.attr_int("transB", 1)]
    gemm = lambda x, w, y: ow.node("Gemm", [x, w], [y], "", tb)  # noqa: E731
    add = lambda a, b, y: ow.node("Add", [a, b], [y], "add_" + y)  # noqa: E731
    relu = lambda x, y: ow.node("Relu", [x], [y])  # noqa: E731
    inits = [("W0", f32(6, 8)), ("W1", f32(6, 6)), ("W2", f32(6, 6)), ("W3", f32(6, 6)), ("Wo", f32(3, 6)),
             ("g", np.ones(6, np.float32))]
    nodes = [gemm("obs", "W0", "g0"), relu("g0", "z")]
    inputs, out_n = [("obs", [1, 8])], 3
    ln = lambda x, y: ow.node("LayerNormalization", [x, "g"], [y], "", [ow.attr_int("axis", -1)])  # noqa: E731
    if kind == "two_adds":
        nodes += [gemm("z", "W1", "h1"), add("h1", "z", "s1"), relu("s1", "a1"), gemm("a1", "W2", "h2"),
                  add("h2", "z", "s2"), relu("s2", "a2"), gemm("a2", "Wo", "act")]
    elif kind == "three_consumers":
        nodes += [gemm("z", "W1", "h1"), gemm("z", "W2", "side"), add("h1", "z", "s1"), relu("s1", "a1"),
                  gemm("a1", "Wo", "act")]
    elif kind == "nested":
        nodes += [gemm("z", "W1", "h1"), relu("h1", "a1"), gemm("a1", "W2", "h2"), add("h2", "a1", "s2"),
                  relu("s2", "a2"), gemm("a2", "W3", "h3"), add("h3", "z", "s3"), relu("s3", "a3"),
                  gemm("a3", "Wo", "act")]
    elif kind == "width":  # a 1-wide carried value broadcast over 6 features
        inits += [("Wn", f32(1, 6)), ("Wb", f32(6, 1))]
        nodes += [gemm("z", "Wn", "hn"), relu("hn", "t"), gemm("t", "Wb", "h1"), add("h1", "t", "s1"),
                  relu("s1", "a1"), gemm("a1", "Wo", "act")]
    elif kind == "obs_add":
        inits += [("W8", f32(8, 8)), ("Wo8", f32(3, 8))]
        nodes = [gemm("obs", "W8", "h0"), add("h0", "obs", "s0"), relu("s0", "a0"), gemm("a0", "Wo8", "act")]
    elif kind == "obs_slice_add":
        inits += [("st", np.array([0], np.int64)), ("en", np.array([6], np.int64)), ("ax", np.array([1], np.int64))]
        nodes = [gemm("obs", "W0", "g0"), ow.node("Slice", ["obs", "st", "en", "ax"], ["part"]),
                 add("g0", "part", "s0"), relu("s0", "a0"), gemm("a0", "Wo", "act")]
    elif kind == "output_layer":
        nodes += [gemm("z", "W1", "h1"), relu("h1", "a1"), gemm("a1", "W2", "h2"), add("h2", "a1", "act")]
        out_n = 6
    elif kind == "post_act":  # x + act(W x)
        nodes += [gemm("z", "W1", "h1"), relu("h1", "a1"), add("a1", "z", "s1"), gemm("s1", "Wo", "act")]
    elif kind == "bronet":  # x + LN(W x)
        nodes += [gemm("z", "W1", "h1"), ln("h1", "n1"), add("n1", "z", "s1"), relu("s1", "a1"),
                  gemm("a1", "Wo", "act")]
    elif kind == "pre_act_tap":  # the tap between a Gemm and its activation, no LN
        nodes += [gemm("z", "W1", "h1"), add("h1", "g0", "s1"), relu("s1", "a1"), gemm("a1", "Wo", "act")]
    elif kind == "ln_out_tap":
        nodes = [gemm("obs", "W0", "g0"), ln("g0", "n0"), relu("n0", "z"), gemm("z", "W1", "h1"),
                 add("h1", "n0", "s1"), relu("s1", "a1"), gemm("a1", "Wo", "act")]
    elif kind == "held_scale":
        inits += [("two", np.array(2.0, np.float32))]
        nodes += [ow.node("Mul", ["z", "two"], ["zs"]), gemm("zs", "W1", "h1"), add("h1", "zs", "s1"), relu("s1", "a1"),
                  gemm("a1", "Wo", "act")]
    elif kind == "gru":
        H = 6
        inits += [("Wg", f32(1, 3 * H, 8)), ("Rg", f32(1, 3 * H, H)), ("Bg", f32(1, 6 * H)),
                  ("ax0", np.array([0], np.int64))]
        nodes = [ow.node("Unsqueeze", ["obs", "ax0"], ["x3"]),
                 ow.node("GRU", ["x3", "Wg", "Rg", "Bg", "", "h_in"], ["Y", "Yh"], "gru",
                         [ow.attr_int("hidden_size", H), ow.attr_int("linear_before_reset", 1)]),
                 ow.node("Squeeze", ["Yh", "ax0"], ["z"]), gemm("z", "W1", "h1"), relu("h1", "a1"),
                 gemm("a1", "W2", "h2"), add("h2", "a1", "s2"), relu("s2", "a2"), gemm("a2", "Wo", "act")]
        inputs = [("obs", [1, 8]), ("h_in", [1, 1, H])]
    elif kind == "gemm_add_gemm":  # tests/test_cpu_skip.py's graph, its message unchanged
        from test_cpu_skip import _refusal as skip_refusal
        return skip_refusal("residual")
    elif kind == "two_networks":  # matches none of the residual forms: today's message
        nodes = [gemm("obs", "W0", "g0"), relu("g0", "z"), gemm("obs", "W0", "g0b"), ow.node("Tanh", ["g0b"], ["zb"]),
                 add("z", "zb", "s"), gemm("s", "Wo", "act")]
    else:
        raise KeyError(kind)
    return ow.model(nodes, inits, inputs, [("act", [1, out_n])])


REFUSALS = {
    "two_adds": "is consumed by more than one Add",
    "three_consumers": "a value with more than two consumers",
    "nested": "nested or overlapping residual connections",
    "width": "adds the 1 features of layer 1 to the 6 of layer 2",
    "obs_add": "the observation .or a Slice of it. as the added operand",
    "obs_slice_add": "the observation .or a Slice of it. as the added operand",
    "output_layer": "a residual connection on the output layer",
    "post_act": "added behind a layer's activation or LayerNormalization",
    "bronet": "added behind a layer's activation or LayerNormalization",
    "pre_act_tap": "tapped between a Gemm / MatMul and its activation",
    "ln_out_tap": "tapped from a LayerNormalization's output",
    "held_scale": "a constant Mul / Div",
    "gru": "a residual connection in a policy with a GRU or LSTM cell",
    "gemm_add_gemm": "a residual connection",
    "two_networks": "Add of two computed values .a residual connection. is unsupported",
}


@pytest.mark.parametrize("kind", list(REFUSALS))
def test_refusals(tmp_path, kind):
    from go2_onnx_controller_amd import engine
    p = tmp_path / f"{kind}.onnx"
    p.write_bytes(_refusal(kind))
    with pytest.raises(engine.Go2piError, match=REFUSALS[kind]) as ei:
        engine.inspect_model(str(p))
    assert "residual connection" in str(ei.value)
    # the reference evaluates it: a refusal is the loader's decision, not a malformed graph
    if kind != "gru":
        x = np.random.default_rng(0).standard_normal((1, 8)).astype(np.float32)
        assert np.isfinite(ln_ref.LnRef(str(p)).f64(x)).all()


# ---- 3. the probes' own arithmetic
@pytest.mark.parametrize("name", ps.RES.probes)
def test_probe_forward_is_the_reference(name):
    ref = ps.ref(name)
    assert ps.probe_bound(name) < 2 ** 24
    for B in (33, 1, 16, 17, 8, 5):
        x = ps.probe_obs(name, B)
        want = ps.probe_forward(name, x)
        for y in (ref.f64(x), ref.f32(x)):
            assert np.array_equal(y, want.astype(y.dtype)) and np.array_equal(y.astype(np.int64), want)


@pytest.mark.parametrize("name", ps.RES.probes)
def test_probe_observes_the_carried_path(name):
    """Zeroing any unit of a carried value on its way to the Add (the main chain keeps the
    unit) changes an output: a kernel that drops or misplaces the carried value is seen."""
    _, _, layers = ps.spec(name)
    x = ps.probe_obs(name, 33)
    want = ps.probe_forward(name, x)
    for l, ly in enumerate(layers):
        if ly["res"] is None:
            continue
        for j in range(ly["n"]):
            assert not np.array_equal(ps.probe_forward(name, x, zero_carried=(l, j)), want), (name, l, j)


# ---- 4. the input condition of tests/test_gpu_res.py
@pytest.mark.parametrize("name", ps.RES.names)
def test_float32_alone_is_within_a_third_of_the_tolerance(name):
    ref = ps.ref(name)
    for B in ps.RES.parity_batches:
        for k in range(3 if B in (5, 33) else 1):
            x = ps.obs(name, B, k)
            err = abs_err(ref.f32(x), ref.f64(x))
            assert err <= TOL / 3, (name, B, k, err)


# ---- 5. plan
@pytest.mark.parametrize("name", ps.RES.names + ps.RES.probes)
def test_plan(name):
    from test_cpu_plan import plan
    path = ps.path(name)
    for args, extra in (((), {}), (("GO2PI_SKIP_SMALL",), {"ln_small": 3}), ((), {"waves": 8})):
        got = plan(path, *args, resident_ms=100, **extra)
        assert got["batched_kernel"].startswith("policy_fused_res_kernel<8>"), got["batched_kernel"]
        assert got["small_kernel"] == "gemv_layer_kernel graph"
        assert got["resident_kernel"].startswith("none"), got["resident_kernel"]
        assert got["controller_kernel"].startswith("none")
        assert got["waves"] == 8 and got["latency_ok"] == 0 and got["done_ok"] == 0
        assert got["w4_tpw"] == 0 and got["head_fuse"] == 0
    assert plan(path, small_batch=-1)["small_kernel"].startswith("policy_fused_res_kernel<8>")
    for waves in (4, 16):
        got = plan(path, waves=waves)
        assert got["code"] == E_INVALID and "residual connections" in got["error"] and f"waves = {waves}" in got["error"]


def test_plan_res_skip_consumer_is_padded_past_its_source():
    """res_skip: the consumer's N_pad (its skip successor's K_pad) exceeds the source's, so
    the carried tile has columns no source writes."""
    from test_cpu_plan import plan
    got = plan(ps.path("res_skip"))
    k_pad = [g["k_pad"] for g in got["lds"]["gemv"]]
    assert k_pad[3] == 64 and k_pad[5] == 128  # N_pad of layers 2 (the source) and 4 (the consumer)


def test_plan_cost_counts_the_add():
    from test_cpu_plan import plan
    _, _, layers = ps.spec("simba_64")
    want = sum(2.0 * k * ly["n"] for k, ly in zip([48] + [ly["n"] for ly in layers[:-1]], layers))
    want += sum(ly["n"] for ly in layers if ly["res"] is not None)
    assert plan(ps.path("simba_64"))["cost"]["flops_per_row"] == want


def _wide_bytes(width):
    r = np.random.default_rng(5)
    f32 = lambda *s: (r.standard_normal(s) * 0.03).astype(np.float32)  # noqa: E731
    tb = [ow.attr_int("transB", 1)]
    nodes = [ow.node("Gemm", ["obs", "W0"], ["g0"], "", tb), ow.node("Relu", ["g0"], ["z"]),
             ow.node("Gemm", ["z", "W1"], ["h1"], "", tb), ow.node("Add", ["h1", "z"], ["s1"]),
             ow.node("Relu", ["s1"], ["a1"]), ow.node("Gemm", ["a1", "Wo"], ["act"], "", tb)]
    inits = [("W0", f32(width, 48)), ("W1", f32(width, width)), ("Wo", f32(12, width))]
    return ow.model(nodes, inits, [("obs", ["batch", 48])], [("act", ["batch", 12])])


def test_plan_lds(tmp_path):
    """Three [16][width + 4] buffers: 512 wide fits (99 KiB), 896 wide passes 160 KiB and is
    refused with the width in the message; without the Add the same 896-wide layers fit."""
    from test_cpu_plan import plan
    p = tmp_path / "w512.onnx"
    p.write_bytes(_wide_bytes(512))
    got = plan(str(p), small_batch=-1)
    assert got["batched_kernel"].startswith("policy_fused_res_kernel<8>") and got["lds_stride"] == 516
    p = tmp_path / "w896.onnx"
    p.write_bytes(_wide_bytes(896))
    got = plan(str(p))
    assert got["code"] == E_MODEL and "layer width 896" in got["error"] and "carried tile" in got["error"]


# the plan of policies without a residual, as the parent commit's build printed it
PARENT_CASES = {
    "shipped": {}, "shipped_b": {"small_batch": -1}, "shipped_r": {"resident_ms": 100},
    "ln_512_pre": {}, "ln_512_pre_s": {"ln_small": 3, "resident_ms": 100},
    "ea_98": {}, "ea_98_r": {"resident_ms": 100, "waves": 16},
}


def parent_case_path(case, directory):
    if case.startswith("shipped"):
        return SHIPPED
    if case.startswith("ln_512_pre"):
        return lm.model_path("ln_512_pre", directory)
    return ps.model_path("ea_98", directory)


@pytest.mark.parametrize("case", list(PARENT_CASES))
def test_plan_without_a_residual_is_the_parents(case, tmp_path):
    from test_cpu_plan import plan
    with open(os.path.join(GOLDEN, "res_plan_parent.json")) as fh:
        want = json.load(fh)[case]
    assert plan(parent_case_path(case, tmp_path), **PARENT_CASES[case]) == want
