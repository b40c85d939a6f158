"""CPU: estimator-actor policies (observation skip inputs, the skip family of tests/policy_specs.py) through the
loader, the planner and the oracle; no device is touched.

1. the loader's view (inspect_model): K, N, act, ln and the skip columns per layer, and the
   checksum of the permuted weights; unchanged views with "skip": [] for earlier models;
2. every refusal, one graph each, by its message;
3. the plan (tests/cpp/plan_probe.cpp): general batched body, GEMV chain, no resident kernel;
4. the input condition of tests/test_gpu_skip.py: float32 against float64 on exactly its inputs;
5. the integer probes: exactness bound, and every observation column and latent unit matters;
6. the loader under AddressSanitizer / UBSan on the graphs and a few hundred mutations of each.
"""
import numpy as np
import pytest

import graphs
import ln_ref
import policy_specs as ps
from conftest import SHIPPED, abs_err
from go2_onnx_controller_amd import onnx_writer as ow
from loader_harness import harness, run as _run  # noqa: F401 (harness: a fixture)


# ---- 1. loader view
@pytest.mark.parametrize("name", ps.SKIP.names + ps.SKIP.probes)
def test_loader_view(tmp_path, name):
    v = ps.inspect(ps.model_path(name, tmp_path))
    assert v["in_dim"] == ps.in_dim(name)
    got = [{k: ly[k] for k in ("K", "N", "act", "ln", "skip", "res")} for ly in v["layers"]]
    assert got == ps.expected_view(name)
    # checksums are of the permuted W (device column order)
    for ly, W, (_, b, _, _) in zip(v["layers"], ps.device_weights(name), ps.weights(name)):
        s = 0.0
        for x in W.ravel():  # the loader's own order and precision: a double sum over [N][K]
            s += float(x)
        assert ly["w_sum"] == s
        assert ly["b_sum"] == float(np.sum(b.astype(np.float64)))
    c = ps.front_constants(name)
    assert v["pre_sub"] == (ps.in_dim(name) if c else 0) and v["pre_clip"] == ([-5.0, 5.0] if c else [-1e308, 1e308])


def test_permutation_is_not_the_identity():
    """ea_k64 and ea_two put observation parts first: device order differs from ONNX order."""
    for name, l in (("ea_k64", 3), ("ea_two", 2), ("probe_k64", 2)):
        assert not np.array_equal(ps.device_weights(name)[l], ps.weights(name)[l][0])
    assert np.array_equal(ps.device_weights("ea_98")[3], ps.weights("ea_98")[3][0])


@pytest.mark.parametrize("kind", ["shipped", "slice_concat_blocks", "slice_concat_mixed"])
def test_earlier_models_report_no_skip(tmp_path, kind):
    v = ps.inspect(SHIPPED if kind == "shipped" else graphs.write(tmp_path, kind))
    assert all(ly["skip"] == [] for ly in v["layers"]) and len(v["layers"]) >= 1
    if kind != "shipped":  # the front-end is still a prologue, layer 0 reads every column
        assert v["pre_sub"] > 1 or v["pre_div"] > 1 or v["pre_mul"] > 1
        assert v["layers"][0]["K"] == v["in_dim"]


def test_held_scale_folds_into_the_running_columns_only(tmp_path):
    """A Mul after the encoder's activation, held across the Concat: the running value's weight
    columns carry it, the observation parts' columns do not."""
    r = np.random.default_rng(5)
    W0, W1 = r.standard_normal((6, 8)).astype(np.float32), r.standard_normal((3, 10)).astype(np.float32)
    sc = r.uniform(0.5, 2.0, 6).astype(np.float32)
    inits = [("W0", W0), ("W1", W1), ("sc", sc), ("st", np.array([2], np.int64)), ("en", np.array([6], np.int64)),
             ("ax", np.array([1], np.int64))]
    nodes = [ow.node("Gemm", ["obs", "W0"], ["g0"], "", [ow.attr_int("transB", 1)]),
             ow.node("Tanh", ["g0"], ["t0"]), ow.node("Mul", ["t0", "sc"], ["z"]),
             ow.node("Slice", ["obs", "st", "en", "ax"], ["part"]), ow.node("Identity", ["part"], ["part_i"]),
             ow.node("Concat", ["part_i", "z"], ["cat"], "", [ow.attr_int("axis", 1)]),
             ow.node("Gemm", ["cat", "W1"], ["act"], "", [ow.attr_int("transB", 1)])]
    p = tmp_path / "held.onnx"
    p.write_bytes(ow.model(nodes, inits, [("obs", ["N", 8])], [("act", ["N", 3])]))
    v = ps.inspect(p)
    assert v["layers"][1]["skip"] == [2, 3, 4, 5] and v["layers"][1]["K"] == 10
    want = np.concatenate([W1[:, 4:] * sc, W1[:, :4]], axis=1)  # device order, the scale on the first 6
    s = 0.0
    for x in want.ravel():
        s += float(x)
    assert abs(v["layers"][1]["w_sum"] - s) < 1e-5
    ref = ln_ref.LnRef(str(p))
    x = r.standard_normal((4, 8)).astype(np.float32)
    y = np.concatenate([np.tanh(x.astype(np.float64) @ W0.T.astype(np.float64)), x[:, 2:6]], axis=1) @ want.T.astype(np.float64)
    assert abs_err(ref.f64(x), y) < 1e-6


# ---- 2. refusals
def _refusal(kind):
    """obs[8] -> Gemm(6) -> Tanh -> z; then the faulty construct -> Gemm -> act[3]."""
    r = np.random.default_rng(11)
    f32 = lambda *s: r.standard_normal(s).astype(np.float32)  # noqa: E731
    i64 = lambda *v: np.array(v, np.int64)  # noqa: E731
    inits = [("W0", f32(6, 8)), ("st", i64(0)), ("en", i64(4)), ("ax", i64(1))]
    nodes = [ow.node("Gemm", ["obs", "W0"], ["g0"], "", [ow.attr_int("transB", 1)]), ow.node("Tanh", ["g0"], ["z"])]
    gemm = lambda x, k: [ow.node("Gemm", [x, "W1"], ["act"], "", [ow.attr_int("transB", 1)])]  # noqa: E731
    sl = ow.node("Slice", ["obs", "st", "en", "ax"], ["part"])
    cat = lambda ins, axis=1: ow.node("Concat", ins, ["cat"], "cat", [ow.attr_int("axis", axis)])  # noqa: E731
    inputs = [("obs", [1, 8])]
    if kind == "two_running":
        inits += [("W0b", f32(6, 8)), ("W1", f32(3, 12))]
        nodes = [ow.node("Gemm", ["obs", "W0b"], ["h0"], "", [ow.attr_int("transB", 1)]), ow.node("Relu", ["h0"], ["zb"])] + nodes
        nodes += [cat(["z", "zb"])] + gemm("cat", 12)
    elif kind == "axis0":
        inits += [("W1", f32(3, 10))]
        nodes += [sl, cat(["z", "part"], 0)] + gemm("cat", 10)
    elif kind == "step2":
        inits += [("W1", f32(3, 8)), ("sp", i64(2))]
        nodes += [ow.node("Slice", ["obs", "st", "en", "ax", "sp"], ["part"]), cat(["z", "part"])] + gemm("cat", 8)
    elif kind == "batch_axis":
        inits += [("W1", f32(3, 14)), ("ax0", i64(0))]
        nodes += [ow.node("Slice", ["obs", "st", "en", "ax0"], ["part"]), cat(["z", "part"])] + gemm("cat", 14)
    elif kind == "part_arith":  # the part is scaled, layer 0 reads the raw observation
        inits += [("W1", f32(3, 10)), ("two", np.array(2.0, np.float32))]
        nodes += [sl, ow.node("Mul", ["part", "two"], ["part2"]), cat(["z", "part2"])] + gemm("cat", 10)
    elif kind == "part_raw":  # layer 0 reads the normalised observation, the part the raw one
        inits = [("mean", f32(8))] + inits + [("W1", f32(3, 10))]
        nodes = [ow.node("Sub", ["obs", "mean"], ["x0"]),
                 ow.node("Gemm", ["x0", "W0"], ["g0"], "", [ow.attr_int("transB", 1)]), ow.node("Tanh", ["g0"], ["z"]),
                 sl, cat(["z", "part"])] + gemm("cat", 10)
    elif kind == "act_on_concat":
        inits += [("W1", f32(3, 10))]
        nodes += [sl, cat(["z", "part"]), ow.node("Relu", ["cat"], ["rc"])] + gemm("rc", 10)
    elif kind == "ln_on_concat":
        inits += [("W1", f32(3, 10)), ("g", np.ones(10, np.float32))]
        nodes += [sl, cat(["z", "part"]), ow.node("LayerNormalization", ["cat", "g"], ["rc"], "", [ow.attr_int("axis", -1)])]
        nodes += gemm("rc", 10)
    elif kind == "clip_on_concat":
        inits += [("W1", f32(3, 10)), ("lo", np.array(-1, np.float32)), ("hi", np.array(1, np.float32))]
        nodes += [sl, cat(["z", "part"]), ow.node("Clip", ["cat", "lo", "hi"], ["rc"])] + gemm("rc", 10)
    elif kind == "residual":
        inits += [("W1", f32(3, 6)), ("W0b", f32(6, 6))]
        nodes += [ow.node("Gemm", ["z", "W0b"], ["h1"], "", [ow.attr_int("transB", 1)]), ow.node("Add", ["h1", "z"], ["s"])]
        nodes += gemm("s", 6)
    elif kind == "front_only":  # observation parts alone in front of layer 0, out of order
        inits = [("W1", f32(3, 8)), ("st", i64(0)), ("en", i64(4)), ("ax", i64(1)), ("st2", i64(4)), ("en2", i64(8))]
        nodes = [sl, ow.node("Slice", ["obs", "st2", "en2", "ax"], ["part2"]), cat(["part2", "part"])] + gemm("cat", 8)
    elif kind == "gru":
        H = 16
        inits = [("Wg", f32(1, 3 * H, 8)), ("Rg", f32(1, 3 * H, H)), ("Bg", f32(1, 6 * H)), ("ax0", i64(0)),
                 ("W1", f32(3, H + 4)), ("st", i64(0)), ("en", i64(4)), ("ax", i64(1))]
        nodes = [ow.node("Unsqueeze", ["obs", "ax0"], ["x3"]),
                 ow.node("GRU", ["x3", "Wg", "Rg", "Bg", "", "h_in"], ["Y", "Yh"], "gru",
                         [ow.attr_int("hidden_size", H), ow.attr_int("linear_before_reset", 1)]),
                 ow.node("Squeeze", ["Yh", "ax0"], ["z"]), sl, cat(["z", "part"])] + gemm("cat", H + 4)
        inputs = [("obs", [1, 8]), ("h_in", [1, 1, H])]
    else:
        raise KeyError(kind)
    return ow.model(nodes, inits, inputs, [("act", [1, 3])])


REFUSALS = {
    "two_running": "Concat of two running values",
    "axis0": "must be on the feature axis",
    "step2": "Slice with a step other than 1",
    "batch_axis": "Slice on the batch axis",
    "part_arith": "with no arithmetic of its own",
    "part_raw": "must be taken from the value layer 0 reads",
    "act_on_concat": "a skip Concat must feed a Gemm or MatMul: 'Relu'",
    "ln_on_concat": "a skip Concat must feed a Gemm or MatMul: 'LayerNormalization'",
    "clip_on_concat": "a skip Concat must feed a Gemm or MatMul: 'Clip'",
    "residual": "a residual connection",
    "front_only": "cover its columns in order",
    "gru": "a skip Concat in a policy with a GRU or LSTM cell",
}


@pytest.mark.parametrize("kind", list(REFUSALS))
def test_refusals(tmp_path, kind):
    from go2_onnx_controller_amd import engine
    p = tmp_path / f"{kind}.onnx"
    p.write_bytes(_refusal(kind))
    with pytest.raises(engine.Go2piError, match=REFUSALS[kind]) as ei:
        engine.inspect_model(str(p))
    assert "GO2PI_E_MODEL" in str(ei.value) or ei.value.args
    # the oracle evaluates the others: a refusal is the loader's decision, not a malformed graph
    if kind not in ("gru", "axis0"):  # (axis 0: the widths differ, no such tensor)
        x = np.random.default_rng(0).standard_normal((1, 8)).astype(np.float32)
        assert np.isfinite(ln_ref.LnRef(str(p)).f64(x)).all()


# ---- 3. plan
@pytest.mark.parametrize("name", ["ea_98", "ea_k64"])
def test_plan(tmp_path, name):
    from test_cpu_plan import plan
    path = ps.model_path(name, tmp_path)
    for extra in ({}, {"ln_small": 3}):
        for waves, nw in ((0, 8), (4, 4), (8, 8), (16, 16)):
            got = plan(path, waves=waves, resident_ms=100, **extra)
            assert got["batched_kernel"].startswith(f"policy_fused_kernel<{nw}, 0, 0, 0, 0,"), got["batched_kernel"]
            assert got["small_kernel"] == "gemv_layer_kernel graph"
            assert got["resident_kernel"].startswith("none"), got["resident_kernel"]
            assert got["controller_kernel"].startswith("none")
            assert got["latency_ok"] == 0 and got["w4_tpw"] == 0
    got = plan(path, resident_ms=100)
    cost = got["cost"]
    view = ps.expected_view(name)
    assert cost["flops_per_row"] == sum(2.0 * ly["K"] * ly["N"] for ly in view)  # the layers' real K
    assert cost["weight_bytes"] == sum(4.0 * (ly["K"] * ly["N"] + ly["N"]) for ly in view)
    # the skip layer's K_pad = ceil64(prev.N + skip_n), the layer in front padded to it
    k = [g["k_pad"] for g in got["lds"]["gemv"]]
    assert k == [(ly["K"] + 63) // 64 * 64 for ly in view]
    assert got["lds_stride"] >= max(k) + 4


def test_plan_head_fuse(tmp_path):
    from test_cpu_plan import plan
    # a skip on the head itself: no head fusion; on the layer in front of the head: as ever
    assert plan(ps.model_path("ea_head", tmp_path))["head_fuse"] == 0
    assert plan(ps.model_path("ea_sig", tmp_path), waves=4)["head_fuse"] == 1


# ---- 4. the oracle's own float32 error on the GPU tests' inputs
@pytest.mark.parametrize("name", ps.SKIP.names)
def test_input_condition(tmp_path, name):
    ref = ln_ref.LnRef(ps.model_path(name, tmp_path))
    worst = 0.0
    for B in ps.SKIP.parity_batches:
        for k in (0, 1):
            x = ps.obs(name, B, k)
            worst = max(worst, abs_err(ref.f32(x), ref.f64(x)))
    print(f"{name}: worst fp32-vs-fp64 error {worst:.3g}")
    assert worst <= 1e-5 / 3
    c = ps.front_constants(name)
    if c:  # the front's Clip binds on both sides
        v = (ps.obs(name, 33) - c[0]) / c[1]
        assert (v < -c[2]).any() and (v > c[2]).any()


# ---- 5. probes
@pytest.mark.parametrize("name", ps.SKIP.probes)
def test_probe_is_exact_and_every_unit_matters(tmp_path, name):
    bound = ps.probe_bound(name)
    print(f"{name}: largest sum |w||h| + |b| = {bound} (2^24 = {1 << 24})")
    assert bound < 1 << 24
    ref = ln_ref.LnRef(ps.model_path(name, tmp_path))
    x = ps.probe_obs(name, 33)
    want = ps.probe_forward(name, x)
    for dt in (np.float64, np.float32):  # the oracle agrees with the int64 answer, exactly
        y = ref._act(x, dt)
        assert np.array_equal(y, want.astype(dt)), dt
    assert np.abs(want).max() <= bound
    _, _, layers = ps.spec(name)
    for j in range(ps.in_dim(name)):
        assert not np.array_equal(ps.probe_forward(name, x, zero_unit=(-1, j)), want), ("obs", j)
    for l, ly in enumerate(layers[:-1]):
        for j in range(ly["n"]):
            assert not np.array_equal(ps.probe_forward(name, x, zero_unit=(l, j)), want), (l, j)


# ---- 6. the loader under the sanitizers (a stand-alone program, tests/loader_harness.py)
def _mutations(name, n):
    """n mutations of the model: truncations, bit flips, and every Slice bound rewritten to a
    negative, huge or past-the-width value (the int64 initialisers' payloads and the
    attribute-form varints)."""
    data = ps.model_bytes(name)
    rng = np.random.default_rng(ps.weight_seed(name) + 7)
    out = []
    bounds = [-1, -3, -(1 << 40), -(1 << 63), (1 << 63) - 1, 1 << 40, (1 << 31) - 1, ps.in_dim(name) + 1, 0, 1 << 31]
    # the Slice bounds stored as int64 raw_data: an 8-byte little-endian payload behind "st<k>" / "en<k>"
    spots = []
    for key in (b"st", b"en"):
        at = 0
        while True:
            at = data.find(key, at)
            if at < 0:
                break
            j = data.find(b"\x4a\x08", at, at + 16)  # field 9 (raw_data), 8 bytes
            if j >= 0:
                spots.append(j + 2)
            at += 2
    for i in range(n):
        d = bytearray(data)
        kind = i % 3
        if kind == 0:
            d = d[: int(rng.integers(0, len(d)))]
        elif kind == 1:
            for _ in range(int(rng.integers(1, 8))):
                d[int(rng.integers(0, len(d)))] ^= 1 << int(rng.integers(0, 8))
        elif spots:
            for s in rng.choice(spots, size=min(len(spots), int(rng.integers(1, 3))), replace=False):
                v = bounds[int(rng.integers(0, len(bounds)))]
                d[s:s + 8] = int(v & ((1 << 64) - 1)).to_bytes(8, "little")
        out.append(bytes(d))
    return out


def test_loader_sanitized(harness, tmp_path):
    paths, n_valid = [], 0
    for name in ps.SKIP.names:
        paths.append(ps.model_path(name, tmp_path))
        n_valid += 1
    for name in ps.SKIP.names:
        for i, d in enumerate(_mutations(name, 300)):
            p = tmp_path / f"{name}_m{i}.onnx"
            p.write_bytes(d)
            paths.append(p)
    for kind in REFUSALS:
        p = tmp_path / f"refuse_{kind}.onnx"
        p.write_bytes(_refusal(kind))
        paths.append(p)
    lines = []
    for k in range(0, len(paths), 500):
        lines += _run(harness, paths[k:k + 500])
    assert all(l.startswith("ok ") for l in lines[:n_valid]), lines[:n_valid]
    assert all(l.startswith(("ok ", "error ")) for l in lines)
    assert all(l.startswith("error onnx: ") for l in lines[-len(REFUSALS):])
    muts = lines[n_valid:-len(REFUSALS)]
    assert sum(l.startswith("error") for l in muts) > len(muts) // 4
    assert sum(l.startswith("ok") for l in muts) > 0  # (a clamped Slice bound can still load)
