"""CPU: the probe policies of tests/probe_models.py themselves, for every probe and input
schedule the GPU tests use (test_gpu_probe_shapes.py, test_gpu_probe_activations.py).

Integer probes: the exactness condition (abs_sum_bound < 2^24), the oracle's float64 and
float32 evaluation equal to the int64 reference bit for bit (a pin of oracle/onnx_ref.py
that does not come from itself), zero unobserved observation columns and hidden units
(a condition on the generator: a kernel that mishandles any one of them changes an
output), a tail that binds, and the loader's view of each graph.
Activation probes: the oracle's float64 answer equals the module's per-element reference
to 1e-15 relative, its float32 answer is inside the GPU tests' bound (so the bound is
one float32 arithmetic can meet), and the loader's view.

Not probed, as probe_models.py explains: recurrent cells, controller ticks,
LayerNormalization, multi-GPU, timing."""
import numpy as np
import pytest

import probe_models as pm

SCHEDULES = ([(n, "small") for n in pm.SMALL_PROBES] + [(n, "batched") for n in pm.BATCHED_PROBES])


def _rows(name, which):
    _, layers = pm.int_probe(name)
    return np.concatenate(pm.int_inputs(layers, pm.SMALL_SCHEDULE if which == "small" else pm.BATCH_SCHEDULE))


def test_every_probe_is_scheduled():
    assert set(pm.SMALL_PROBES) | set(pm.BATCHED_PROBES) == set(pm.INT_PROBES)


@pytest.mark.parametrize("name,which", SCHEDULES)
def test_int_probe_exact_and_observed(name, which):
    from oracle import onnx_ref
    data, layers = pm.int_probe(name)
    xs = _rows(name, which)
    lo = -6 if layers["front"] is not None else -3
    assert xs.min() >= lo - 3 and xs.max() <= 9 and (layers["signed"] or layers["front"] is not None or xs.min() >= 0)
    bound = pm.abs_sum_bound(layers, xs)
    print(f"{name} {which}: {len(xs)} rows, abs-sum bound {bound:.0f} (x 2^-{pm.frac_bits(layers)})")
    assert bound < 2 ** 24
    ref = pm.int_ref(layers, xs)
    assert ref.dtype == (np.float64 if (layers["front"] is not None or layers["tail"] is not None
                                        or layers["act"] == "LeakyRelu") else np.int64)
    g = onnx_ref.load(data)
    y64 = onnx_ref.act(g, xs.astype(np.float64), np.float64)
    y32 = onnx_ref.act(g, xs, np.float32)
    assert y64.dtype == np.float64 and y32.dtype == np.float32
    assert np.array_equal(y64, ref)
    assert np.array_equal(y32, ref)
    assert pm.unobserved(layers, xs) == []
    if layers["tail"] is not None:
        lo, hi, k = layers["tail"]
        assert (ref == lo * k).any() and (ref == hi * k).any() and ((ref > lo * k) & (ref < hi * k)).any()
    if layers["act"] in ("Relu", "LeakyRelu", "Clip"):
        z = np.concatenate([np.ravel(z) for z, _ in pm._int_forward(layers, xs)[:-1]])
        if layers["signed"]:
            assert (z < 0).any() and (z > 0).any()   # both branches of the activation are taken


def test_unobserved_reports_a_dead_unit():
    """The sensitivity measure sees what it is for: a hidden unit no later layer reads, an
    observation column no row reads, and a unit that Relu keeps at zero."""
    for act, signed in (("Relu", True), ("Elu", False)):
        _, layers = pm.int_policy((6, 16, 8, 3), act, signed)
        xs = np.concatenate(pm.int_inputs(layers, [8, 5]))
        assert pm.unobserved(layers, xs) == []
        layers["dense"][1]["W"][:, 5] = 0
        layers["dense"][0]["W"][:, 2] = 0
        assert pm.unobserved(layers, xs) == [(-1, 2), (0, 5)]
    _, layers = pm.int_policy((6, 16, 8, 3), "Relu", True)
    layers["dense"][1]["W"][3] = -np.abs(layers["dense"][1]["W"][3])
    layers["dense"][1]["b"][3] = -1
    # (and with it the layer-0 units that only unit 3 reads)
    assert (1, 3) in pm.unobserved(layers, np.concatenate(pm.int_inputs(layers, [8, 5])))


def _inspect(tmp_path, data):
    from go2_onnx_controller_amd import engine
    p = tmp_path / "probe.onnx"
    p.write_bytes(data)
    return engine.inspect_model(str(p))


INF = 1e308   # inspect_model prints an infinite bound so


@pytest.mark.parametrize("name", list(pm.INT_PROBES))
def test_int_probe_loader_view(tmp_path, name):
    data, layers = pm.int_probe(name)
    info = _inspect(tmp_path, data)
    want = pm.int_expected_layers(layers)
    assert info["in_dim"] == layers["dims"][0] and info["out_dim"] == layers["dims"][-1]
    assert len(info["layers"]) == len(want)
    for got, (K, N, act, alpha, beta), d in zip(info["layers"], want, layers["dense"]):
        assert (got["K"], got["N"], got["act"], got["alpha"], got["beta"], got["ln"]) == (K, N, act, alpha, beta, 0)
        assert got["w_sum"] == d["W"].sum() and got["b_sum"] == d["b"].sum()
    front, tail = layers["front"] is not None, layers["tail"] is not None
    assert (info["pre_sub"], info["pre_div"], info["pre_mul"]) == ((layers["dims"][0], 0, 1) if front else (0, 0, 0))
    assert info["pre_clip"] == [-INF, INF] and info["clip"] == [-INF, INF]
    assert info["post_scale"] == (0.25 if tail else 1.0)
    assert info["gru"] is None


ACT_CASES = [(oid, shape, where) for oid, _, _ in pm.ACT_OPS for shape in ("h64", "h128", "h256x2")
             for where in ("hidden", "head")] + [("elu", "h128x3", "hidden")]
_OPS = {oid: (op, attrs) for oid, op, attrs in pm.ACT_OPS}


@pytest.mark.parametrize("oid,shape,where", ACT_CASES)
def test_act_probe_reference_and_loader(tmp_path, oid, shape, where):
    from oracle import onnx_ref
    op, attrs = _OPS[oid]
    in_dim, hidden, out_dim = pm.ACT_SHAPES[shape]
    d = len(hidden) if where == "hidden" else 1
    data = pm.act_policy(in_dim, hidden, out_dim, op, attrs, where)
    points = pm.act_points(op, attrs)
    assert np.isfinite(points).all() and (np.abs(points[points != 0]) >= 2.0 ** -126).all() and (np.abs(points) < 2.0 ** 126).all()
    x, pts = pm.act_inputs(points, in_dim, out_dim)
    ref = pm.act_ref(op, attrs, pts, d)
    g = onnx_ref.load(data)
    with np.errstate(all="ignore"):
        y64 = onnx_ref.act(g, x.astype(np.float64), np.float64)
        y32 = onnx_ref.act(g, x, np.float32)
    assert not np.isnan(y64).any() and not np.isnan(y32).any()
    assert (np.abs(y64 - ref) <= 1e-15 * np.abs(ref)).all()
    err = np.abs(y32.astype(np.float64) - ref) / (2.0 ** -23 * pm.act_unit(op, attrs, d) * np.maximum(1.0, np.abs(ref)))
    print(f"{oid} {shape} {where}: float32 oracle worst {err.max():.2f} ulp")
    assert (np.abs(y32.astype(np.float64) - ref) <= pm.act_bound(op, attrs, ref, d)).all()
    # the loader's view
    info = _inspect(tmp_path, data)
    al, be = pm.act_attrs(op, attrs)
    nl = len(hidden) + 1
    assert [(L["K"], L["N"]) for L in info["layers"]] == list(zip((in_dim,) + tuple(hidden), tuple(hidden) + (out_dim,)))
    for l, L in enumerate(info["layers"]):
        has = (l < nl - 1) if where == "hidden" else (l == nl - 1)
        assert (L["act"], L["alpha"], L["beta"]) == ((pm.ACT_CODE[op], al, be) if has else (0, 0.0, 0.0))
        assert L["b_sum"] == 0 and L["w_sum"] == min(L["K"], L["N"])
    assert info["pre_clip"] == [-INF, INF] and info["clip"] == [-INF, INF] and info["post_scale"] == 1.0


@pytest.mark.parametrize("oid", [oid for oid, _, _ in pm.ACT_OPS])
def test_overflow_rows_reference(oid):
    """The overflow rows' reference against the oracle's float32 evaluation of the same graph:
    the same NaN pattern and the same infinities (both follow IEEE 754 through the head)."""
    from oracle import onnx_ref
    op, attrs = _OPS[oid]
    in_dim, hidden, out_dim = pm.ACT_SHAPES["h64"]
    x, ref = pm.overflow_case(op, attrs, in_dim, hidden[0], out_dim)
    g = onnx_ref.load(pm.act_policy(in_dim, hidden, out_dim, op, attrs, "hidden", diag=2.0))
    with np.errstate(all="ignore"):
        y = onnx_ref.act(g, x, np.float32)
        assert np.isinf(np.float32(2.0) * x).sum() == pm.OVERFLOW_ROWS
    assert np.array_equal(np.isnan(y), np.isnan(ref))
    assert np.array_equal(np.isinf(y), np.isinf(ref)) and np.array_equal(y[np.isinf(ref)], ref[np.isinf(ref)])
    fin = np.isfinite(ref)
    assert (np.abs(y[fin].astype(np.float64) - ref[fin]) <= pm.act_bound(op, attrs, ref[fin].astype(np.float64))).all()
