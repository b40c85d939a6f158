"""GPU: every activation, element by element, on every kernel form.

An activation probe (tests/probe_models.py act_policy) is identity layers around one
activation: output j of a row is act(x[j]), composed d times where d hidden layers carry
it, so each epilogue site is seen per element at points a random network never reaches:
+-0, tiny |x| (Elu's exp2(x log2 e) - 1 cancellation, the lean kernel's integer-min
select), the Clip and HardSigmoid corners, saturation (|x| = 20 ... 1e30), the exp2
overflow side of Sigmoid / Softplus, and +-inf (the overflow rows). Each form takes the
smallest policy it accepts; `where` puts the activation after the hidden layers or after
the head (on the pipeline: policy_mlp_seq_kernel).

Bound: |y - ref| <= 4 * 2^-23 * s * L_d * max(1, |ref|) (probe_models.act_bound: from the
documented ~1 ulp of v_exp_f32 / v_rcp_f32 / v_log_f32 and two roundings, not from these
kernels). Exact, with no tolerance: Relu everywhere; LeakyRelu for x >= 0; Clip (x inside
its bounds, the bound outside); Elu for x >= 2^-10 returns x on every form. Below 2^-10
the lean kernel's Elu (fused_impl.hpp w4_epi_elu1) selects by a signed-integer min of x
and exp2(x log2 e) - 1, which for tiny positive x can return the rounded e - 1 (within
one ulp of 1) instead of x: there the bound alone holds. +-0 gives a value inside the
bound and never a NaN. Overflow rows (hidden placement, d = 1): the NaN pattern and the
infinities of the IEEE reference, finite values inside the bound.

Measured worst error on an MI355X, in units of 2^-23 * s * L_d * max(1, |ref|) (the bound
is 4), hidden / head placement:

                  generic      pipeline  pipeline_elu        launch         chain          act1            r1         multi          wide
elu           0.29 / 0.29   0.29 / 0.29          0.15   0.29 / 0.29   0.29 / 0.29   0.29 / 0.29   0.29 / 0.29   0.29 / 0.29   0.23 / 0.29
elu_a07       0.30 / 0.30   0.30 / 0.30             -   0.30 / 0.30   0.30 / 0.30   0.30 / 0.30   0.30 / 0.30   0.30 / 0.30   0.16 / 0.30
relu          0.00 / 0.00   0.00 / 0.00             -   0.00 / 0.00   0.00 / 0.00   0.00 / 0.00   0.00 / 0.00   0.00 / 0.00   0.00 / 0.00
tanh          0.23 / 0.23   0.23 / 0.23             -   0.23 / 0.23   0.23 / 0.23   0.23 / 0.23   0.23 / 0.23   0.23 / 0.23   0.10 / 0.23
sigmoid       0.43 / 0.43   0.43 / 0.43             -   0.43 / 0.43   0.43 / 0.43   0.43 / 0.43   0.43 / 0.43   0.43 / 0.43   0.27 / 0.43
leaky         0.41 / 0.41   0.41 / 0.41             -   0.41 / 0.41   0.41 / 0.41   0.41 / 0.41   0.41 / 0.41   0.41 / 0.41   0.12 / 0.41
clip          0.00 / 0.00   0.00 / 0.00             -   0.00 / 0.00   0.00 / 0.00   0.00 / 0.00   0.00 / 0.00   0.00 / 0.00   0.00 / 0.00
selu          0.29 / 0.29   0.29 / 0.29             -   0.29 / 0.29   0.29 / 0.29   0.29 / 0.29   0.29 / 0.29   0.29 / 0.29   0.19 / 0.29
selu_attrs    0.59 / 0.59   0.59 / 0.59             -   0.59 / 0.59   0.59 / 0.59   0.59 / 0.59   0.59 / 0.59   0.59 / 0.59   0.38 / 0.59
softplus      0.66 / 0.66   0.66 / 0.66             -   0.66 / 0.66   0.66 / 0.66   0.66 / 0.66   0.66 / 0.66   0.66 / 0.66   0.47 / 0.66
hardsigmoid   0.25 / 0.25   0.25 / 0.25             -   0.25 / 0.25   0.25 / 0.25   0.25 / 0.25   0.25 / 0.25   0.25 / 0.25   0.13 / 0.25
hardswish     0.40 / 0.40   0.40 / 0.40             -   0.40 / 0.40   0.40 / 0.40   0.40 / 0.40   0.40 / 0.40   0.40 / 0.40   0.16 / 0.40
softsign      0.67 / 0.67   0.67 / 0.67             -   0.67 / 0.67   0.67 / 0.67   0.67 / 0.67   0.67 / 0.67   0.67 / 0.67   0.22 / 0.67

(pipeline_elu: the compile-time Elu of the lean kernel, d = 3, hidden placement only. The cells
of the d = 1 forms agree because every epilogue site applies device_fn.hpp act_t to the same
float32 pre-activation; the wide form's hidden cells are in units of L_2.)

Out of scope (probe_models.py says why): recurrent cells, controller ticks,
LayerNormalization epilogues, multi-GPU, timing."""
import numpy as np
import pytest

import probe_models as pm

pytestmark = pytest.mark.gpu

LAT, CHAIN = "policy_latency_kernel", "gemv_layer_kernel graph"
GEN8 = "policy_fused_kernel<8, 0, 0, 0, 0, -1, 0>"

# form -> (policy, engine options, environment switch, batches,
#          (batched | small | resident kernel) for the hidden placement, ... for the head placement)
FORMS = {
    "generic": ("h64", dict(max_batch=64, small_batch=-1, waves=8), None, [17], ("batched", GEN8), ("batched", GEN8)),
    "pipeline": ("h128", dict(max_batch=64, small_batch=-1), "GO2PI_LEAN_RT_ACT", [17],
                 ("batched", "policy_mlp_kernel<2, 1, 3, -1, 0, 4>"), ("batched", "policy_mlp_seq_kernel<2, 1, 3, -1, 0, 4>")),
    "pipeline_elu": ("h128x3", dict(max_batch=64, small_batch=-1), None, [17],
                     ("batched", "policy_mlp_kernel<2, 1, 3, 1, 3, 4>"), None),
    "launch": ("h64", dict(max_batch=8, resident_ms=0), None, [8, 1], ("small", LAT), ("small", LAT)),
    "chain": ("h64", dict(max_batch=8, resident_ms=0), "GO2PI_SMALL_CHAIN", [8], ("small", CHAIN), ("small", CHAIN)),
    "act1": ("h64", dict(max_batch=8, resident_ms=100), None, [8, 1],
             ("resident", "policy_act1_kernel"), ("resident", "policy_act1_kernel")),
    "r1": ("h64", dict(max_batch=8, resident_ms=100), "GO2PI_RES_R1W", [8],
           ("resident", "policy_resident1_kernel"), ("resident", "policy_resident1_kernel")),
    "multi": ("h64", dict(max_batch=8, resident_ms=100), "GO2PI_RES_MULTI", [8],
              ("resident", "policy_resident_kernel"), ("resident", "policy_resident_kernel")),
    "wide": ("h256x2", dict(max_batch=8, resident_ms=100), None, [8, 1],
             ("resident", "policy_wide_kernel<3, 4, 16, 1>"), ("resident", "policy_wide_kernel<3, 4, 16, 1>")),
}
CASES = [(f, oid) for f in FORMS for oid, _, _ in pm.ACT_OPS if f != "pipeline_elu" or oid == "elu"]
_OPS = {oid: (op, attrs) for oid, op, attrs in pm.ACT_OPS}


def _engine(data, form, monkeypatch):
    from go2_onnx_controller_amd import Engine
    _, opts, env, _, _, _ = FORMS[form]
    if env:
        monkeypatch.setenv(env, "1")   # read when the engine is created
    return Engine(data, **opts)


def _check_kernel(e, want):
    which, name = want
    got = {"batched": e.batched_kernel, "small": e.small_kernel, "resident": e.resident_kernel}[which]
    kern, _, ring = got.partition(" ring=")
    if which == "resident" and ring == "host" and name.startswith("policy_wide_kernel"):
        name = "policy_resident_kernel"   # no large BAR: the multi-workgroup kernel serves wide policies
    assert kern == name, (which, got)
    if which != "resident":
        assert e.resident_kernel == "none"
        if which == "batched":
            assert e.small_kernel == got


@pytest.mark.parametrize("form,oid", CASES)
def test_activation_per_element(form, oid, monkeypatch):
    op, attrs = _OPS[oid]
    shape, _, _, batches, want_hidden, want_head = FORMS[form]
    in_dim, hidden, out_dim = pm.ACT_SHAPES[shape]
    points = pm.act_points(op, attrs)
    x, pts = pm.act_inputs(points, in_dim, out_dim, rows=batches[0])
    assert len(x) >= -(-len(points) // out_dim)   # the first request holds every point
    worst = {}
    for where, want in (("hidden", want_hidden), ("head", want_head)):
        if want is None:
            continue
        d = len(hidden) if where == "hidden" else 1
        ref = pm.act_ref(op, attrs, pts, d)
        with _engine(pm.act_policy(in_dim, hidden, out_dim, op, attrs, where), form, monkeypatch) as e:
            _check_kernel(e, want)
            ys = [(pm.run_checked(e, x[:B] if i == 0 else x[3:3 + B]), pts[:B] if i == 0 else pts[3:3 + B],
                   ref[:B] if i == 0 else ref[3:3 + B]) for i, B in enumerate(batches)]
            launches = e.resident_launches
        assert launches == (1 if want[0] == "resident" else 0)
        for y, p, r in ys:
            assert not np.isnan(y).any()
            err = np.abs(y.astype(np.float64) - r)
            unit = 2.0 ** -23 * pm.act_unit(op, attrs, d) * np.maximum(1.0, np.abs(r))
            worst[where] = max(worst.get(where, 0.0), float((err / unit).max()))
            print(f"ACTERR {form} {oid} {where} d={d} B={len(y)}: worst {float((err / unit).max()):.3f} ulp "
                  f"at x={p.ravel()[np.argmax(err / unit)]!r}")
            assert (err <= pm.act_bound(op, attrs, r, d)).all(), (where, float((err / unit).max()))
            # the exact branches
            if op in ("Relu", "Clip"):
                assert np.array_equal(y, r)
            if op == "LeakyRelu":
                assert np.array_equal(y[p >= 0], p[p >= 0])
            if op == "Elu":
                assert np.array_equal(y[p >= 2.0 ** -10], p[p >= 2.0 ** -10])
    # the overflow rows: a pre-activation of +-inf (hidden placement, one hidden layer)
    if len(hidden) == 1:
        xo, ro = pm.overflow_case(op, attrs, in_dim, hidden[0], out_dim)
        with _engine(pm.act_policy(in_dim, hidden, out_dim, op, attrs, "hidden", diag=2.0), form, monkeypatch) as e:
            _check_kernel(e, want_hidden)
            yo = pm.run_checked(e, xo)
        print(f"ACTOVF {form} {oid}: nan {np.array_equal(np.isnan(yo), np.isnan(ro))} "
              f"inf {np.array_equal(np.isinf(yo), np.isinf(ro))}")
        assert np.array_equal(np.isnan(yo), np.isnan(ro)), (yo, ro)
        inf = np.isinf(ro)
        assert np.array_equal(np.isinf(yo), inf) and np.array_equal(yo[inf], ro[inf]), (yo, ro)
        fin = np.isfinite(ro)
        assert (np.abs(yo[fin].astype(np.float64) - ro[fin]) <= pm.act_bound(op, attrs, ro[fin].astype(np.float64))).all()
    print(f"ACTCELL {form} {oid} " + " / ".join(f"{worst[w]:.2f}" for w in ("hidden", "head") if w in worst))
