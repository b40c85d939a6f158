"""GPU: the resident wide-policy kernel (resident_wide.hip policy_wide_kernel) against the
fp64 ONNX oracle on graphs that use what the synthetic wide models leave at identity:
an observation front-end (per-feature, scalar-broadcast and Constant-node constants), a
different activation or different attributes on every layer, and an output tail that binds
(tests/graphs.py WIDE_VARIANTS; test_cpu_boundary.py::test_wide_graph_inputs_bind checks
on the CPU that the clips bind on these inputs and that float32 arithmetic is good for the
bound). Also: the exact instantiation that ran, one launch for a run of requests, NaN rows,
the same graphs on the other batch <= 8 forms and on the batched kernel, and the edges of
the selection predicate (wide_shape).

Bound: |y - oracle| <= 1e-5 absolute, the project's contract (outputs are O(1))."""
import numpy as np
import pytest

import graphs
from conftest import abs_err

pytestmark = pytest.mark.gpu

TOL = 1e-5

# the instantiation launch_resident_wide runs for each graph: <NL, CW, F0, PRO>
WIDE_KERNEL = {"wide_pro_512_4": "policy_wide_kernel<4, 8, 12, 1>", "wide_pro_512_3": "policy_wide_kernel<3, 8, 16, 1>",
               "wide_pro_256_3": "policy_wide_kernel<3, 4, 16, 1>", "wide_pro_256_4": "policy_wide_kernel<4, 4, 16, 1>"}

_cache = {}


def _case(tmp_path_factory, kind, schedule=None, seed=0):
    """(model path, requests, fp64 oracle answers) of a graph, computed once per module."""
    from oracle import onnx_ref
    key = (kind, tuple(schedule or ()), seed)
    if key not in _cache:
        if kind not in _cache:
            p = graphs.write(tmp_path_factory.mktemp(kind), kind)
            _cache[kind] = (p, onnx_ref.load(p))
        p, g = _cache[kind]
        xs = graphs.wide_inputs(kind, schedule, seed)
        _cache[key] = (p, xs, [onnx_ref.act(g, x.astype(np.float64)) for x in xs])
    return _cache[key]


def _serve(e, xs, wants):
    """Every request through e.run, twice: (|y - oracle| per request, the requests whose
    second answer differed in any bit)."""
    errs, unstable = [], []
    for i, (x, want) in enumerate(zip(xs, wants)):
        y = e.run(x)
        assert y.shape == want.shape
        errs.append(abs_err(y, want))
        if not np.array_equal(y, e.run(x)):
            unstable.append(i)
    return errs, unstable


@pytest.mark.parametrize("kind", graphs.WIDE_VARIANTS)
def test_wide_graphs_against_oracle(tmp_path_factory, kind):
    """One resident engine serves graphs.WIDE_SCHEDULE (B = 1 after B = 8 meets stale rows in
    the kernel's x0 / h0 / hh; B = 1 takes the per-lane prologue constants, B >= 2 the sweep
    path): every answer within 1e-5 of the fp64 oracle and the same bits when asked again;
    then one launch served all of it, and the kernel is the instantiation expected (with a
    front-end that is not the identity, per-layer activation parameters that differ and a
    tail that clips: a kernel that used layer 0's parameters elsewhere, skipped a prologue
    op or the tail fails the parity). Without large BAR the multi-workgroup kernel serves:
    the parity holds, the name and launch-count part is skipped.
    Measured on an MI355X (large BAR), worst |y - oracle|: 9.1e-8 wide_pro_512_4, 3.2e-7
    wide_pro_512_3, 1.0e-6 wide_pro_256_3 (one output, up to |4|), 2.7e-7 wide_pro_256_4;
    the float32 oracle on the same inputs: 2.3e-7, 5.3e-7, 9.8e-7, 6.5e-7."""
    from go2_onnx_controller_amd import Engine
    p, xs, wants = _case(tmp_path_factory, kind)
    with Engine(p, max_batch=8, resident_ms=5000) as e:
        name = e.resident_kernel
        errs, unstable = _serve(e, xs, wants)
        launches = e.resident_launches
    print(f"{kind}: {name}, worst |y - oracle| {max(errs):.3e}, {launches} launch(es) for {2 * len(xs)} requests")
    assert max(errs) <= TOL, [f"{v:.2e}" for v in errs]
    assert not unstable, f"requests {unstable}: the answer changed when asked again"
    if name.endswith(" ring=host"):
        assert name == "policy_resident_kernel ring=host"
        pytest.skip("no large BAR: the multi-workgroup kernel serves wide policies here")
    assert launches == 1
    assert name == WIDE_KERNEL[kind] + " ring=vram"


@pytest.mark.parametrize("kind", graphs.WIDE_NAN_VARIANTS)
def test_wide_graphs_nan_rows(tmp_path_factory, kind):
    """A NaN in an observation row (row 2 column 5, row 7 column 0 at B = 8) passes through the
    front-end's Clip, every activation and the tail: those rows come out all NaN, as the
    oracle's do, the other rows stay within 1e-5, and the next clean request on the same live
    kernel is within 1e-5 everywhere (nothing stayed behind in LDS)."""
    from go2_onnx_controller_amd import Engine
    from oracle import onnx_ref
    p, xs, wants = _case(tmp_path_factory, kind, [8, 8], seed=3)
    x = xs[0].copy()
    x[2, 5] = np.nan
    x[7, 0] = np.nan
    want = onnx_ref.act(_cache[kind][1], x.astype(np.float64))
    assert np.isnan(want[[2, 7]]).all() and not np.isnan(np.delete(want, [2, 7], axis=0)).any()
    with Engine(p, max_batch=8, resident_ms=5000) as e:
        y = e.run(x)
        y_clean = e.run(xs[1])
        launches = e.resident_launches
    np.testing.assert_array_equal(np.isnan(y), np.isnan(want))
    ok = ~np.isnan(want)
    print(f"{kind}: clean rows {abs_err(y[ok], want[ok]):.3e}, next request {abs_err(y_clean, wants[1]):.3e}")
    assert abs_err(y[ok], want[ok]) <= TOL
    assert abs_err(y_clean, wants[1]) <= TOL
    assert launches == 1


@pytest.mark.parametrize("form", ["multi", "req_host", "launch", "batched"])
@pytest.mark.parametrize("kind", graphs.WIDE_VARIANTS)
def test_wide_graphs_other_forms(tmp_path_factory, kind, form, monkeypatch):
    """The same graphs on the other kernels: the multi-workgroup resident kernel
    (GO2PI_RES_MULTI=1), the request ring in host memory (GO2PI_REQ_HOST=1), one launch per
    call (resident_ms = 0) at B = 1 and 5, and the batched kernel at B = 300; each within
    1e-5 of the fp64 oracle (measured worst, wide_pro_256_3 each time: 1.0e-6 resident,
    8.5e-7 one launch per call, 1.5e-6 batched, where the float32 oracle is 1.5e-6 too)."""
    from go2_onnx_controller_amd import Engine
    if form in ("multi", "req_host"):
        monkeypatch.setenv("GO2PI_RES_MULTI" if form == "multi" else "GO2PI_REQ_HOST", "1")  # read at engine creation
        p, xs, wants = _case(tmp_path_factory, kind)
        xs, wants = xs[:9], wants[:9]
        kw = dict(max_batch=8, resident_ms=5000)
    elif form == "launch":
        p, xs, wants = _case(tmp_path_factory, kind, [1, 5], seed=1)
        kw = dict(max_batch=8, resident_ms=0)
    else:
        p, xs, wants = _case(tmp_path_factory, kind, [300], seed=2)
        kw = dict(max_batch=512, resident_ms=0)
    with Engine(p, **kw) as e:
        name = e.resident_kernel
        errs, unstable = _serve(e, xs, wants)
    print(f"{kind} {form}: {name}, worst |y - oracle| {max(errs):.3e}")
    if form == "multi":
        assert name.startswith("policy_resident_kernel"), name
    elif form == "req_host":
        assert name == "policy_resident_kernel ring=host"
    else:
        assert name == "none"
    assert max(errs) <= TOL, [f"{v:.2e}" for v in errs]
    assert not unstable


# one shape on each side of every edge of wide_shape (no front-end, Elu): the last shape
# inside runs the generic 3-layer 512-wide instantiation; in_dim 64, K_pad 64 under four
# layers of 512 (a 49-wide observation; a 48-wide one whose layers differ in Elu's alpha, so
# that the engine pads it to 64 columns) and five layers fall to the multi-workgroup kernel;
# a head that pads to 32 has no resident form (its answer is not one tile)
EDGE_KERNEL = {"wide_edge_in63_out16": "policy_wide_kernel<3, 8, 16, 1>", "wide_edge_in64": "policy_resident_kernel",
               "wide_edge_k49_512_4": "policy_resident_kernel", "wide_edge_out17": "none",
               "wide_edge_5_layers": "policy_resident_kernel", "wide_edge_mixed_512_4": "policy_resident_kernel"}


@pytest.mark.parametrize("kind", graphs.WIDE_EDGES)
def test_wide_selection_edges(tmp_path_factory, kind):
    """A predicate loosened past an edge would launch an instantiation whose registers
    cannot hold the shape: the kernel chosen on each side of each edge, by its exact name,
    and parity with the oracle over B = 1, 8, 3, 1 whichever kernel serves."""
    from go2_onnx_controller_amd import Engine
    p, xs, wants = _case(tmp_path_factory, kind, [1, 8, 3, 1], seed=4)
    with Engine(p, max_batch=8, resident_ms=5000) as e:
        name = e.resident_kernel
        errs, unstable = _serve(e, xs, wants)
    print(f"{kind}: {name}, worst |y - oracle| {max(errs):.3e}")
    assert max(errs) <= TOL, [f"{v:.2e}" for v in errs]
    assert not unstable
    want = EDGE_KERNEL[kind]
    if want == "none":
        assert name == "none"
    elif name.endswith(" ring=host"):
        assert name == "policy_resident_kernel ring=host"
        if want.startswith("policy_wide_kernel"):
            pytest.skip("no large BAR: the multi-workgroup kernel serves wide policies here")
    else:
        assert name == want + " ring=vram"


def test_wide_kernel_names(tmp_path_factory, synth_path):
    """go2pi_resident_kernel names the instantiation launch_resident_wide runs (one function
    decides both): only 48 -> 512^3 -> 12 without a prologue has a PRO = 0 build."""
    from go2_onnx_controller_amd import Engine
    cases = [(synth_path("go2_mlp_512"), "policy_wide_kernel<4, 8, 12, 0>"),
             (_case(tmp_path_factory, "wide_pro_512_4")[0], "policy_wide_kernel<4, 8, 12, 1>"),
             (synth_path("wide_512_3"), "policy_wide_kernel<3, 8, 16, 1>"),
             (synth_path("wide_256_3"), "policy_wide_kernel<3, 4, 16, 1>"),
             (synth_path("wide_256_4"), "policy_wide_kernel<4, 4, 16, 1>")]
    names = []
    for p, _ in cases:
        with Engine(p, max_batch=8, resident_ms=100) as e:
            names.append(e.resident_kernel)
    if all(n == "policy_resident_kernel ring=host" for n in names):
        pytest.skip("no large BAR: the multi-workgroup kernel serves wide policies here")
    assert names == [want + " ring=vram" for _, want in cases]
