"""GPU: integer probe policies (tests/probe_models.py) on every kernel form, bit for bit.

Every probe's answer is an exact integer (or dyadic fraction) in float32 whatever the
summation order (tests/test_cpu_probe.py checks abs_sum_bound < 2^24, that the oracle
agrees bit for bit and that no observation column or hidden unit goes unobserved), so
each form must return `np.array_equal(y, int_ref)` for every request of its schedule: no
tolerance that a dropped term, a stale row or an unswept row could hide in. The shapes
sit on either side of the edges of the kernel-selection predicates (plan.cpp latency_shape
/ one_round / done_ok, kernels.hip latency_grid, resident.hip act1_shape /
resident_r1_fits, resident_wide.hip wide_shape, plan.cpp w4_eligible / k0q / head
fusion); the tables below name the kernel each engine must report, and a resident engine
must have served its whole schedule from one launch (a form that gives up on every
request and is relaunched would otherwise pass).

Out of scope (probe_models.py says why): recurrent cells, controller ticks,
LayerNormalization, multi-GPU, timing."""
import numpy as np
import pytest

import probe_models as pm

pytestmark = pytest.mark.gpu

LAT, CHAIN = "policy_latency_kernel", "gemv_layer_kernel graph"
ACT1, R1, MULTI = "policy_act1_kernel", "policy_resident1_kernel", "policy_resident_kernel"
REFUSED = "refused"

# probe -> (what serves one launch per call, the default resident kernel, the resident kernel
# under GO2PI_RES_R1W=1 where that differs); REFUSED: no engine (see test_width_limit)
SMALL = {
    # layer 1's K_pad 1024: two sweep rounds (the general instantiations), the last size inside
    "33_1024_12": (LAT, MULTI, None),
    # K_pad 1088: past the single launch's register slots
    "33_1040_12": (CHAIN, "none", None),
    # one_round on either side (K_pad 512 / 576 behind layer 0)
    "20_512_40_9": (LAT, MULTI, None),
    "20_513_40_9": (LAT, MULTI, None),
    # latency_grid 256 / 257 cannot be reached: see test_width_limit
    "16_4096_8": REFUSED,
    "16_4112_8": REFUSED,
    # done_ok on either side (a head of one tile / two)
    "24_64_16": (LAT, ACT1, R1),
    "24_64_17": (LAT, "none", None),
    # in_dim around the float4 and 64 edges
    "1_64_3": (LAT, ACT1, R1),
    "3_64_3": (LAT, ACT1, R1),
    "63_128x2_12": (LAT, ACT1, R1),
    "64_128x2_12": (LAT, ACT1, R1),
    "65_128x2_12": (LAT, ACT1, R1),
    # act1's corners: (NL 2, F0 1), the shipped shape, (NL 4, F0 4, lds_stride 260)
    "48_64_12": (LAT, ACT1, R1),
    "98_128x2_12": (LAT, ACT1, R1),
    "98_128x2_12_ft": (LAT, ACT1, R1),
    "200_64x3_12": (LAT, ACT1, R1),
    # F0 3 -> 4 with lds_stride 196 < 256, and H 128 with NL 4, F0 4: not act1, and past
    # resident_r1_fits' four weight float4s per lane (layer 0's K_pad 192 / 256 over 8 lanes
    # per output): the multi-workgroup kernel
    "150_128x2_12": (LAT, MULTI, None),
    "200_128x3_12": (LAT, MULTI, None),
    # non-uniform widths
    "17_100_200_33_5": (LAT, MULTI, None),
    # the four wide instantiations (and PRO = 1 of the BASELINE shape)
    "48_512x3_12": (LAT, "policy_wide_kernel<4, 8, 12, 0>", None),
    "48_512x3_12_ft": (LAT, "policy_wide_kernel<4, 8, 12, 1>", None),
    "63_512x2_16": (LAT, "policy_wide_kernel<3, 8, 16, 1>", None),
    "17_256x2_1": (LAT, "policy_wide_kernel<3, 4, 16, 1>", None),
    "60_256x3_12": (LAT, "policy_wide_kernel<4, 4, 16, 1>", None),
}
REQ_HOST = ["98_128x2_12", "48_512x3_12"]   # the request ring in host memory: one act1 and one wide probe

# probe -> {waves option: batched kernel}; 0: the default (the 4-wave pipeline where it applies)
GEN = {4: "policy_fused_kernel<4, 0, 0, 0, 0, -1, 0>", 8: "policy_fused_kernel<8, 0, 0, 0, 0, -1, 0>",
       16: "policy_fused_kernel<16, 0, 0, 0, 0, -1, 0>"}
BATCHED = {
    "17_100_200_33_5": GEN,        # N not a multiple of 16, a 3-tile head (no head fusion)
    "30_96_160_64_200_9": GEN,     # a long chain
    "40_64_20": GEN,               # a 2-tile head fused behind a 4-tile layer at 4 waves only
    "48_128_12_relu": {0: "policy_mlp_kernel<2, 1, 3, -1, 0, 4>"},
    "64_128x2_20": {0: "policy_mlp_kernel<2, 2, 0, 1, 0, 4>"},
    "33_256x3_12": {0: "policy_mlp_kernel<4, 1, 3, 1, 3, 4>"},
    "100_256x2_32": {0: "policy_mlp_kernel<4, 2, 3, -1, 0, 4>"},
    "48_512x3_12": {0: "policy_mlp_kernel<8, 1, 3, 1, 3, 4>", 8: GEN[8]},
    "48_512x3_12_relu": {0: "policy_mlp_kernel<8, 1, 3, -1, 0, 4>"},
    "70_512_16": {0: "policy_mlp_kernel<8, 1, 0, 1, 0, 4>"},
    "48_512x4_12": {0: "policy_mlp_kernel<8, 1, 3, 1, 0, 4>"},
    # with a front-end and a tail: the pipeline's general body
    "98_128x2_12_ft": {0: "policy_fused_kernel<4, 2, 1, 3, 0, -1, 0>"},
    "48_512x3_12_ft": {0: "policy_fused_kernel<4, 8, 1, 3, 0, 1, 3>"},
}

_cases = {}


def _case(name, which):
    """(onnx bytes, requests, exact answers) of a probe and schedule, computed once."""
    if (name, which) not in _cases:
        data, layers = pm.int_probe(name)
        xs = pm.int_inputs(layers, pm.SMALL_SCHEDULE if which == "small" else pm.BATCH_SCHEDULE)
        _cases[(name, which)] = (data, xs, [pm.int_ref(layers, x) for x in xs])
    return _cases[(name, which)]


def _small_forms():
    out = []
    for name, exp in SMALL.items():
        if exp == REFUSED:
            continue
        out += [(name, f) for f in ("launch", "resident", "multi", "chain")]
        if exp[2] is not None:
            out.append((name, "r1w"))
        if name in REQ_HOST:
            out.append((name, "req_host"))
    return out


def _small_engine(data, form, monkeypatch):
    from go2_onnx_controller_amd import Engine
    env = {"multi": "GO2PI_RES_MULTI", "r1w": "GO2PI_RES_R1W", "chain": "GO2PI_SMALL_CHAIN", "req_host": "GO2PI_REQ_HOST"}
    if form in env:
        monkeypatch.setenv(env[form], "1")   # read when the engine is created
    return Engine(data, max_batch=8, resident_ms=0 if form in ("launch", "chain") else 100)


def _small_expected(name, form):
    """(small_kernel, resident_kernel without its ring, ring or None: either)."""
    small, res, r1w = SMALL[name]
    if form == "chain":
        return CHAIN, "none", None
    if form == "launch" or res == "none":
        return small, "none", None
    if form == "multi":
        return small, MULTI, None
    if form == "r1w":
        return small, r1w, None
    if form == "req_host":   # no ring in device memory: the wide kernel's workgroups could not poll it
        return small, (MULTI if res.startswith("policy_wide_kernel") else res), "host"
    return small, res, None


def _run_all(e, xs, refs):
    bad = []
    for i, (x, ref) in enumerate(zip(xs, refs)):
        y = pm.run_checked(e, x)
        if not (y.shape == ref.shape and np.array_equal(y, ref)):
            bad.append((i, len(x), int((y != ref).sum())))
    return bad


@pytest.mark.parametrize("name,form", _small_forms())
def test_small_forms_bitwise(name, form, monkeypatch):
    """B = 8, 1, 5, 7, 4, 8 on one engine (a smaller request meets the stale rows of a larger
    one): every answer equals the exact reference, the engine reports the kernel the table
    names, and a resident engine served all six requests from one launch."""
    data, xs, refs = _case(name, "small")
    want_small, want_res, want_ring = _small_expected(name, form)
    with _small_engine(data, form, monkeypatch) as e:
        small, res = e.small_kernel, e.resident_kernel
        bad = _run_all(e, xs, refs)
        launches = e.resident_launches
    print(f"PROBE small {name} {form}: small={small!r} resident={res!r} launches={launches} bad={bad}")
    assert not bad, f"(request, rows, differing outputs): {bad}"
    kern, _, ring = res.partition(" ring=")
    if ring == "host" and want_res.startswith("policy_wide_kernel"):
        want_res = MULTI   # no large BAR: the multi-workgroup kernel serves wide policies
    assert (small, kern) == (want_small, want_res)
    assert want_ring is None or ring == want_ring
    assert launches == (0 if want_res == "none" else 1)


@pytest.mark.parametrize("name", [n for n, exp in SMALL.items() if exp == REFUSED])
def test_width_limit(name):
    """latency_grid's 256-workgroup edge (a 4096- against a 4112-wide layer) is out of reach:
    the batched kernel's two activation buffers of 16 rows pass 160 KiB of LDS from about
    1200 columns on, and the engine refuses such a policy when it is created, with a
    message, before any small-batch kernel is chosen."""
    from go2_onnx_controller_amd import Engine
    from go2_onnx_controller_amd.engine import Go2piError
    with pytest.raises(Go2piError, match="LDS") as info:
        Engine(pm.int_probe(name)[0], max_batch=8)
    assert info.value.code == -2


@pytest.mark.parametrize("name,waves", [(n, w) for n, t in BATCHED.items() for w in t])
def test_batched_forms_bitwise(name, waves):
    """B = 33, 1, 16, 17, 15 on the batched kernel alone (small_batch = -1): exact answers,
    and the kernel instantiation the table names."""
    from go2_onnx_controller_amd import Engine
    data, xs, refs = _case(name, "batched")
    with Engine(data, max_batch=64, small_batch=-1, waves=waves) as e:
        kern, small, res = e.batched_kernel, e.small_kernel, e.resident_kernel
        bad = _run_all(e, xs, refs)
    print(f"PROBE batched {name} waves={waves}: batched={kern!r} small={small!r} resident={res!r} bad={bad}")
    assert not bad, f"(request, rows, differing outputs): {bad}"
    assert (kern, small, res) == (BATCHED[name][waves], BATCHED[name][waves], "none")


def test_forms_agree_bitwise(monkeypatch):
    """Everything is exact, so the forms agree with each other bit for bit, not only with the
    reference: the BASELINE shape's first request on the single launch, the wide resident
    kernel, the multi-workgroup kernel, the GEMV chain, the pipeline and the generic body."""
    from go2_onnx_controller_amd import Engine
    data, xs, refs = _case("48_512x3_12", "small")
    ys = {}
    for form in ("launch", "resident", "multi", "chain"):
        with monkeypatch.context() as mp, _small_engine(data, form, mp) as e:
            ys[form] = pm.run_checked(e, xs[0])
    for waves in (0, 8):
        with Engine(data, max_batch=64, small_batch=-1, waves=waves) as e:
            ys[f"batched waves={waves}"] = pm.run_checked(e, xs[0])
    first = ys["launch"]
    assert np.array_equal(first, refs[0])
    for form, y in ys.items():
        assert y.tobytes() == first.tobytes(), form
