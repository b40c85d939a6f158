"""CPU: the dynamic-LDS layout of every small-batch and resident kernel (csrc/lds_layout.hpp),
read through tests/cpp/plan_probe.cpp's "lds" object: no device is touched.

Kernel and launcher take a layout from the same function, so what can still go wrong is
the layout itself. For every form the plan uses, on the models the GPU tests run:
regions sorted, disjoint, inside the total and without a gap; 16-byte alignment of the
regions read as double or float4 or filled by direct-to-LDS loads; the CU's 160 KiB (64 KiB
for the wide kernel, whose launcher never raises the limit); and the byte count of the
launcher formula this layout replaced, restated here from the printed arguments alone, so
the allocation of every launch is what it was.
"""
import pytest

import graphs
import ln_small_models as lm
from conftest import SHIPPED
from test_cpu_plan import _write, plan

MAXB, WAVES, KIB = 8, 8, 1024
# regions read as double / float4 or written by direct-to-LDS loads (image.*: the controller
# inputs' image, q0 double; w0l / wol: float4 weights; xs, x0, hx: float4 input rows)
ALIGNED = {"image.q0", "image.st", "image.jy", "image.act", "image.obs", "w0l", "wol", "xs", "x0", "hx"}


def check_regions(regions, total_floats, aligned=ALIGNED):
    """Raises AssertionError unless the [name, offset, size] table (floats) is sorted,
    disjoint, gap-free, inside total_floats, and its `aligned` regions start on 16 bytes."""
    at = 0
    for name, off, size in regions:
        assert size >= 0, (name, size)
        assert off >= at, f"{name} at {off} overlaps the region before it (ends at {at})"
        assert off == at, f"unnamed gap of {off - at} floats in front of {name}"
        if name in aligned and size:
            assert off % 4 == 0, f"{name} at {off}: not 16-byte aligned"
        at = off + size
    assert at == total_floats, f"regions end at {at}, the total is {total_floats}"


# ---- the launchers' formulas as they stood before lds_layout.hpp (kernels.hip, resident.hip,
# resident_wide.hip), from the probe's arguments
def c64(x):
    return (x + 63) & ~63


def ctl_floats(in_dim):  # ctl_fn.hpp ctl_lds_floats(GO2PI_SMALL_MAXB, in_dim)
    return 64 + c64(MAXB * 36) + c64(MAXB * 5) + c64(MAXB * 12) + c64(MAXB * in_dim) + 16


def latency_bytes(a, ctl):  # launch_latency / launch_latency_ctl
    f = MAXB * a["lds_stride"] + WAVES * MAXB * 16 + 4
    if ctl:
        f += MAXB * a["in_dim"] + MAXB + ctl_floats(a["in_dim"])
    return 4 * f


def gemv_bytes(k_pad):  # gemv_lds_bytes
    return 4 * (MAXB * k_pad + WAVES * MAXB * 16)


def wide_bytes(a, f):  # wide_lds_bytes
    return 4 * (MAXB * (4 * f["f0"] + 2 * 64 * f["cw"] + 16 + 256) + 4)


def r1_bytes(a, f, ctl):  # resident1_lds_bytes
    n = 3 * MAXB * a["lds_stride"] + 4 + (MAXB * a["in_dim"] + 3) // 4 * 4
    if ctl:
        n += ctl_floats(a["in_dim"]) + MAXB * (53 + a["in_dim"])
    return 4 * n


def act1_bytes(a, f, ctl):  # launch_resident1's lds1
    w = f["f0"] * (f["h"] // 32) * 512 * 4 + (f["h"] // 64) * 256 * 4
    n = 3 * MAXB * a["lds_stride"] + 4
    if ctl:
        n += ctl_floats(a["in_dim"]) + w + MAXB * a["in_dim"]
    if not ctl and a["ln"] and f["h"] == 128 and f["nl"] == 4:
        n += w
    return 4 * n


def multi_bytes(a, f, ctl):  # launch_resident's ctl_off + tail
    n0, c0 = a["n0_pad"], a["k0_pad"] >> 4
    ks = 512 // n0 if n0 > 0 and 512 % n0 == 0 else 0
    nf = 4 * ((c0 + ks - 1) // ks) if ks > 0 else 0
    local0 = not a["rnn"] and a["nl"] >= 2 and nf in (8, 12, 16) and not f["tiled0"]
    assert f["nf"] == (nf if local0 else 0)
    x0len = (nf // 4) * ks * 16 if local0 else a["k0_pad"]
    ctl_off = (MAXB * a["lds_stride"] + WAVES * MAXB * 16 + 4 + MAXB * a["in_dim"] + MAXB * x0len +
               (ks if ks > 1 else 0) * MAXB * n0 + 3) // 4 * 4
    tail = 0
    if ctl:
        tail = ctl_floats(a["in_dim"]) + MAXB * (53 + a["in_dim"])
    if a["rnn"]:
        tail = MAXB * (a["i_pad"] + a["gru_h"]) + WAVES * 4 * MAXB * 16 + 2 * MAXB + 4 * MAXB * 16
    return 4 * (ctl_off + tail)


PARENT = {"act1": act1_bytes, "r1": r1_bytes, "multi": multi_bytes, "wide": lambda a, f, ctl: wide_bytes(a, f)}


def check_plan(got, forms, regions=()):
    """Every layout of one probe run; forms: the resident forms (act, ctl) it must hold;
    regions: names that must appear with a size > 0. Returns the forms seen."""
    a = got["lds"]
    seen, names = [], set()

    def one(lay, want_bytes, limit=160 * KIB):
        assert lay["total_bytes"] % 4 == 0
        check_regions(lay["regions"], lay["total_bytes"] // 4)
        assert lay["total_bytes"] <= limit
        assert lay["total_bytes"] == want_bytes
        names.update(n for n, _, s in lay["regions"] if s)

    assert len(a["gemv"]) == a["nl"]
    for lay in a["gemv"]:
        one(lay, gemv_bytes(lay["k_pad"]))
    if got["latency_ok"]:
        one(a["latency"], latency_bytes(a, False))
        one(a["latency_ctl"], latency_bytes(a, True))
    for key in ("act", "ctl"):
        if key in a:
            f = a[key]
            one(f, PARENT[f["form"]](a, f, key == "ctl"), 64 * KIB if f["form"] == "wide" else 160 * KIB)
            seen.append(f["form"])
        else:
            seen.append(None)
    assert tuple(seen) == tuple(forms), (seen, forms)
    assert set(regions) <= names, set(regions) - names
    return a


# ---- the cases
CTL_IMAGE = ("image.q0", "image.st", "image.jy", "image.act", "image.obs", "image.nanf")


@pytest.mark.parametrize("switches,forms,regions", [
    ((), ("act1", "act1"), CTL_IMAGE + ("w0l", "wol", "obsn", "okeep", "slack")),
    (("GO2PI_RES_R1W",), ("r1", "r1"), CTL_IMAGE + ("obsv", "craw")),
    (("GO2PI_RES_MULTI",), ("multi", "multi"), CTL_IMAGE + ("x0", "p0", "craw")),
    (("GO2PI_RES_MULTI", "GO2PI_RES_TILED0"), ("multi", "multi"), CTL_IMAGE + ("x0", "p0", "craw")),
], ids=["act1", "r1", "multi", "multi_tiled0"])
def test_shipped_model(switches, forms, regions):
    a = check_plan(plan(SHIPPED, *switches, resident_ms=100), forms, regions)
    if forms[0] == "multi":  # 98 -> 128: four slices of two chunks, unless tiled
        assert a["act"]["nf"] == a["ctl"]["nf"] == (0 if "GO2PI_RES_TILED0" in switches else 8)


WIDE = [("go2_mlp_512", 8, 12), ("wide_pro_512_4", 8, 12), ("wide_512_3", 8, 16), ("wide_256_3", 4, 16),
        ("wide_256_4", 4, 16)]  # test_gpu_resident_wide.py test_wide_kernel_names: the five instantiations


@pytest.mark.parametrize("name,cw,f0", WIDE)
def test_wide_shapes(synth_path, tmp_path, name, cw, f0):
    p = graphs.write(tmp_path, name) if name.startswith("wide_pro") else synth_path(name)
    a = check_plan(plan(p, resident_ms=100), ("wide", "multi"), ("pp", "st", "ho"))
    assert (a["act"]["cw"], a["act"]["f0"]) == (cw, f0)
    # without a large BAR the multi-workgroup kernel serves them (512 / 512: one slice, no partials)
    a = check_plan(plan(p, "ring=host", resident_ms=100), ("multi", "multi"))
    p0 = dict((n, s) for n, _, s in a["act"]["regions"])["p0"]
    assert a["act"]["nf"] in (8, 12, 16) and p0 == (0 if cw == 8 else 2 * 8 * 256)


@pytest.mark.parametrize("name", ["gru_128", "lstm_128", "go2_gru_256", "go2_lstm_256"])
def test_recurrent_cells(synth_path, name):
    a = check_plan(plan(synth_path(name), resident_ms=100), ("multi", None),
                   ("hx", "hpart", "le", "lb", "hown", "cown", "hst", "cst"))
    assert a["rnn"] == 1 and a["act"]["nf"] == 0


@pytest.mark.parametrize("name", lm.ALL_MODELS)
def test_ln_small_models(tmp_path, name):
    form = {"policy_act1_kernel": "act1", "policy_resident_kernel": "multi"}[lm.RESIDENT_FORM[name]]
    a = check_plan(plan(lm.model_path(name, tmp_path), ln_small=True, resident_ms=5000), (form, None))
    assert a["ln"] == 1
    if form == "act1":  # the weights in LDS for four layers of 128 only
        f = a["act"]
        sizes = dict((n, s) for n, _, s in f["regions"])
        in_lds = f["h"] == 128 and f["nl"] == 4
        assert (sizes["w0l"] > 0, sizes["wol"] > 0) == (in_lds, in_lds)
        assert in_lds == (name == "ln_ctl_post")


@pytest.mark.parametrize("name,hist,form", [("ctl_h1", 1, "act1"), ("ctl_h16", 16, "multi")])
def test_controller_histories(synth_path, name, hist, form):
    """test_gpu_controller.py's history models at the shortest and the longest history (the
    image's observation rows: 49 and 784 floats a robot)."""
    got = plan(synth_path(name), resident_ms=500)
    assert got["ctl_hist"] == hist
    a = check_plan(got, (form, form), CTL_IMAGE)
    assert a["in_dim"] == 49 * hist
    check_plan(plan(synth_path(name), "GO2PI_RES_MULTI", resident_ms=500), ("multi", "multi"), CTL_IMAGE + ("craw",))


def test_layer_wider_than_512(tmp_path):
    """A 600-wide layer: the general instantiations (a second sweep round), no local layer 0."""
    from go2_onnx_controller_amd import synth
    p = _write(tmp_path, "plain_wide", synth.mlp_model_bytes(lm.PLAIN_WIDE["dims"], seed=lm.PLAIN_WIDE["seed"]))
    got = plan(p, resident_ms=100)
    assert got["one_round"] == 0 and got["resident_kernel"].startswith("policy_resident_kernel")
    a = check_plan(got, ("multi", None))
    assert a["act"]["nf"] == 0 and max(l["k_pad"] for l in a["gemv"]) == 640


# ---- the checker itself
def test_checker_rejects_overlap_and_misalignment():
    """The r06 mistake (fixed in 79f76a2): the wide kernel's status words placed inside its
    head-product block; and a float4 region two floats off. Both must be refused."""
    good = [["x0", 0, 384], ["h0", 384, 4096], ["hh", 4480, 4096], ["ho", 8576, 128], ["pp", 8704, 2048],
            ["st", 10752, 4]]
    check_regions(good, 10756)
    bad = [r[:] for r in good]
    bad[5][1] = 8704 + 8 * 16  # st = pp + MB * 16: inside pp [8][16][16]
    with pytest.raises(AssertionError, match="st at 8832 overlaps"):
        check_regions(bad, 10756)
    with pytest.raises(AssertionError, match="w0l at 6: not 16-byte aligned"):
        check_regions([["st", 0, 6], ["w0l", 6, 1024]], 1030)
    with pytest.raises(AssertionError, match="unnamed gap of 2 floats in front of w0l"):
        check_regions([["st", 0, 6], ["w0l", 8, 1024]], 1032)
    with pytest.raises(AssertionError, match="the total is"):
        check_regions(good, 10760)
