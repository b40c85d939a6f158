"""CPU: the engine's kernel choice, planned in pure host code (csrc/plan.cpp) and read
through tests/cpp/plan_probe.cpp: no device is touched.

The expected kernel names are the GPU tests' own tables (imported, not copied): what a GPU
run asserts of a live engine is asserted here of the plan, so a selection bug shows on a
machine without a GPU. Then every diagnostic switch changes the reported kernel as
plan.hpp's Switches says, the refusals keep their messages, the pipeline's bias pack
is the hidden layers' biases back to back, and the recurrent cell's fragment pack is
pack_gru's layout, recomputed here in numpy.
"""
import functools
import json
import os
import subprocess
import types

import numpy as np
import pytest

import graphs
import ln_small_models as lm
import probe_models as pm
import test_gpu_abi_confinement as abi
import test_gpu_lean_tick as lean_tick
import test_gpu_lean_transition as lean_transition
import test_gpu_probe_activations as probe_act
import test_gpu_rnn_widths as rnn_widths
from conftest import ROOT, SHIPPED

GEN8 = probe_act.GEN8


@functools.lru_cache(maxsize=None)
def _exe():
    exe = os.path.join(ROOT, "build", "plan_probe")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    lib = os.path.join(ROOT, "go2_onnx_controller_amd", "lib")
    subprocess.run(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-Werror",
                    "-I" + os.path.join(ROOT, "go2_onnx_controller_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "plan_probe.cpp"),
                    "-L" + lib, "-lgo2pi", "-Wl,-rpath," + lib, "-o", exe], check=True)
    return exe


def plan(model, *args, **opts):
    """The probe's JSON for `model` (a path); args: GO2PI_* switches and ring=...; opts:
    engine options. The switches go on the command line, never into this process."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("GO2PI_")}
    opts.pop("max_batch", None)  # (device buffers only: no part of the plan)
    cmd = [_exe(), str(model)] + [f"{k}={int(v) if isinstance(v, bool) else v}" for k, v in opts.items()] + list(args)
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode in (0, 1), r.stdout + r.stderr
    out = json.loads(r.stdout)
    assert ("error" in out) == (r.returncode == 1)
    return out


def _write(tmp_path, name, data):
    p = tmp_path / (name + ".onnx")
    p.write_bytes(data)
    return str(p)


# ---- 1. the GPU tests' tables
@pytest.mark.parametrize("name", sorted(lean_tick.SHAPES))
def test_one_tick_shapes(synth_path, name):
    p = SHIPPED if name == "shipped" else synth_path(name)
    assert plan(p, small_batch=-1)["batched_kernel"] == lean_tick.SHAPES[name]


def test_head_with_activation_takes_the_looped_form(tmp_path):
    p = _write(tmp_path, "tanh_head", lean_tick._tanh_head_bytes())
    assert plan(p, small_batch=-1)["batched_kernel"] == "policy_mlp_seq_kernel<4, 1, 3, 1, 3, 4>"


@pytest.mark.parametrize("dims", list(lean_transition.PROBES), ids=lean_transition._id)
def test_lean_transition_probes(tmp_path, dims):
    data, _ = pm.int_policy(dims, "Elu", False)
    got = plan(_write(tmp_path, "probe", data), small_batch=-1)
    assert got["batched_kernel"] == lean_transition.PROBES[dims]
    assert got["small_kernel"] == got["batched_kernel"]  # small_batch = -1: no small-batch path


@pytest.mark.parametrize("ring", ["vram", "host"])
@pytest.mark.parametrize("form", list(probe_act.FORMS))
def test_activation_probe_forms(tmp_path, form, ring):
    """Every row of test_gpu_probe_activations.FORMS, both placements, every activation it
    runs, checked by that module's own _check_kernel (with its rule that without a large
    BAR a wide policy gets policy_resident_kernel)."""
    shape, opts, env, _, want_hidden, want_head = probe_act.FORMS[form]
    in_dim, hidden, out_dim = pm.ACT_SHAPES[shape]
    for f, oid in probe_act.CASES:
        if f != form:
            continue
        op, attrs = probe_act._OPS[oid]
        for where, want in (("hidden", want_hidden), ("head", want_head)):
            if want is None:
                continue
            p = _write(tmp_path, f"{oid}_{where}", pm.act_policy(in_dim, hidden, out_dim, op, attrs, where))
            got = plan(p, *([env] if env else []), "ring=" + ring, **opts)
            e = types.SimpleNamespace(batched_kernel=got["batched_kernel"], small_kernel=got["small_kernel"],
                                      resident_kernel=got["resident_kernel"])
            probe_act._check_kernel(e, want)
            if want[0] == "resident":
                assert got["resident_kernel"].endswith(" ring=" + ring)


@pytest.mark.parametrize("name", lm.ALL_MODELS)
def test_ln_small_selection(tmp_path, name):
    """test_gpu_layernorm_small.py test_selection, of the plan."""
    p = lm.model_path(name, tmp_path)
    got = plan(p, ln_small=True)
    assert (got["small_kernel"], got["resident_kernel"]) == ("policy_latency_kernel", "none")
    assert got["batched_kernel"].startswith("policy_fused_kernel<8, 0, 0, 0, 0,")
    for ring in ("vram", "host"):
        got = plan(p, "ring=" + ring, ln_small=True, resident_ms=5000)
        assert got["small_kernel"] == "policy_latency_kernel"
        assert got["resident_kernel"] == lm.RESIDENT_FORM[name] + " ring=" + ring
        assert got["controller_kernel"] == "none"  # no resident controller form for LN
    for res in (0, 5000):  # ln_small off
        got = plan(p, resident_ms=res)
        assert (got["small_kernel"], got["resident_kernel"]) == ("gemv_layer_kernel graph", "none")
    assert plan(p, use_graph=False)["small_kernel"] == "gemv_layer_kernel"
    got = plan(p, small_batch=-1, ln_small=True)
    assert got["small_kernel"] == got["batched_kernel"]


@pytest.mark.parametrize("row", abi.TABLE + [r for r in abi.ALIGN_ROWS if r not in abi.TABLE], ids=lambda r: r.id)
def test_abi_confinement_table(tmp_path, row):
    """tests/test_gpu_abi_confinement.py's table: the batched kernel every row names (a prefix)
    and what serves its batches <= 8."""
    src = abi._source(row.model)
    p = _write(tmp_path, row.id, src) if isinstance(src, bytes) else src
    opts = dict(row.opts)
    if opts.pop("ln_batched", False):
        opts["ln_small"] = 2  # go2pi.h GO2PI_LN_BATCHED
    got = plan(p, *[f"{k}={v}" for k, v in row.env.items()], **opts)
    assert got["batched_kernel"].startswith(row.kernel)
    assert got["small_kernel"] == (row.small or got["batched_kernel"])


def test_abi_confinement_table_reaches_every_batched_body():
    """Every name kernels.hip batched_kernel_name can give has a row: the general body at 4, 8
    and 16 waves, the pipeline's general body, the lean kernel in both forms, the lean
    recurrent ticks, the LN and the residual pipeline, the general residual kernel."""
    for fam in abi.FAMILIES:
        assert any(r.kernel.startswith(fam) for r in abi.TABLE), fam


# ---- 2. the switches (plan.hpp Switches)
SHIPPED_LEAN = "policy_mlp_kernel<2, 1, 3, 1, 3, 4>"


def test_shipped_model_plan():
    got = plan(SHIPPED, resident_ms=100)
    assert got["batched_kernel"] == SHIPPED_LEAN == lean_tick.SHAPES["shipped"]
    assert (got["waves"], got["w4_tpw"], got["head_fuse"], got["w4_c0m"], got["w4_plain"], got["w4_actc"],
            got["w4_nhc"], got["w4_gru_lean"]) == (4, 2, 1, 3, 1, 1, 3, 0)
    assert (got["lds_stride"], got["in_pad"], got["zero_fill"]) == (132, 112, 0)  # 98 padded to 16, not 64
    assert (got["latency_ok"], got["one_round"], got["ctl_hist"]) == (1, 1, 2)
    assert got["small_kernel"] == "policy_latency_kernel"
    assert got["resident_kernel"] == "policy_act1_kernel ring=vram" == got["controller_kernel"]
    c = got["cost"]
    macs = 98 * 128 + 128 * 128 * 2 + 128 * 12
    assert (c["flops_per_row"], c["weight_bytes"], c["io_bytes_per_row"], c["n_layers"], c["has_gru"]) == \
           (2.0 * macs, 4.0 * (macs + 3 * 128 + 12), 4.0 * (98 + 12), 4, 0)


@pytest.mark.parametrize("arg", ["GO2PI_NO_W4", "GO2PI_NO_HEAD_FUSE", "waves=8"])
def test_no_pipeline(arg):
    got = plan(SHIPPED, arg)
    assert got["batched_kernel"] == GEN8 and (got["waves"], got["w4_tpw"]) == (8, 0)
    assert got["head_fuse"] == (0 if arg == "GO2PI_NO_HEAD_FUSE" else 1)


def test_no_plain():
    got = plan(SHIPPED, "GO2PI_NO_PLAIN")
    assert got["batched_kernel"] == "policy_fused_kernel<4, 2, 1, 3, 0, 1, 3>" and got["w4_plain"] == 0


def test_k0_pad64():
    got = plan(SHIPPED, "GO2PI_K0_PAD64")
    assert (got["w4_c0m"], got["in_pad"]) == (0, 128)
    assert got["batched_kernel"] == "policy_mlp_kernel<2, 1, 0, 1, 3, 4>"


@pytest.mark.parametrize("switch,act,nh", [("GO2PI_LEAN_RT_ACT", -1, 0), ("GO2PI_LEAN_RT_NH", 1, 0)])
def test_lean_run_time_forms(switch, act, nh):
    got = plan(SHIPPED, switch)
    assert (got["w4_actc"], got["w4_nhc"]) == (act, nh)
    assert got["batched_kernel"] == f"policy_mlp_kernel<2, 1, 3, {act}, {nh}, 4>"


def test_gru_general(synth_path, tmp_path):
    """A GRU-256 cell in front of three 256-wide hidden layers, and the registry's go2_gru_256
    (512-wide: tests/test_gpu_pipeline.py test_pipeline_gru_ticks names the same kernels)."""
    from go2_onnx_controller_amd import synth
    p256 = _write(tmp_path, "gru_256_h256", synth.gru_model_bytes(head=(256, 256, 256, 12), seed=21))
    for p, tpw in ((p256, 4), (synth_path("go2_gru_256"), 8)):
        got = plan(p)
        assert got["batched_kernel"] == f"policy_gru_kernel<{tpw}, 1, 4>" and got["w4_gru_lean"] == 1
        assert got["small_kernel"] == got["batched_kernel"] and got["cost"]["has_gru"] == 1
        got = plan(p, "GO2PI_GRU_GENERAL")
        assert got["batched_kernel"] == f"policy_fused_kernel<4, {tpw}, 1, 0, 0, 1, 3>" and got["w4_gru_lean"] == 0


@pytest.mark.parametrize("case", rnn_widths.CASES, ids=rnn_widths._id)
def test_rnn_width_cases(tmp_path, case):
    """test_gpu_rnn_widths.py's table, of the plan: the kernel every case names (lean tick or
    general body, its switches given as an engine would read them), and the LDS row and x
    padding its staging relies on."""
    p = _write(tmp_path, "rnn", rnn_widths.model_bytes(case))
    got = plan(p, *[f"{k}={v}" for k, v in case.env], small_batch=-1)
    assert got["batched_kernel"] == case.kernel
    assert got["small_kernel"] == got["batched_kernel"]
    assert (got["w4_gru_lean"], got["lds_stride"], got["in_pad"]) == rnn_widths.plan_scalars(case)
    assert (got["waves"], got["w4_tpw"], got["zero_fill"]) == (4, case.head[0] // 64, 0)


def test_small_chain():
    assert plan(SHIPPED)["small_kernel"] == "policy_latency_kernel"
    got = plan(SHIPPED, "GO2PI_SMALL_CHAIN", resident_ms=100)
    assert got["small_kernel"] == "gemv_layer_kernel graph" and got["latency_ok"] == 0
    assert got["resident_kernel"] == "none"  # ... and no resident form


@pytest.mark.parametrize("switch,act,ctl", [(None, "policy_act1_kernel", "policy_act1_kernel"),
                                            ("GO2PI_RES_R1W", "policy_resident1_kernel", "policy_resident1_kernel"),
                                            ("GO2PI_RES_MULTI", "policy_resident_kernel", "policy_resident_kernel")])
def test_resident_form_switches(switch, act, ctl):
    got = plan(SHIPPED, *([switch] if switch else []), resident_ms=100)
    assert (got["resident_kernel"], got["controller_kernel"]) == (act + " ring=vram", ctl + " ring=vram")
    assert plan(SHIPPED, *([switch] if switch else []))["resident_kernel"] == "none"  # resident_ms = 0


def test_req_host_keeps_the_ring_out_of_device_memory(synth_path):
    p = synth_path("go2_mlp_512")
    assert plan(p, resident_ms=100)["resident_kernel"] == "policy_wide_kernel<4, 8, 12, 0> ring=vram"
    assert plan(p, resident_ms=100, obs_clip=5.0)["resident_kernel"] == "policy_wide_kernel<4, 8, 12, 1> ring=vram"
    assert plan(p, "GO2PI_REQ_HOST", resident_ms=100)["resident_kernel"] == "policy_resident_kernel ring=host"


# ---- 3. the refusals: messages and codes as go2pi_create gives them
E_INVALID, E_MODEL = -1, -2


def test_refusals(tmp_path):
    from go2_onnx_controller_amd import synth
    norm = graphs.write(tmp_path, "normalized_tanh_clip")  # Sub / Div in front, a Clip behind
    assert plan(norm, obs_mean=0.5) == {"error": "model already normalises its input; obs_mean not allowed",
                                        "code": E_INVALID}
    assert plan(norm, obs_std=2.0) == {"error": "model already normalises its input; obs_std not allowed",
                                       "code": E_INVALID}
    assert plan(norm, action_tanh=1) == {
        "error": "action_tanh on a graph that clips or scales its output is not supported", "code": E_INVALID}
    assert "error" not in plan(norm)
    gru = _write(tmp_path, "gru_lbr0_272", synth.gru_model_bytes(I=10, H=272, head=(64, 6), seed=5, lbr=0))
    assert plan(gru) == {"error": "GRU linear_before_reset=0 with hidden size > 256 is not supported", "code": E_MODEL}
    wide = _write(tmp_path, "wide_1400", synth.mlp_model_bytes((24, 1400, 8), seed=3))
    got = plan(wide)  # (two 16-row activation buffers of 1408 + 4 floats alone are 180736 B)
    assert got["code"] == E_MODEL
    assert got["error"].startswith("layer width 1408 needs ") and got["error"].endswith(" B of LDS per tile (> 160 KiB)")
    assert int(got["error"].split()[4]) > 2 * 16 * 1412 * 4 > 160 * 1024


# ---- 4. the bias pack
def _fnv(a):
    h = 0xcbf29ce484222325
    for b in np.ascontiguousarray(a, np.float32).tobytes():
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def test_bias_pack_is_the_hidden_biases_back_to_back(synth_path):
    """go2_mlp_512 (48 -> 512^3 -> 12, three hidden layers on the pipeline): every layer's
    bias vector is the model's (the head's zero-padded to its tile), and the pack the
    pipeline streams is the hidden layers' in order."""
    from test_cpu_boundary import _oracle_layers
    p = synth_path("go2_mlp_512")
    biases = [np.asarray(b, np.float32) for _, b, _, _, _ in _oracle_layers(p)]
    assert [len(b) for b in biases] == [512, 512, 512, 12]
    assert len({_fnv(b) for b in biases[:3]}) == 3  # the three differ: an order would show
    got = plan(p)
    assert got["w4_tpw"] == 8
    padded = biases[:3] + [np.concatenate([biases[3], np.zeros(4, np.float32)])]
    assert got["bias"] == [{"len": len(b), "fnv": _fnv(b)} for b in padded]
    assert got["bpack"] == {"len": 3 * 512, "fnv": _fnv(np.concatenate(biases[:3]))}
    assert plan(p, "GO2PI_NO_W4")["bpack"]["len"] == 0  # no pipeline, no pack


# ---- 5. the recurrent cell's pack
def _pack_gru(W, R, I, H, G):
    """plan.cpp pack_gru in numpy: [Cx + Ch][Ht][gate][lane] float4 over the concatenated
    [x (I padded to 64) | h] axis; lane l of tile t holds unit 16 t + (l & 15), columns
    16 c + 4 (l >> 4) + j; x chunks from W (zeros for k >= I), h chunks from R."""
    ipad = -(-I // 64) * 64
    full = np.zeros((G * H, ipad + H), np.float32)
    full[:, :I], full[:, ipad:] = W, R
    a = full.reshape(G, H // 16, 16, (ipad + H) // 16, 4, 4)   # [gate, t, l & 15, c, l >> 4, j]
    return a.transpose(3, 1, 0, 4, 2, 5).reshape(-1)            # [c, t, gate, l >> 4, l & 15, j]


@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("I", [1, 49, 98, 245])
@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_recurrent_pack_layout(tmp_path, cell, I, H):
    """gru_w, gru_bzr and gru_bh as the cell reads them: lengths and FNVs of the numpy layout.
    GRU: bzr the summed z and r biases, bh the candidate's input and recurrent biases apart;
    LSTM: bzr the four summed gate biases (i, o, f, c), bh unused (zeros)."""
    from go2_onnx_controller_amd import synth
    seed, head = 40 + I + H, (256, 256, 256, 12)
    if cell == "gru":
        G, data = 3, synth.gru_model_bytes(I=I, H=H, head=head, seed=seed, lbr=1)
        W, R, B = synth.gru_params(I, H, seed)
        bzr = B[0, :2 * H] + B[0, 3 * H:5 * H]
        bh = np.concatenate([B[0, 2 * H:3 * H], B[0, 5 * H:]])
    else:
        G, data = 4, synth.lstm_model_bytes(I=I, H=H, head=head, seed=seed)
        W, R, B = synth.lstm_params(I, H, seed)
        bzr, bh = B[0, :4 * H] + B[0, 4 * H:], np.zeros(2 * H, np.float32)
    want = _pack_gru(W[0], R[0], I, H, G)
    assert len(want) == (-(-I // 64) * 64 + H) * G * H
    # the layout, spelled out for a few elements: (chunk, tile, gate, lane, j) -> W or R
    ipad, Ht = -(-I // 64) * 64, H // 16
    for c, t, g, lane, j in [(0, 0, 0, 0, 0), (0, Ht - 1, G - 1, 63, 3), (ipad // 16 - 1, 1, 1, 17, 2),
                             (ipad // 16, 2, 0, 35, 1), ((ipad + H) // 16 - 1, Ht - 1, G - 1, 63, 3)]:
        row, k = g * H + 16 * t + (lane & 15), 16 * c + 4 * (lane >> 4) + j
        v = (W[0][row, k] if k < I else 0.0) if k < ipad else R[0][row, k - ipad]
        assert want[((((c * Ht + t) * G + g) * 64 + lane) * 4) + j] == v
    got = plan(_write(tmp_path, "cell", data))
    assert got["gru_w"] == {"len": len(want), "fnv": _fnv(want)}
    assert got["gru_bzr"] == {"len": len(bzr), "fnv": _fnv(bzr)}
    assert got["gru_bh"] == {"len": len(bh), "fnv": _fnv(bh)}


def test_no_cell_no_recurrent_pack():
    got = plan(SHIPPED)
    assert got["gru_w"]["len"] == got["gru_bzr"]["len"] == got["gru_bh"]["len"] == 0
