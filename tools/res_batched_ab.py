#!/usr/bin/env python3
"""The 4-wave pipeline's residual kernel against the general residual body.

One batched launch at 4096 robots, timed with HIP events on the launching stream, of one SimBa
block (48 -> H pre-LN -> H Relu -> H + carried, pre-LN -> 12; tests/policy_specs.py simba_256's
and tests/res_batched_specs.py resb_t8_simba's layers) at H = 256 and H = 512:
  simba256_general  default: policy_fused_res_kernel<8>, the carried value in a third LDS tile
  simba256_batched  the same policy under GO2PI_RESIDUAL_BATCHED: policy_mlp_res_kernel<4, 1>
  simba512_general / simba512_batched  likewise: policy_mlp_res_kernel<8, 1>
Both legs of a pair run the same library; the switch is read when an engine is created, so it
is set around the creation of the batched legs alone. All engines live in one process; every
round times each of them once (alternating, so drift hits them alike), `--reps` launches
between one pair of events. Prints per-leg min / median / max over the rounds and writes them,
every round's figure, the verdict of the rule below and the new instantiations' registers
(from make asm, where the listings exist) to --out (profiles/res_batched_ab.json).

The rule, per pair: the pipeline is "faster" only where its maximum over the rounds lies below
the general body's minimum.

  python3 tools/res_batched_ab.py --rounds 12 --reps 200
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SW = "GO2PI_RESIDUAL_BATCHED"
GENERAL = "policy_fused_res_kernel<8>"
IN, OUT = 48, 12
ASM_DIR = os.path.join(ROOT, "go2_onnx_controller_amd", "lib", "asm")


def model_bytes(H, seed=70):
    from go2_onnx_controller_amd import onnx_writer as ow
    rng = np.random.default_rng(seed + H)
    # (N, activation, pre-LN, adds layer 0's carried value)
    layers = [(H, None, True, False), (H, "Relu", False, False), (H, None, True, True), (OUT, None, False, False)]
    nodes, inits, cur, K, tap = [], [], "observation", IN, None
    for l, (N, act, ln, add) in enumerate(layers):
        a = 1.0 / np.sqrt(K)
        inits += [(f"w{l}", rng.uniform(-a, a, (N, K)).astype(np.float32)), (f"b{l}", rng.uniform(-a, a, N).astype(np.float32))]
        y = "action" if l == len(layers) - 1 else f"g{l}"
        nodes.append(ow.node("Gemm", [cur, f"w{l}", f"b{l}"], [y], "", [ow.attr_int("transB", 1)]))
        if add:
            nodes.append(ow.node("Add", [tap, y], [f"s{l}"]))
            y = f"s{l}"
        if ln:
            if l == 0:
                tap = y
            inits += [(f"g{l}s", rng.uniform(0.75, 1.25, N).astype(np.float32)),
                      (f"g{l}b", rng.uniform(-0.25, 0.25, N).astype(np.float32))]
            nodes.append(ow.node("LayerNormalization", [y, f"g{l}s", f"g{l}b"], [f"n{l}"], "", [ow.attr_int("axis", -1)]))
            y = f"n{l}"
        if act:
            nodes.append(ow.node(act, [y], [f"a{l}"]))
            y = f"a{l}"
        cur, K = y, N
    return ow.model(nodes, inits, [("observation", ["batch", IN])], [("action", ["batch", OUT])])


def instantiations(asm_dir=ASM_DIR):
    """Registers, spills, scratch and occupancy of every policy_mlp_res_kernel instantiation,
    read from the units' device listings (make -C go2_onnx_controller_amd/csrc asm); {} where
    they have not been made."""
    import re
    out = {}
    for t in (2, 4, 8):
        path = os.path.join(asm_dir, f"kernels_w4res_t{t}.s")
        if not os.path.exists(path):
            continue
        text = open(path).read()
        for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S*policy_mlp_res_kernelILi(\d)ELi(\d)E\S*)", text, re.M):
            sym, name = m.group(1), f"policy_mlp_res_kernel<{m.group(2)}, {m.group(3)}>"
            figs = {}
            body = text[text.index(f"\n{sym}:"):]
            for key in ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "Occupancy"):
                figs[key] = int(re.search(rf"; {key}: (\d+)", body).group(1))
            # (the kernel's entry of the metadata: entries start at "- .agpr_count")
            for block in text.split("- .agpr_count")[1:]:
                if re.search(rf"\.name:\s+{re.escape(sym)}\s", block):
                    for key in ("sgpr_spill_count", "vgpr_spill_count"):
                        figs[key] = int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))
            out[name] = figs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "res_batched_ab.json"))
    args = ap.parse_args()
    if args.rounds < 10:
        raise SystemExit("at least 10 rounds")

    import torch
    from go2_onnx_controller_amd import Engine

    B = args.batch
    os.environ.pop(SW, None)
    legs, want = {}, {}
    for H, tpw in ((256, 4), (512, 8)):
        data = model_bytes(H)
        legs[f"simba{H}_general"], want[f"simba{H}_general"] = Engine(data, max_batch=B), GENERAL
        os.environ[SW] = "1"  # read by the engine at creation, for its life
        legs[f"simba{H}_batched"] = Engine(data, max_batch=B)
        want[f"simba{H}_batched"] = f"policy_mlp_res_kernel<{tpw}, 1>"
        del os.environ[SW]
    for name, e in legs.items():
        if not e.batched_kernel.startswith(want[name]):
            raise SystemExit(f"{name}: expected {want[name]}, got {e.batched_kernel}")

    obs = torch.randn(B, IN, device="cuda")
    out = {n: torch.empty(B, OUT, device="cuda") for n in legs}
    stream = torch.cuda.current_stream()
    launch = {n: e.device_launcher(obs.data_ptr(), out[n].data_ptr(), B, stream.cuda_stream) for n, e in legs.items()}
    for fn in launch.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    # the two legs of a pair compute the same function (each in its own order of additions)
    agree = {f"simba{H}": float((out[f"simba{H}_general"] - out[f"simba{H}_batched"]).abs().max()) for H in (256, 512)}
    for pair, d in agree.items():
        if not d <= 2e-5:
            raise SystemExit(f"{pair}: the legs differ by {d}")

    us = {n: [] for n in legs}
    for _ in range(args.rounds):
        for n, fn in launch.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(args.reps):
                fn()
            t1.record(stream)
            t1.synchronize()
            us[n].append(t0.elapsed_time(t1) * 1e3 / args.reps)
    res = {"batch": B, "rounds": args.rounds, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "kernel": {n: e.batched_kernel for n, e in legs.items()},
           "us_per_launch": {n: {"min": min(v), "median": statistics.median(v), "max": max(v)} for n, v in us.items()},
           "us_per_round": us, "legs_max_abs_difference": agree}
    res["rule"] = {}
    for H in (256, 512):
        g, b = us[f"simba{H}_general"], us[f"simba{H}_batched"]
        res["rule"][f"simba{H}"] = {
            "batched_max_us": max(b), "general_min_us": min(g),
            "faster": max(b) < min(g),  # the claim stands only where the spreads do not touch
            "median_gap_us": statistics.median(g) - statistics.median(b),
        }
    res["instantiations"] = instantiations()
    for n, s in res["us_per_launch"].items():
        print(f"{n:17s} min {s['min']:7.2f}  median {s['median']:7.2f}  max {s['max']:7.2f} us per launch")
    for pair, r in res["rule"].items():
        print(f"{pair}: pipeline max {r['batched_max_us']:.2f} us, general min {r['general_min_us']:.2f} us: "
              f"{'faster' if r['faster'] else 'NOT shown faster'} (median gap {r['median_gap_us']:.2f} us)")
    for e in legs.values():
        e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
