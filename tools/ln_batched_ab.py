#!/usr/bin/env python3
"""The 4-wave pipeline's LayerNormalization kernel against the general body.

One batched launch at 4096 robots, timed with HIP events on the launching stream:
  ln512_general   ln_512_pre (48 -> 512^3 -> 12, pre-LN + Elu), default options: the general
                  body with its separate LN pass
  ln512_batched   the same policy, Engine(ln_batched=True): policy_mlp_ln_kernel<8, 1>
  plain512_lean   go2_mlp_512 (the same shape without LN), default: the lean pipeline kernel
  ctl_general     ln_ctl_post (98 -> 128^3 -> 12, Elu + post-LN), default
  ctl_batched     the same policy, ln_batched=True: policy_mlp_ln_kernel<2, 1>
All engines live in one process; every round times each of them once (alternating, so drift
hits them alike), `--reps` launches between one pair of events. Prints per-leg min / median
/ max over the rounds and writes them, every round's figure and the verdict of the rule
below to --out (profiles/ln_batched_ab.json).

The rule, per pair (general, batched): the new kernel's time is below the general body's in
every round, and the gap between the medians is larger than the general body's own min-max
spread over the rounds.

  python3 tools/ln_batched_ab.py --rounds 12 --reps 200
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENERAL = "policy_fused_kernel<8, 0, 0, 0, 0,"
ASM_DIR = os.path.join(ROOT, "go2_onnx_controller_amd", "lib", "asm")


def instantiations(asm_dir=ASM_DIR):
    """Registers, spills, scratch and occupancy of every policy_mlp_ln_kernel instantiation,
    read from the units' device listings (make -C go2_onnx_controller_amd/csrc asm); {} where
    they have not been made."""
    import re
    out = {}
    for t in (2, 4, 8):
        path = os.path.join(asm_dir, f"kernels_w4ln_t{t}.s")
        if not os.path.exists(path):
            continue
        text = open(path).read()
        for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S*policy_mlp_ln_kernelILi(\d)ELi(\d)E\S*)", text, re.M):
            sym, name = m.group(1), f"policy_mlp_ln_kernel<{m.group(2)}, {m.group(3)}>"
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ln_batched_ab.json"))
    args = ap.parse_args()
    if args.rounds < 10:
        raise SystemExit("at least 10 rounds")

    import torch
    from go2_onnx_controller_amd import Engine, synth

    B = args.batch
    ln512, plain512, ctl = (synth.ensure_model(n) for n in ("ln_512_pre", "go2_mlp_512", "ln_ctl_post"))
    legs = {
        "ln512_general": (Engine(ln512, max_batch=B), 48, GENERAL),
        "ln512_batched": (Engine(ln512, max_batch=B, ln_batched=True), 48, "policy_mlp_ln_kernel<8, 1>"),
        "plain512_lean": (Engine(plain512, max_batch=B), 48, "policy_mlp_kernel<8, 1, 3, 1, 3, 4>"),
        "ctl_general": (Engine(ctl, max_batch=B), 98, GENERAL),
        "ctl_batched": (Engine(ctl, max_batch=B, ln_batched=True), 98, "policy_mlp_ln_kernel<2, 1>"),
    }
    for name, (e, _, want) in legs.items():
        if not e.batched_kernel.startswith(want):
            raise SystemExit(f"{name}: expected {want}, got {e.batched_kernel}")

    obs = {w: torch.randn(B, w, device="cuda") for w in (48, 98)}
    out = torch.empty(B, 12, device="cuda")
    stream = torch.cuda.current_stream()
    launch = {n: e.device_launcher(obs[w].data_ptr(), out.data_ptr(), B, stream.cuda_stream)
              for n, (e, w, _) in legs.items()}
    for fn in launch.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()

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
           "kernel": {n: e.batched_kernel for n, (e, _, _) in legs.items()},
           "us_per_launch": {n: {"min": min(v), "median": statistics.median(v), "max": max(v)} for n, v in us.items()},
           "us_per_round": us}
    m = {n: s["median"] for n, s in res["us_per_launch"].items()}
    res["rule"] = {}
    for pair, g, b in (("ln_512_pre", "ln512_general", "ln512_batched"), ("ln_ctl_post", "ctl_general", "ctl_batched")):
        spread = max(us[g]) - min(us[g])
        res["rule"][pair] = {
            "below_in_every_round": all(y < x for x, y in zip(us[g], us[b])),
            "median_gap_us": m[g] - m[b],
            "general_spread_us": spread,
            "gap_exceeds_spread": m[g] - m[b] > spread,
        }
    res["gap_to_lean_us"] = m["ln512_batched"] - m["plain512_lean"]
    res["instantiations"] = instantiations()
    for n, s in res["us_per_launch"].items():
        print(f"{n:14s} min {s['min']:7.2f}  median {s['median']:7.2f}  max {s['max']:7.2f} us per launch")
    for pair, r in res["rule"].items():
        print(f"{pair}: below in every round {r['below_in_every_round']}, median gap {r['median_gap_us']:.2f} us, "
              f"general body's spread {r['general_spread_us']:.2f} us")
    print(f"ln512_batched - plain512_lean {res['gap_to_lean_us']:.2f} us (medians)")
    for e, _, _ in legs.values():
        e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
