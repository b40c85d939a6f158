#!/usr/bin/env python3
"""Cost of the LayerNormalization pass in the general batched body.

One batched launch at 4096 robots, timed with HIP events on the launching stream:
  ln        ln_512_pre  (48 -> 512^3 -> 12, pre-LN + Elu on every hidden layer)
  plain     go2_mlp_512 (the same shape without LN) forced onto the same general body
            (waves=8): the baseline the pass is charged against, not the lean kernel
  plain_nhf plain with GO2PI_NO_HEAD_FUSE=1 at create: an LN in front of the head turns
            head fusion off, so this leg shows how much of the difference is the head
All engines live in one process; every round times each of them once (alternating, so
drift hits them alike), `--reps` launches between one pair of events. Prints per-leg
min / median / max over the rounds and writes them to --out (profiles/ln_ab.json).

  python3 tools/ln_ab.py --rounds 20 --reps 200
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ln_ab.json"))
    args = ap.parse_args()

    import torch
    from go2_onnx_controller_amd import Engine, synth

    B = args.batch
    legs = {}
    legs["ln"] = Engine(synth.ensure_model("ln_512_pre"), max_batch=B, waves=8)
    legs["plain"] = Engine(synth.ensure_model("go2_mlp_512"), max_batch=B, waves=8)
    os.environ["GO2PI_NO_HEAD_FUSE"] = "1"  # read at engine creation
    legs["plain_nhf"] = Engine(synth.ensure_model("go2_mlp_512"), max_batch=B, waves=8)
    del os.environ["GO2PI_NO_HEAD_FUSE"]
    for name, e in legs.items():
        if not e.batched_kernel.startswith("policy_fused_kernel<8, 0, 0, 0, 0,"):
            raise SystemExit(f"{name}: not the general body: {e.batched_kernel}")

    obs = torch.randn(B, 48, device="cuda")
    out = torch.empty(B, 12, device="cuda")
    stream = torch.cuda.current_stream()
    launch = {n: e.device_launcher(obs.data_ptr(), out.data_ptr(), B, stream.cuda_stream) for n, e in legs.items()}
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
           "kernel": {n: e.batched_kernel for n, e in legs.items()},
           "us_per_launch": {n: {"min": min(v), "median": statistics.median(v), "max": max(v)} for n, v in us.items()}}
    m = {n: s["median"] for n, s in res["us_per_launch"].items()}
    res["ln_minus_plain_us"] = m["ln"] - m["plain"]
    res["ln_minus_plain_nhf_us"] = m["ln"] - m["plain_nhf"]
    for n, s in res["us_per_launch"].items():
        print(f"{n:10s} min {s['min']:7.2f}  median {s['median']:7.2f}  max {s['max']:7.2f} us per launch")
    print(f"ln - plain {res['ln_minus_plain_us']:.2f} us, ln - plain_nhf {res['ln_minus_plain_nhf_us']:.2f} us (medians)")
    for e in legs.values():
        e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
