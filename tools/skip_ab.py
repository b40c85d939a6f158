#!/usr/bin/env python3
"""Cost of the observation skip pass in the general batched body.

One batched launch at 4096 robots, timed with HIP events on the launching stream:
  skip   270 -> 128 -> 64 -> 19, Concat(obs[0:45], z) -> 512 -> 256 -> 128 -> 12 (Elu): an
         estimator-actor policy; the 512-wide layer reads [19 encoder outputs | 45 observation
         columns], K = 64
  plain  270 -> 128 -> 64 -> 64 -> 512 -> 256 -> 128 -> 12 (Elu): the same padded layer shapes
         (the 19-wide layer pads to 64 in both), the 512-wide layer's K = 64 with no skip
Both run the general body (policy_fused_kernel<8, 0, 0, 0, 0, ...>), so the difference is the
pass: one 16 x 45 gather from L2 and one more barrier per tile. All engines live in one
process; every round times each of them once (alternating, so drift hits them alike),
`--reps` launches between one pair of events. Prints per-leg min / median / max over the
rounds and writes them to --out (profiles/skip_ab.json).

  python3 tools/skip_ab.py --rounds 20 --reps 200
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ENC, ACTOR, PART, IN = (128, 64, 19), (512, 256, 128, 12), 45, 270


def skip_model_bytes(seed=60):
    from go2_onnx_controller_amd import onnx_writer as ow
    rng = np.random.default_rng(seed)
    nodes, inits = [], [("st", np.array([0], np.int64)), ("en", np.array([PART], np.int64)), ("ax", np.array([1], np.int64))]
    dims = [IN] + list(ENC) + list(ACTOR)
    cur = "observation"
    for l in range(len(dims) - 1):
        K, N = dims[l] + (PART if l == len(ENC) else 0), dims[l + 1]
        a = 1.0 / np.sqrt(K)
        inits += [(f"w{l}", rng.uniform(-a, a, (N, K)).astype(np.float32)), (f"b{l}", rng.uniform(-a, a, N).astype(np.float32))]
        if l == len(ENC):
            nodes += [ow.node("Slice", ["observation", "st", "en", "ax"], ["part"]),
                      ow.node("Concat", ["part", cur], ["cat"], "", [ow.attr_int("axis", 1)])]
            cur = "cat"
        last = l == len(dims) - 2
        nodes.append(ow.node("Gemm", [cur, f"w{l}", f"b{l}"], ["action" if last else f"g{l}"], "", [ow.attr_int("transB", 1)]))
        cur = f"g{l}"
        if not last and l != len(ENC) - 1:  # (the encoder's output layer has no activation)
            nodes.append(ow.node("Elu", [cur], [f"a{l}"]))
            cur = f"a{l}"
    return ow.model(nodes, inits, [("observation", ["batch", IN])], [("action", ["batch", ACTOR[-1]])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skip_ab.json"))
    args = ap.parse_args()

    import torch
    from go2_onnx_controller_amd import Engine, synth

    B = args.batch
    plain_dims = (IN,) + ENC[:-1] + (64,) + ACTOR
    legs = {"skip": Engine(skip_model_bytes(), max_batch=B, waves=8),
            "plain": Engine(synth.mlp_model_bytes(dims=plain_dims, seed=61, act="Elu"), max_batch=B, waves=8)}
    for name, e in legs.items():
        if not e.batched_kernel.startswith("policy_fused_kernel<8, 0, 0, 0, 0,"):
            raise SystemExit(f"{name}: not the general body: {e.batched_kernel}")

    obs = torch.randn(B, IN, device="cuda")
    out = torch.empty(B, ACTOR[-1], device="cuda")
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
           "dims": {"skip": [IN, *ENC, f"+{PART}", *ACTOR], "plain": list(plain_dims)},
           "kernel": {n: e.batched_kernel for n, e in legs.items()},
           "us_per_launch": {n: {"min": min(v), "median": statistics.median(v), "max": max(v)} for n, v in us.items()}}
    m = {n: s["median"] for n, s in res["us_per_launch"].items()}
    res["skip_minus_plain_us"] = m["skip"] - m["plain"]
    for n, s in res["us_per_launch"].items():
        print(f"{n:6s} min {s['min']:7.2f}  median {s['median']:7.2f}  max {s['max']:7.2f} us per launch")
    print(f"skip - plain {res['skip_minus_plain_us']:.2f} us (medians)")
    for e in legs.values():
        e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
