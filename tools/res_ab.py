#!/usr/bin/env python3
"""Cost of a residual layer in the general batched body.

One batched launch at 4096 robots, timed with HIP events on the launching stream:
  res    48 -> 256 (pre-LN) -> 256 Relu -> 256 + carried (pre-LN) -> 12: one SimBa block; layer
         0's un-normalised sum is carried and added behind layer 2's Gemm
  plain  the same layers, weights and LayerNormalizations without the Add
`res` runs policy_fused_res_kernel<8>, `plain` the 8-wave general body it is an instantiation
of, so the difference is the carried tile: one float4 store per lane and tile in the source
layer, one float4 load and four adds in the consumer, the tile's clear at kernel start and a
third LDS buffer. All engines live in one process; every round times each of them once
(alternating, so drift hits them alike), `--reps` launches between one pair of events. Prints
per-leg min / median / max over the rounds and writes them to --out (profiles/res_ab.json).

  python3 tools/res_ab.py --rounds 20 --reps 200
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IN, H, OUT = 48, 256, 12


def model_bytes(res, seed=70):
    from go2_onnx_controller_amd import onnx_writer as ow
    rng = np.random.default_rng(seed)
    # (N, activation, pre-LN, adds layer 0's carried value)
    layers = [(H, None, True, False), (H, "Relu", False, False), (H, None, True, res), (OUT, None, False, False)]
    nodes, inits, cur, K, tap = [], [], "observation", IN, None
    for l, (N, act, ln, add) in enumerate(layers):
        a = 1.0 / np.sqrt(K)
        inits += [(f"w{l}", rng.uniform(-a, a, (N, K)).astype(np.float32)), (f"b{l}", rng.uniform(-a, a, N).astype(np.float32))]
        last = l == len(layers) - 1
        y = "action" if last else f"g{l}"
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "res_ab.json"))
    args = ap.parse_args()

    import torch
    from go2_onnx_controller_amd import Engine

    B = args.batch
    legs = {"res": Engine(model_bytes(True), max_batch=B, waves=8), "plain": Engine(model_bytes(False), max_batch=B, waves=8)}
    want = {"res": "policy_fused_res_kernel<8>", "plain": "policy_fused_kernel<8, 0, 0, 0, 0,"}
    for name, e in legs.items():
        if not e.batched_kernel.startswith(want[name]):
            raise SystemExit(f"{name}: not {want[name]}: {e.batched_kernel}")

    obs = torch.randn(B, IN, device="cuda")
    out = torch.empty(B, OUT, device="cuda")
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
           "dims": [IN, H, H, H, OUT], "kernel": {n: e.batched_kernel for n, e in legs.items()},
           "us_per_launch": {n: {"min": min(v), "median": statistics.median(v), "max": max(v)} for n, v in us.items()}}
    m = {n: s["median"] for n, s in res["us_per_launch"].items()}
    res["res_minus_plain_us"] = m["res"] - m["plain"]
    for n, s in res["us_per_launch"].items():
        print(f"{n:6s} min {s['min']:7.2f}  median {s['median']:7.2f}  max {s['max']:7.2f} us per launch")
    print(f"res - plain {res['res_minus_plain_us']:.2f} us (medians)")
    for e in legs.values():
        e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
