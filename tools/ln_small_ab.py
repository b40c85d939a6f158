#!/usr/bin/env python3
"""Batch-1 act() latency of a LayerNormalization policy on each small-batch path.

Host to host around one go2pi_run at batch 1 (Engine.run_ptr on fixed buffers, the
observation rewritten before every call), p50 / p99 over `--calls` calls per leg after
`--warmup`, on ln_ctl_post (98 -> 128^3 -> 12, post-LN) and ln_512_pre (48 -> 512^3 -> 12,
pre-LN):
  chain     ln_small = 0: gemv_layer_kernel, one launch per layer replayed as a hipGraph
            (what an LN policy's act() ran before ln_small existed: the baseline)
  launch    ln_small = 1, resident_ms = 0: policy_latency_kernel, one launch
  resident  ln_small = 1, resident_ms > 0: the default resident form
  multi     the same with GO2PI_RES_MULTI=1 at create: the multi-workgroup resident form
and, for what the LN pass itself costs per request, the same shapes without LN on the same
resident forms:
  plain_resident  shipped model (98 -> 128^3 -> 12) / go2_mlp_512 with GO2PI_RES_MULTI=1
  plain_multi     shipped model with GO2PI_RES_MULTI=1 (go2_mlp_512: the same leg again)
All engines of a model live in one process; a round times `--chunk` calls of each leg in
turn (alternating, so drift hits them alike). Each leg has its own engine; with the
default --resident-ms 20 a resident leg's kernel idles out while the other legs run, so
no other leg's kernel polls beside the one being timed, and the 20 untimed calls in front
of every chunk relaunch it. Writes --out (profiles/ln_small_ab.json).

  python3 tools/ln_small_ab.py --calls 4000
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHIPPED = os.path.join(ROOT, "tests", "golden", "model.onnx")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--chunk", type=int, default=500)
    ap.add_argument("--resident-ms", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ln_small_ab.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from go2_onnx_controller_amd import Engine, synth

    def engine(path, multi=False, **kw):
        if multi:
            os.environ["GO2PI_RES_MULTI"] = "1"  # read at engine creation
        try:
            return Engine(path, max_batch=8, **kw)
        finally:
            os.environ.pop("GO2PI_RES_MULTI", None)

    res = {"calls": args.calls, "warmup": args.warmup, "chunk": args.chunk, "resident_ms": args.resident_ms,
           "device": torch.cuda.get_device_name(0), "models": {}}
    rms = args.resident_ms
    for ln_name, plain_path, plain_name in (("ln_ctl_post", SHIPPED, "shipped"),
                                            ("ln_512_pre", synth.ensure_model("go2_mlp_512"), "go2_mlp_512")):
        p = synth.ensure_model(ln_name)
        legs = {
            "chain": engine(p),
            "launch": engine(p, ln_small=True),
            "resident": engine(p, ln_small=True, resident_ms=rms),
            "multi": engine(p, multi=True, ln_small=True, resident_ms=rms),
            "plain_resident": engine(plain_path, multi=plain_name == "go2_mlp_512", resident_ms=rms),
            "plain_multi": engine(plain_path, multi=True, resident_ms=rms),
        }
        rng = np.random.default_rng(0)
        obs = rng.standard_normal((1, legs["chain"].in_dim)).astype(np.float32)
        act = np.zeros((1, 12), np.float32)
        us = {n: [] for n in legs}

        def burst(e, n, sink):
            for i in range(n):
                obs[0, i % obs.shape[1]] += np.float32(1e-3)  # a fresh observation every call
                t0 = time.perf_counter_ns()
                e.run_ptr(obs.ctypes.data, act.ctypes.data, 1)
                t1 = time.perf_counter_ns()
                if sink is not None:
                    sink.append((t1 - t0) * 1e-3)

        for n, e in legs.items():
            burst(e, args.warmup, None)
        done = 0
        while done < args.calls:
            k = min(args.chunk, args.calls - done)
            for n, e in legs.items():
                burst(e, 20, None)  # (the leg's resident kernel idled out while the others ran: relaunch, untimed)
                burst(e, k, us[n])
            done += k
        out = {}
        for n, e in legs.items():
            v = sorted(us[n])
            out[n] = {"small_kernel": e.small_kernel, "resident_kernel": e.resident_kernel,
                      "resident_launches": e.resident_launches, "p50_us": v[len(v) // 2],
                      "p99_us": v[int(len(v) * 0.99)], "min_us": v[0]}
            print(f"{ln_name:12s} {n:15s} p50 {out[n]['p50_us']:7.2f}  p99 {out[n]['p99_us']:7.2f}  min {v[0]:7.2f} us"
                  f"  [{e.resident_kernel if e.resident_kernel != 'none' else e.small_kernel}]", flush=True)
        res["models"][ln_name] = {"plain": plain_name, "legs": out}
        for e in legs.values():
            e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
