#!/usr/bin/env python3
"""act() latency of a residual MLP policy at batch 1 and 8 on each small-batch path (DESIGN §4.7,
"small-batch forms"), in the method of tools/skip_small_ab.py.

Host to host around one go2pi_run (Engine.run_ptr on fixed buffers, the observation rewritten
before every call), p50 / p99 over `--calls` calls after `--warmup`, on simba_64 (48 -> 64 ->
128 -> 64 -> 128 -> 64 -> 12: six layers, two blocks) and simba_256 (four layers, one block) of
tests/policy_specs.py, both under ln_small = 1. Legs:
  a         GO2PI_RESIDUAL_SMALL unset: gemv_layer_kernel, one launch per layer replayed as a graph
  a_parent  the same on another build of the library (--parent-lib: the parent commit's), control
  b         GO2PI_RESIDUAL_SMALL=1, resident_ms = 0: policy_latency_kernel, one launch
  c         GO2PI_RESIDUAL_SMALL=1, resident_ms > 0: the multi-workgroup resident kernel
  d         a LayerNormalization MLP of the same padded layer shapes without the Adds on the same
            resident kernel with the same tiled layer 0 (GO2PI_RES_MULTI=1, GO2PI_RES_TILED0=1):
            what the carried add itself costs per request
One process per leg and round (the switch is read at engine creation; nothing of another leg
polls or holds CUs beside the one being timed), legs alternated within a round, `--rounds`
rounds; per leg the median [min, max] over the rounds of each figure.

  python3 tools/res_small_ab.py --rounds 5 --parent-lib go2_onnx_controller_amd/lib/diag/libgo2pi_parent.so
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# the residual models' layer shapes and LayerNormalizations without the Adds
PLAIN = {"simba_64": dict(dims=(48, 64, 128, 64, 128, 64, 12), layer_norm=("pre", None, "pre", None, "pre")),
         "simba_256": dict(dims=(48, 256, 256, 256, 12), layer_norm=("pre", None, "pre"))}
BATCHES = (1, 8)


def child(args):
    """One leg in this process: {model: {batch: {p50_us, p99_us, min_us}, kernel}} as one JSON line."""
    import tempfile

    import numpy as np
    import policy_specs as ps
    from go2_onnx_controller_amd import Engine, synth

    leg, out = args.leg, {}
    d = tempfile.mkdtemp(prefix="res_small_ab_")
    res_ms = args.resident_ms if leg in ("c", "d") else 0
    for name in PLAIN:
        if leg == "d":
            path = os.path.join(d, name + "_plain.onnx")
            with open(path, "wb") as fh:
                fh.write(synth.mlp_model_bytes(seed=61, act="Relu", **PLAIN[name]))
        else:
            path = ps.model_path(name, d)
        with Engine(path, max_batch=8, resident_ms=res_ms, ln_small=True) as e:
            rng = np.random.default_rng(0)
            per = {}
            for B in BATCHES:
                obs = rng.standard_normal((B, e.in_dim)).astype(np.float32)
                act = np.zeros((B, e.out_dim), np.float32)
                us = []
                for i in range(args.warmup + args.calls):
                    obs[i % B, i % obs.shape[1]] += np.float32(1e-3)  # a fresh observation every call
                    t0 = time.perf_counter_ns()
                    e.run_ptr(obs.ctypes.data, act.ctypes.data, B)
                    t1 = time.perf_counter_ns()
                    if i >= args.warmup:
                        us.append((t1 - t0) * 1e-3)
                us.sort()
                per[str(B)] = {"p50_us": us[len(us) // 2], "p99_us": us[int(len(us) * 0.99)], "min_us": us[0]}
            out[name] = {"batch": per, "small_kernel": e.small_kernel, "resident_kernel": e.resident_kernel,
                         "resident_launches": e.resident_launches}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg")  # (set by the parent process for its children)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--resident-ms", type=int, default=1000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "res_small_ab.json"))
    args = ap.parse_args()
    if args.leg:
        return child(args)

    base = {k: v for k, v in os.environ.items() if not k.startswith("GO2PI_")}
    on = {"GO2PI_RESIDUAL_SMALL": "1"}
    legs = {"a": {}, "b": on, "c": on, "d": {"GO2PI_RES_MULTI": "1", "GO2PI_RES_TILED0": "1"}}
    if args.parent_lib:
        legs["a_parent"] = {"GO2PI_LIB": os.path.abspath(args.parent_lib)}
    runs = {n: [] for n in legs}
    for r in range(args.rounds):
        for n, env in legs.items():
            if n == "a_parent" and r > 0:
                continue  # the control: once
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", n, "--calls", str(args.calls), "--warmup",
                   str(args.warmup), "--resident-ms", str(args.resident_ms)]
            p = subprocess.run(cmd, capture_output=True, text=True, env=dict(base, **env), timeout=300)
            line = next((l for l in p.stdout.splitlines() if l.startswith("RESULT ")), None)
            if p.returncode != 0 or line is None:
                raise SystemExit(f"leg {n} round {r} failed ({p.returncode}):\n{p.stdout[-2000:]}{p.stderr[-2000:]}")
            runs[n].append(json.loads(line[7:]))
            print(f"round {r} leg {n} done", flush=True)

    res = {"rounds": args.rounds, "calls": args.calls, "warmup": args.warmup, "resident_ms": args.resident_ms,
           "legs": {}}
    for n, rs in runs.items():
        res["legs"][n] = {}
        for model in rs[0]:
            m = {"small_kernel": rs[0][model]["small_kernel"], "resident_kernel": rs[0][model]["resident_kernel"],
                 "resident_launches": [r[model]["resident_launches"] for r in rs], "batch": {}}
            for B in rs[0][model]["batch"]:
                m["batch"][B] = {}
                for fig in ("p50_us", "p99_us"):
                    v = [r[model]["batch"][B][fig] for r in rs]
                    m["batch"][B][fig] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
                s = m["batch"][B]
                print(f"{n:9s} {model:10s} B={B}  p50 {s['p50_us']['median']:7.2f} [{s['p50_us']['min']:.2f}, "
                      f"{s['p50_us']['max']:.2f}]  p99 {s['p99_us']['median']:7.2f} [{s['p99_us']['min']:.2f}, "
                      f"{s['p99_us']['max']:.2f}] us  [{m['resident_kernel'] if m['resident_kernel'] != 'none' else m['small_kernel']}]")
            res["legs"][n][model] = m
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
