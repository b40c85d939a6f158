#!/usr/bin/env python3
"""gemv_layer_kernel regression check for a change that touches it: the chain
legs of profiles/skip_touched_ab.json on this tree's library and on two copies of a parent
build, so that the spread between the two identical copies shows what a difference means.

ln_512_pre (synth) at batch 1 and 8 on the GEMV chain, host to host: p50 of --calls
Engine.run calls after --warmup. One process per leg (the library is chosen when the package
is imported, GO2PI_LIB), alternated over --rounds rounds. Writes profiles/res_touched_ab.json.

  python3 tools/res_touched_ab.py --parent-lib A.so --parent2-lib B.so --rounds 5
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


def worker(calls, warmup):
    import numpy as np
    from go2_onnx_controller_amd import Engine, synth
    out = {}
    with Engine(synth.ensure_model("ln_512_pre"), max_batch=8) as e:
        assert e.small_kernel == "gemv_layer_kernel graph", e.small_kernel
        for B in (1, 8):
            x = np.random.default_rng(B).standard_normal((B, e.in_dim)).astype(np.float32)
            for _ in range(warmup):
                e.run(x)
            t = []
            for _ in range(calls):
                t0 = time.perf_counter_ns()
                e.run(x)
                t.append(time.perf_counter_ns() - t0)
            out[f"chain_b{B}_p50_us"] = statistics.median(t) / 1e3
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--parent2-lib")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "res_touched_ab.json"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.calls, args.warmup)
    base = {k: v for k, v in os.environ.items() if not k.startswith("GO2PI_")}
    legs = {"new": {}, "parent": {"GO2PI_LIB": os.path.abspath(args.parent_lib)},
            "parent2": {"GO2PI_LIB": os.path.abspath(args.parent2_lib)}}
    got = {n: {} for n in legs}
    for _ in range(args.rounds):
        for n, env in legs.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--calls", str(args.calls),
                                "--warmup", str(args.warmup)], env=dict(base, **env), capture_output=True, text=True,
                               timeout=300)
            if r.returncode:
                raise SystemExit(f"{n}: exit {r.returncode}\n{r.stdout}{r.stderr}")
            for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items():
                got[n].setdefault(k, []).append(v)
    summary = {n: {k: {"min": min(v), "median": statistics.median(v), "max": max(v), "all": v} for k, v in d.items()}
               for n, d in got.items()}
    res = {"what": "ln_512_pre on the GEMV chain (batch 1 / 8, host to host p50 of %d calls); one process per leg, "
                   "alternated, %d rounds; parent / parent2: two copies of the parent commit's library"
                   % (args.calls, args.rounds), "summary": summary}
    for n, d in summary.items():
        print(n, {k: (round(s["median"], 2), round(s["min"], 2), round(s["max"], 2)) for k, s in d.items()})
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
