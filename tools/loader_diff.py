#!/usr/bin/env python3
"""No GPU: this checkout's ONNX loader against another checkout's, file by file over one corpus.

    git worktree add /tmp/parent HEAD~1
    tools/loader_diff.py /tmp/parent/go2_onnx_controller_amd/csrc [--time] [--keep DIR]

tests/cpp/loader_dump.cpp is built with plain g++ against both csrc directories' onnx_model.cpp
and both programs read the same files. Per file they print the inspect_json text and a hash over
every field of Model, or the exception's text; the first differing line ends the run with status
1. A change that is meant to leave the loader's behaviour alone has no differing line.

The corpus is what the CPU tests generate: the shipped model, the synth registry, every
tests/graphs.py variant, the skip / residual / LayerNormalization / probe model builders, every
refusal graph of the CPU tests, graphs on either side of the graph queries' depth caps
(cap_graphs), the derandomised mutants of tests/test_cpu_fuzz.py and the mutations of
tests/test_cpu_skip.py. The last line counts it: files, ok, error, and the share of
the mutants that are refused (the fuzz test asks for more than a quarter).

--time: the median parse time of go2_mlp_512 and of the 270-wide skip model ea_k64 under both
loaders (loader_dump's own timer, 20 runs each), for the record.
"""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "go2_onnx_controller_amd", "csrc")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def build(csrc, exe):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++20", "-O2", "-I" + csrc, os.path.join(ROOT, "tests", "cpp", "loader_dump.cpp"),
                    os.path.join(csrc, "onnx_model.cpp"), "-o", exe], check=True)
    return exe


def cap_graphs():
    """Graphs on either side of the graph queries' depth caps: the observation (or a Slice of it)
    through n Identity nodes into an Add of two computed values (the refusal changes where the
    search stops seeing the Add), and a residual connection's tap n Identity nodes from its Add."""
    import numpy as np
    from go2_onnx_controller_amd import onnx_writer as ow
    r = np.random.default_rng(0)
    tb = [ow.attr_int("transB", 1)]
    inits = [("W0", r.standard_normal((8, 8)).astype(np.float32)), ("W1", r.standard_normal((8, 8)).astype(np.float32)),
             ("Wo", r.standard_normal((3, 8)).astype(np.float32)), ("st", np.array([0], np.int64)),
             ("en", np.array([8], np.int64)), ("ax", np.array([1], np.int64))]

    def idents(v, n, tag, slice_at=-1):
        nodes = []
        for i in range(n):
            op, ins = ("Slice", [v, "st", "en", "ax"]) if i == slice_at else ("Identity", [v])
            nodes.append(ow.node(op, ins, [f"{tag}{i}"]))
            v = f"{tag}{i}"
        return nodes, v

    out = []
    for n in range(14, 21):
        for kind, slice_at in (("obs", -1), ("slice", 0), ("mid", n // 2)):
            for first in (0, 1):  # the chain in front of the main Gemm in node order, or behind it
                chain, v = idents("obs", n, "i", slice_at)
                main = [ow.node("Gemm", ["obs", "W0"], ["g0"], "", tb)]
                nodes = (chain + main if first else main + chain) + [
                    ow.node("Add", ["g0", v], ["s0"], "add"), ow.node("Relu", ["s0"], ["a0"]),
                    ow.node("Gemm", ["a0", "Wo"], ["act"], "", tb)]
                out.append((f"cap/{kind}/{first}/{n}", ow.model(nodes, inits, [("obs", [1, 8])], [("act", [1, 3])])))
        for long_main in (0, 1):
            side, v = idents("z", n, "i")
            main, mv = idents("z", 4 * n * long_main, "m")
            nodes = [ow.node("Gemm", ["obs", "W0"], ["g0"], "", tb), ow.node("Relu", ["g0"], ["z"])] + side + main + [
                ow.node("Gemm", [mv, "W1"], ["h1"], "", tb), ow.node("Add", ["h1", v], ["s1"], "add"),
                ow.node("Relu", ["s1"], ["a1"]), ow.node("Gemm", ["a1", "Wo"], ["act"], "", tb)]
            out.append((f"cap/tap/{long_main}/{n}", ow.model(nodes, inits, [("obs", [1, 8])], [("act", [1, 3])])))
    # two refusals at once in the prologue: a second Mul / Sub whose constant is INT64 (a Mul names
    # the repetition, a Sub the constant)
    for op in ("Mul", "Sub"):
        nodes = [ow.node(op, ["obs", "c0"], ["x1"]), ow.node(op, ["x1", "ci"], ["x2"]), ow.node("Gemm", ["x2", "Wo"], ["act"], "", tb)]
        consts = inits + [("c0", np.ones(8, np.float32)), ("ci", np.ones(8, np.int64))]
        out.append((f"order/prologue/{op}", ow.model(nodes, consts, [("obs", [1, 8])], [("act", [1, 3])])))
    return out


def corpus():
    """[(label, bytes)] in a fixed order, and the index range of the mutants."""
    import graphs
    import ln_batched_models
    import ln_small_models
    import policy_specs as ps
    import probe_models as pm
    import test_cpu_fuzz
    import test_cpu_layernorm
    import test_cpu_res
    import test_cpu_skip
    from go2_onnx_controller_amd import synth

    out = [("shipped", open(test_cpu_fuzz.SHIPPED, "rb").read())]
    out += [(f"synth/{n}", make()) for n, make in synth.MODELS.items()]
    out += [(f"graphs/{k}/{seed}", graphs.variant_bytes(k, seed)) for k in graphs.VARIANTS for seed in (0, 3)]
    out += [(f"graphs/{k}", graphs.wide_bytes(k)) for k in graphs.WIDE_VARIANTS + graphs.WIDE_EDGES]
    # (labelled as before tests/policy_specs.py held these models, so that kept outputs compare)
    for label, names in (("skip_models", ps.SKIP.names + ps.SKIP.probes),
                         ("skip_small_models", ps.SMALL_NAMES + ps.SMALL_PROBES),
                         ("res_models", ps.RES.names + ps.RES.probes)):
        out += [(f"{label}/{n}", ps.model_bytes(n)) for n in names]
    for mod in (ln_small_models, ln_batched_models):
        out += [(f"{mod.__name__}/{n}", mod.model_bytes(n)) for n in mod.ALL_MODELS]
        out.append((f"{mod.__name__}/zero_variance", mod.zero_variance_model()[0]))
    out += [(f"probe/int/{n}", pm.int_probe(n)[0]) for n in pm.INT_PROBES]
    for shape, (i, hidden, o) in pm.ACT_SHAPES.items():
        for tag, op, attrs in pm.ACT_OPS:
            for where in ("hidden", "head"):
                out.append((f"probe/act/{shape}/{tag}/{where}", pm.act_policy(i, hidden, o, op, attrs, where)))
    out += [(f"refuse/boundary/{k}", make()) for k, make in graphs.UNSUPPORTED.items()]
    out += [(f"refuse/skip/{k}", test_cpu_skip._refusal(k)) for k in test_cpu_skip.REFUSALS]
    out += [(f"refuse/res/{k}", test_cpu_res._refusal(k)) for k in test_cpu_res.REFUSALS]
    for k in sorted(test_cpu_layernorm.REFUSED):
        make, steps, kw, _ = test_cpu_layernorm.REFUSED[k]
        out.append((f"refuse/ln/{k}", make(steps, **kw)))
    out += cap_graphs()
    first = len(out)
    cases = []
    test_cpu_fuzz._collect(sink=cases)
    assert len(cases) >= 2000, len(cases)
    out += [(f"fuzz/{i}", d) for i, d in enumerate(cases)]
    for n in ps.SKIP.names:
        out += [(f"skip_mut/{n}/{i}", d) for i, d in enumerate(test_cpu_skip._mutations(n, 300))]
    return out, range(first, len(out))


def run(exe, listing):
    r = subprocess.run([exe, listing], capture_output=True, text=True, errors="replace", check=True)
    return r.stdout.splitlines()


def main():
    args = sys.argv[1:]
    timed = "--time" in args
    keep = args[args.index("--keep") + 1] if "--keep" in args else None
    rest = [a for a in args if a != "--time" and a != "--keep" and a != keep]
    if len(rest) != 1 or not os.path.exists(os.path.join(rest[0], "onnx_model.cpp")):
        sys.exit(__doc__)
    new = build(CSRC, os.path.join(ROOT, "build", "loader_dump_new"))
    old = build(rest[0], os.path.join(ROOT, "build", "loader_dump_parent"))
    files, mutants = corpus()
    work = keep or tempfile.mkdtemp(prefix="loader_diff_")
    os.makedirs(work, exist_ok=True)
    try:
        paths = []
        for i, (_, data) in enumerate(files):
            paths.append(os.path.join(work, f"{i}.onnx"))
            with open(paths[-1], "wb") as fh:
                fh.write(data)
        listing = os.path.join(work, "list.txt")
        with open(listing, "w") as fh:
            fh.write("\n".join(paths) + "\n")
        a, b = run(old, listing), run(new, listing)
        if keep:
            for name, lines in (("parent.txt", a), ("new.txt", b)):
                with open(os.path.join(work, name), "w") as fh:
                    fh.write("".join(f"{label}\t{l}\n" for (label, _), l in zip(files, lines)))
        if len(a) != len(files) or len(b) != len(files):
            sys.exit(f"{len(files)} files, but {len(a)} lines from the parent's loader and {len(b)} from this one")
        for (label, _), la, lb in zip(files, a, b):
            if la != lb:
                sys.exit(f"DIFF at {label}:\n  parent: {la[:600]}\n  this:   {lb[:600]}")
        n_err = sum(l.startswith("error ") for l in b)
        refused = sum(b[i].startswith("error ") for i in mutants)
        print(f"{len(files)} files, 0 differing lines: {len(files) - n_err} ok, {n_err} error; "
              f"{refused} of {len(mutants)} mutants refused")
        if refused * 4 <= len(mutants):
            sys.exit("fewer than a quarter of the mutants are refused")
        if timed:
            from go2_onnx_controller_amd import synth
            for label, data in (("go2_mlp_512", synth.MODELS["go2_mlp_512"]()),
                                ("ea_k64", dict(files)["skip_models/ea_k64"])):
                p = os.path.join(work, "timed.onnx")
                with open(p, "wb") as fh:
                    fh.write(data)
                us = [subprocess.run([exe, "--time", "20", p], capture_output=True, text=True, check=True).stdout.strip()
                      for exe in (old, new)]
                print(f"parse {label} ({len(data)} bytes): parent {us[0]} us, this {us[1]} us (median of 20)")
    finally:
        if not keep:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
