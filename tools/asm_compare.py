#!/usr/bin/env python3
"""Two device listings of the same kernel unit (make asm), compared kernel by kernel.

    tools/asm_compare.py parent/kernels_w4_t8.s go2_onnx_controller_amd/lib/asm/kernels_w4_t8.s

One line per kernel, by demangled name: 'same' when the instruction streams are equal with
local labels normalised, else 'DIFF'; then a/b of the instruction count, the v_mfma count
and NumVgprs / NumAgprs / NumSgprs / ScratchSize / Occupancy. --changed prints only the
kernels that differ. The exit status is 0 when every kernel is the same, 1 otherwise.

A kernel's text runs from its symbol's label to its .Lfunc_end, and its figures are read
behind that up to the next kernel symbol's label, so a kernel can never take in a
neighbour, wherever the metadata blocks stand.
"""
import re
import sys

from prologue_count import demangle, norm

FIGS = ("NumVgprs", "NumAgprs", "NumSgprs", "ScratchSize", "Occupancy")


def kernels(path):
    """{demangled name: (normalised instructions, {figure: value})} of one listing."""
    lines = open(path).read().splitlines()
    syms = {m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))}
    starts = [(i, m.group(1)) for i, l in enumerate(lines) if (m := re.match(r"([\w.$]+):", l)) and m.group(1) in syms]
    names = demangle([s for _, s in starts])
    out = {}
    for (a, sym), (b, _) in zip(starts, starts[1:] + [(len(lines), None)]):
        end = next(i for i in range(a, b) if lines[i].startswith(".Lfunc_end"))
        labels = {}  # local label -> its order of definition in this kernel
        for l in lines[a + 1:end]:
            if m := re.match(r"(\.L\w+):", l):
                labels[m.group(1)] = f".L{len(labels)}"
        ins = [re.sub(r"\.L\w+", lambda m: labels.get(m.group(0), m.group(0)), t) for l in lines[a + 1:end]
               if (t := l.split(";")[0].strip()) and not t.startswith(".") and not t.endswith(":")]
        figs = {}  # (the listing's SGPR line is TotalNumSgprs: with VCC and the like)
        for l in lines[end:b]:
            if m := re.match(r"; (NumVgprs|NumAgprs|TotalNumSgprs|ScratchSize|Occupancy): (\d+)", l):
                figs.setdefault(m.group(1).replace("Total", ""), int(m.group(2)))
        out[norm(names[sym])] = (ins, figs)
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--changed"]
    if len(args) != 2:
        sys.exit(__doc__)
    ka, kb = kernels(args[0]), kernels(args[1])
    differ = sorted(set(ka) ^ set(kb))
    for name in differ:
        print(f"ONLY in {args[0] if name in ka else args[1]}: {name}")
    for name in sorted(set(ka) & set(kb)):
        (ia, fa), (ib, fb) = ka[name], kb[name]
        same = ia == ib
        differ += [] if same else [name]
        if same and "--changed" in sys.argv:
            continue
        mf = [sum(t.startswith("v_mfma") for t in i) for i in (ia, ib)]
        print(f"{'same' if same else 'DIFF'} {name}: instructions {len(ia)}/{len(ib)} v_mfma {mf[0]}/{mf[1]} "
              + " ".join(f"{k} {fa.get(k)}/{fb.get(k)}" for k in FIGS))
    print(f"{len(set(ka) & set(kb))} kernels in both, {len(differ)} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
