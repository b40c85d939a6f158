#!/usr/bin/env python3
"""Where a pipeline kernel's prologue stands in its device assembly, without a GPU.

    make -C go2_onnx_controller_amd/csrc asm        # lib/asm/kernels_w4_t{2,4,8}.s
    tools/prologue_count.py 'policy_mlp_kernel<8, 1, 3, 1, 3, 4>'
    tools/prologue_count.py --list lib/asm/kernels_w4_t2.s

For the kernel it prints, in program order (instruction positions from the entry, labels
and directives not counted): every load in front of the first MFMA (direct-to-LDS loads,
weight-fragment buffer loads, scalar loads), the atomics, the barriers and the first MFMA
itself; then the kernel's lane-spill moves (v_writelane_b32 / v_readlane_b32: SGPRs the
compiler parked in VGPR lanes), and its register and LDS figures from the metadata.

Positions are static (program order). A loop in front of the first MFMA is reported with its
label so that the dynamic path can be walked from the listing: --path prints the instructions
up to the first MFMA with their positions.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASM_DIR = os.path.join(ROOT, "go2_onnx_controller_amd", "lib", "asm")

_FUNC = re.compile(r"^([A-Za-z_.$][\w.$]*):\s*(;.*)?$")
_LABEL = re.compile(r"^(\.LBB\w+):")


def demangle(names):
    """{mangled: demangled}; c++filt ships with binutils and with ROCm's llvm (llvm-cxxfilt)."""
    for tool in ("c++filt", "llvm-cxxfilt", "/opt/rocm/llvm/bin/llvm-cxxfilt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
            return dict(zip(names, out.splitlines()))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def norm(name):
    """A kernel's demangled name without its return type, argument list and blanks."""
    name = re.sub(r"^void\s+", "", name)
    name = re.sub(r"\(.*$", "", name)
    name = name.replace("go2pi::", "")
    return re.sub(r"\s+", "", name)


def kernels(path):
    """{mangled symbol: (first line, last line)} of the .amdhsa kernels in a listing."""
    lines = open(path).read().splitlines()
    syms = [m.group(1) for l in lines if (m := re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", l))]
    out = {}
    for s in syms:
        try:
            a = lines.index(s + ":")
        except ValueError:
            a = next(i for i, l in enumerate(lines) if l.startswith(s + ":"))
        b = next(i for i in range(a, len(lines)) if lines[i].strip().startswith("s_endpgm"))
        # a kernel may hold more than one s_endpgm: its text ends at .Lfunc_end
        e = next((i for i in range(b, len(lines)) if lines[i].startswith(".Lfunc_end")), b + 1)
        out[s] = (a + 1, e)
    return lines, out


def instructions(lines, span):
    """[(position, label or None, text)]: position counts instructions only."""
    pos, label, out = 0, None, []
    for l in lines[span[0]:span[1]]:
        if m := _LABEL.match(l):
            label = m.group(1)
            continue
        t = l.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        out.append((pos, label, t))
        label = None
        pos += 1
    return out


def classify(t):
    op = t.split()[0]
    if op.startswith("v_mfma"):
        return "mfma"
    if op == "s_barrier":
        return "barrier"
    if op.startswith("s_waitcnt"):
        return "wait"
    if "atomic" in op:
        return "atomic"
    if op.startswith("global_load_lds") or (op.startswith("buffer_load") and t.endswith(" lds")):
        return "lds_load"
    if op.startswith("buffer_load"):
        return "fragment_load"
    if op.startswith(("global_load", "flat_load")):
        return "vector_load"
    if op.startswith(("s_load", "s_buffer_load")):
        return "scalar_load"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    return None


def report(path, sym, name, show_path):
    lines, ks = kernels(path)
    ins = instructions(lines, ks[sym])
    first_mfma = next((p for p, _, t in ins if classify(t) == "mfma"), None)
    res = {"kernel": name, "listing": os.path.relpath(path, ROOT), "instructions": len(ins), "first_mfma": first_mfma}
    pro = [(p, lab, t, classify(t)) for p, lab, t in ins if first_mfma is None or p <= first_mfma]
    for kind in ("fragment_load", "lds_load", "scalar_load", "vector_load", "atomic", "barrier"):
        res[kind + "s"] = [p for p, _, _, k in pro if k == kind]
    res["prologue_waits"] = [[p, t.split(None, 1)[1]] for p, _, t, k in pro if k == "wait"]
    res["prologue_branches"] = [[p, t] for p, _, t, k in pro if k == "branch"]
    res["prologue_loops"] = [lab for p, lab, t, _ in pro if lab and any(
        k == "branch" and t2.split()[-1] == lab and p2 >= p for p2, _, t2, k in pro)]
    res["v_writelane_b32"] = sum(t.startswith("v_writelane_b32") for _, _, t in ins)
    res["v_readlane_b32"] = sum(t.startswith("v_readlane_b32") for _, _, t in ins)
    meta = "\n".join(lines)
    m = re.search(r"\.amdhsa_kernel\s+" + re.escape(sym) + r"\n(.*?)\.end_amdhsa_kernel", meta, re.S)
    if m:
        for key in ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size"):
            if v := re.search(r"\.amdhsa_" + key + r"\s+(\S+)", m.group(1)):
                res[key] = v.group(1)
    if show_path:
        for p, lab, t, k in pro:
            print(f"{p:5d} {lab or '':12s} {t}" + (f"    ; <{k}>" if k and k != "wait" else ""))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("kernel", nargs="?", help="demangled name, e.g. 'policy_mlp_kernel<8, 1, 3, 1, 3, 4>'")
    ap.add_argument("--asm", nargs="*", help="listings to search (default: lib/asm/*.s)")
    ap.add_argument("--list", metavar="LISTING", help="print the kernels of one listing")
    ap.add_argument("--path", action="store_true", help="print the instructions up to the first MFMA")
    a = ap.parse_args()
    if a.list:
        _, ks = kernels(a.list)
        for s, d in sorted(demangle(list(ks)).items(), key=lambda x: x[1]):
            print(norm(d))
        return 0
    if not a.kernel:
        ap.error("a kernel name (or --list)")
    paths = a.asm or sorted(glob.glob(os.path.join(ASM_DIR, "*.s")))
    if not paths:
        sys.exit("no listing: make -C go2_onnx_controller_amd/csrc asm")
    want = norm(a.kernel)
    for path in paths:
        _, ks = kernels(path)
        for s, d in demangle(list(ks)).items():
            if norm(d) == want:
                print(json.dumps(report(path, s, want, a.path)))
                return 0
    sys.exit(f"{a.kernel}: not in {', '.join(os.path.relpath(p, ROOT) for p in paths)} (try --list)")


if __name__ == "__main__":
    sys.exit(main())
