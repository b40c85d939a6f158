#!/usr/bin/env python3
"""What a pipeline kernel runs between its MFMA phases, from its device assembly, without a GPU.

    make -C go2_onnx_controller_amd/csrc asm        # lib/asm/kernels_w4_t{2,4,8}.s
    tools/transition_count.py 'policy_mlp_kernel<8, 1, 3, 1, 3, 4>'
    tools/transition_count.py --json 'policy_mlp_kernel<8, 1, 3, 1, 3, 4>'
    tools/transition_count.py --spills              # scratch and spill figures of the w4 units

While a wave runs the instructions between two MFMA phases (a layer's epilogue, the
publish, the flag wait; the head's epilogue; the partial sums and the store), its SIMD's
matrix pipe is idle. This tool finds those stretches in program order and counts their
instructions by class, the class read from the mnemonic's prefix:

    trans   v_exp / v_log / v_rcp / v_rsq / v_sqrt / v_sin / v_cos (8-cycle issue)
    packed  v_pk_*
    mov     v_mov_* / v_accvgpr_*
    plain   every other v_* (VALU)
    lds     ds_*
    vmem    buffer_* / global_* / flat_* / scratch_*
    smem    s_load_* / s_buffer_load_* / s_memtime / s_memrealtime
    salu    every other s_* that is none of the following
    wait    s_waitcnt* / s_nop / s_sleep
    barrier s_barrier
    branch  s_branch / s_cbranch_*

A *gap* is the run of instructions between two MFMAs that follow each other in program
order. Inside a phase a gap holds a fragment load or an LDS read (a few instructions);
a gap of at least --min instructions (default 24) in front of the head is reported as a
transition, with the ordinal of the MFMA in front of it (static, so a rolled loop counts
once). The last 4 * TPW * HT MFMAs are the head's (TPW and HT are the kernel's first two
template arguments; --head-mfmas overrides): everything from the MFMA in front of them
(the last one of the last LDS phase) to the last global store is the head and the tail,
counted together with the head's own MFMAs left out; `tail` is the part after the last
MFMA.

The scheduler may move an epilogue up between the last MFMAs of the phase in front of it, a
tile per gap, and then no single gap is long. So the gaps that hold a transcendental (the
epilogue's v_exp) are reported too, as runs of such gaps at most 3 MFMAs apart: the MFMAs a
run spans, how many of its gaps hold a v_exp, and every non-MFMA instruction between its
first and last MFMA by class. An epilogue that stands as one block shows as 1-3 gaps.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from prologue_count import ASM_DIR, ROOT, demangle, instructions, kernels, norm  # noqa: E402

CLASSES = ("trans", "packed", "mov", "plain", "lds", "vmem", "smem", "salu", "wait", "barrier", "branch")
_TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")


def classify(t):
    op = t.split()[0]
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_"):
        if op.startswith(_TRANS):
            return "trans"
        if op.startswith("v_pk_"):
            return "packed"
        if op.startswith(("v_mov_", "v_accvgpr_")):
            return "mov"
        return "plain"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op == "s_barrier":
        return "barrier"
    if op.startswith(("s_waitcnt", "s_nop", "s_sleep")):
        return "wait"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime")):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    return "plain"


def count(ins):
    c = dict.fromkeys(CLASSES, 0)
    for _, _, t in ins:
        k = classify(t)
        if k != "mfma":
            c[k] += 1
    c["valu"] = c["trans"] + c["packed"] + c["mov"] + c["plain"]
    c["total"] = sum(c[k] for k in CLASSES)
    return c


def head_mfmas(name):
    m = re.match(r"[\w:]+<(\d+),(\d+)", name)
    return 4 * int(m.group(1)) * int(m.group(2)) if m else 0


def report(path, sym, name, min_gap, nhead):
    lines, ks = kernels(path)
    ins = instructions(lines, ks[sym])
    mf = [i for i, (_, _, t) in enumerate(ins) if classify(t) == "mfma"]
    if not mf:
        sys.exit(f"{name}: no MFMA")
    nhead = min(nhead if nhead is not None else head_mfmas(name), len(mf) - 1)
    last_lds = mf[len(mf) - nhead - 1]  # the MFMA in front of the head's
    stores = [i for i, (_, _, t) in enumerate(ins) if t.startswith("global_store") and i > mf[-1]]
    end = stores[-1] if stores else len(ins) - 1
    res = {"kernel": name, "listing": os.path.relpath(path, ROOT), "instructions": len(ins), "mfmas": len(mf),
           "head_mfmas": nhead, "transitions": []}
    for n, (a, b) in enumerate(zip(mf[:-1], mf[1:])):
        if a >= last_lds:
            break
        if b - a - 1 >= min_gap:
            gap = ins[a + 1:b]
            c = count(gap)
            c["after_mfma"] = n + 1
            c["waitcnts"] = [t.split(None, 1)[1] for _, _, t in gap if t.startswith("s_waitcnt")]
            res["transitions"].append(c)
    # where the epilogues (the gaps that hold a transcendental) stand: runs of such gaps at most
    # 3 MFMAs apart, with the MFMAs they span and everything between those MFMAs counted
    runs, cur = [], None
    for n, (a, b) in enumerate(zip(mf[:-1], mf[1:])):
        if any(classify(t) == "trans" for _, _, t in ins[a + 1:b]):
            if cur is not None and n - cur[1] <= 3:
                cur[1], cur[2] = n, cur[2] + 1
            else:
                cur = [n, n, 1]
                runs.append(cur)
    res["epilogues"] = []
    for first, last, gaps in runs:
        c = count([i for i in ins[mf[first] + 1:mf[last + 1]] if classify(i[2]) != "mfma"])
        c.update(first_gap_after_mfma=first + 1, last_gap_after_mfma=last + 1, gaps_with_transcendentals=gaps)
        res["epilogues"].append(c)
    res["head_and_tail"] = count(ins[last_lds + 1:end + 1])
    res["head_largest_gap"] = max((b - a - 1 for a, b in zip(mf[:-1], mf[1:]) if a >= last_lds), default=0)
    res["tail"] = count(ins[mf[-1] + 1:end + 1])
    res["tail"]["waitcnts"] = [t.split(None, 1)[1] for _, _, t in ins[mf[-1] + 1:end + 1] if t.startswith("s_waitcnt")]
    return res


def table(res):
    cols = ("total", "valu", "trans", "packed", "plain", "mov", "lds", "vmem", "smem", "salu", "wait", "barrier", "branch")
    rows = [(f"gap after MFMA {t['after_mfma']}", t) for t in res["transitions"]]
    rows += [(f"epilogue, MFMA {e['first_gap_after_mfma']}-{e['last_gap_after_mfma'] + 1}: "
              f"{e['gaps_with_transcendentals']} gaps hold v_exp", e) for e in res["epilogues"]]
    rows += [("head + tail", res["head_and_tail"]), ("  tail only", res["tail"])]
    out = [f"{res['kernel']}  ({res['listing']}: {res['instructions']} instructions, {res['mfmas']} MFMAs in program "
           f"order, the last {res['head_mfmas']} the head's; largest gap inside the head {res['head_largest_gap']})",
           "| stretch | " + " | ".join(cols) + " |", "|---|" + "---|" * len(cols)]
    for label, c in rows:
        out.append(f"| {label} | " + " | ".join(str(c[k]) for k in cols) + " |")
    return "\n".join(out)


def spills(paths):
    """Per listing: the largest scratch size and the spill counts over its kernels' metadata."""
    out = {}
    for p in paths:
        txt = open(p).read()
        keys = {"private_segment_fixed_size": r"\.private_segment_fixed_size:\s*(\d+)",
                "sgpr_spill_count": r"\.sgpr_spill_count:\s*(\d+)", "vgpr_spill_count": r"\.vgpr_spill_count:\s*(\d+)"}
        out[os.path.relpath(p, ROOT)] = {k: max((int(v) for v in re.findall(rx, txt)), default=None)
                                         for k, rx in keys.items()}
        out[os.path.relpath(p, ROOT)]["kernels"] = len(re.findall(r"^\s*\.amdhsa_kernel\s", txt, re.M))
        # the kernels that use scratch or spill vector registers, by name (metadata keys are in name order)
        per = re.findall(r"\.name:\s*(\S+)\n(?:(?!\.name:).)*?\.private_segment_fixed_size:\s*(\d+)"
                         r"(?:(?!\.name:).)*?\.vgpr_spill_count:\s*(\d+)", txt, re.S)
        bad = [(n, int(s), int(v)) for n, s, v in per if int(s) or int(v)]
        names = demangle([n for n, _, _ in bad])
        out[os.path.relpath(p, ROOT)]["with_scratch"] = {norm(names[n]): {"scratch": s, "vgpr_spills": v} for n, s, v in bad}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("kernel", nargs="?", help="demangled name, e.g. 'policy_mlp_kernel<8, 1, 3, 1, 3, 4>'")
    ap.add_argument("--asm", nargs="*", help="listings to search (default: lib/asm/*.s)")
    ap.add_argument("--min", type=int, default=24, help="smallest gap between two MFMAs reported as a transition")
    ap.add_argument("--head-mfmas", type=int, default=None, help="MFMAs of the head (default 4 * TPW * HT from the name)")
    ap.add_argument("--json", action="store_true", help="one JSON line instead of the table")
    ap.add_argument("--spills", action="store_true", help="scratch size and spill counts of the kernels_w4_t* listings")
    a = ap.parse_args()
    if a.spills:
        paths = a.asm or sorted(glob.glob(os.path.join(ASM_DIR, "kernels_w4_t*.s")))
        if not paths:
            sys.exit("no listing: make -C go2_onnx_controller_amd/csrc asm")
        print(json.dumps(spills(paths), indent=1))
        return 0
    if not a.kernel:
        ap.error("a kernel name (or --spills)")
    paths = a.asm or sorted(glob.glob(os.path.join(ASM_DIR, "*.s")))
    if not paths:
        sys.exit("no listing: make -C go2_onnx_controller_amd/csrc asm")
    want = norm(a.kernel)
    for path in paths:
        _, ks = kernels(path)
        for s, d in demangle(list(ks)).items():
            if norm(d) == want:
                res = report(path, s, want, a.min, a.head_mfmas)
                print(json.dumps(res) if a.json else table(res))
                return 0
    sys.exit(f"{a.kernel}: not in {', '.join(os.path.relpath(p, ROOT) for p in paths)}")


if __name__ == "__main__":
    sys.exit(main())
