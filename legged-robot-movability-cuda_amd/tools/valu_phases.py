#!/usr/bin/env python3
"""Static per-phase instruction split of the table kernels' loop (no GPU needed).

Cross-compiles csrc/lrm_tol_kernels.hip to gfx950 assembly with the Makefile's flags, once as shipped and once with
-DLRM_PHASE_MARKS (an `s_nop` with a comment at every phase boundary: lrm_point_tol.h LRM_PHASE), and prints for
dist_tab_kernel<2,false,true> (LRM_MODE_TOL_REL) and dist_tab_kernel<2,false,false> (LRM_MODE_TOL) the instructions of the
loop's COMMON path by phase and by class.  Text between a "rare_*" mark and the next numbered mark is left out: outer-grid
lanes, the second candidate, the in-loop flush, the doubt push.  An instruction belongs to the last mark in front of it in
the assembly text; the scheduler may move instructions across a mark, so the split is a guide (a few instructions either
way), the totals are what counts.  The marks themselves perturb the code: the tool prints whole-kernel totals of both builds.

--xtab prints the same for the bit-exact side instead: the loop of dist_xtab_kernel<2,false> (LRM_MODE_FAST; its alternative and
twin phases are run by every wave and belong to the common path), the replay tail of dist_tab_kernel<2,false,true> (the text
between its replay_* marks, behind the loop) and the whole of tol_fixup_kernel<2,false> (one latency chain, no phases).

    python tools/valu_phases.py [--src DIR] > profiles/valu_phases.txt
    python tools/valu_phases.py --xtab [--src DIR] > profiles/valu_phases_xtab.txt
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = [("dist_tab_kernel<2,false,true>  (tol_rel)", "dist_tab_kernelILi2ELb0ELb1EE"),
           ("dist_tab_kernel<2,false,false> (tol)", "dist_tab_kernelILi2ELb0ELb0EE")]
XTAB = ("dist_xtab_kernel<2,false> (fast)", "dist_xtab_kernelILi2ELb0EE")
REPLAY = ("dist_tab_kernel<2,false,true>: replay tail (tol_rel)", "dist_tab_kernelILi2ELb0ELb1EE")
FIXUP = ("tol_fixup_kernel<2,false> (fix-up of every mode)", "tol_fixup_kernelILi2ELb0E")
CLASSES = ["vop12_vgpr", "v_cndmask", "v_cmp", "vop3_sgpr_lit", "trans_cvt", "SALU", "s_load", "LDS", "global", "s_waitcnt"]
VALU = CLASSES[:5]
TRANS = re.compile(r"v_(rsq|sqrt|rcp|exp|log|sin|cos|cvt)_")
LITERAL = re.compile(r"(?<![\w.])(0x[0-9a-f]+|\d{3,}|6[5-9]|[7-9]\d)(?![\w.\]])")  # not an inline constant (-16..64, a few floats)


def makefile_flags(src):
    text = open(os.path.join(src, "Makefile")).read()
    arch = re.search(r"^GPU_ARCH\s*=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M).group(1).split()
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", text, re.M).group(1)
    return hipcc, ["--offload-arch=" + arch] + flags


def assembly(src, extra, out):
    hipcc, flags = makefile_flags(src)
    subprocess.run([hipcc] + flags + extra + ["--cuda-device-only", "-S", "-o", out, os.path.join(src, "lrm_tol_kernels.hip")],
                   check=True, stderr=subprocess.DEVNULL)
    return open(out).read().splitlines()


def function(lines, tag):
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and tag in l.split(":")[0])
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start + 1:end]


def classify(line):
    """class of an instruction line, None for labels / directives / comments / the marks"""
    code = line.split(";")[0].strip()
    if not code or code.endswith(":") or code.startswith("."):
        return None
    op, _, args = code.partition(" ")
    if op == "s_nop":
        return None
    if op.startswith("v_"):
        if op.startswith("v_cndmask"):
            return "v_cndmask"
        if op.startswith("v_cmp"):
            return "v_cmp"
        if TRANS.match(op):
            return "trans_cvt"
        if op.endswith("_e32") and not re.search(r"\bs\d|\bs\[|vcc|exec|\bm0\b", args) and not LITERAL.search(args):
            return "vop12_vgpr"
        return "vop3_sgpr_lit"
    if op.startswith(("s_load", "s_buffer_load")):
        return "s_load"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "global"
    return "SALU"


def totals(body):
    t = dict.fromkeys(CLASSES, 0)
    for l in body:
        c = classify(l)
        if c:
            t[c] += 1
    return t


def phases(body):
    """{phase: {class: count}} of the text behind a mark; the end-of-loop mark ends its phase without opening another.
    The replay_* marks only count behind the loop: the copy of the replay inside the loop stays with the loop's own phase."""
    out, phase, in_loop = {}, None, False
    for l in body:
        m = re.search(r"LRM_PHASE (\w+)", l)
        if m:
            name = m.group(1)
            if name == "end_of_loop":
                phase, in_loop = None, False
            elif not name.startswith("replay_"):
                phase, in_loop = name, True
            elif not in_loop:
                phase = name
            continue
        c = classify(l)
        if phase and c:
            out.setdefault(phase, dict.fromkeys(CLASSES, 0))[c] += 1
    return out


def row(name, t):
    return f"{name:<32}" + "".join(f"{t[c]:>14}" for c in CLASSES) + f"{sum(t[c] for c in VALU):>8}"


def table(title, ph, skip, head):
    print(f"\n== {title} (build with phase marks) ==")
    print(head)
    common = dict.fromkeys(CLASSES, 0)
    for name in sorted(ph):
        if name.startswith(skip[0]):
            continue
        print(row(name, ph[name]))
        if not name.startswith(skip[1:]):
            for c in CLASSES:
                common[c] += ph[name][c]
    return common


def whole(fm, fp):
    tm, tp = totals(fm), totals(fp)
    print(row("whole kernel, with marks", tm))
    print(row("whole kernel, as shipped", tp))
    print(f"the marks moved {sum(tm[c] for c in VALU) - sum(tp[c] for c in VALU):+d} VALU and {tm['SALU'] - tp['SALU']:+d} SALU instructions in the whole kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(HERE, "..", "csrc"), help="directory of lrm_tol_kernels.hip and the Makefile")
    ap.add_argument("--xtab", action="store_true", help="the bit-exact side: dist_xtab_kernel, the replay tail, tol_fixup_kernel")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        plain = assembly(args.src, [], os.path.join(tmp, "plain.s"))
        marked = assembly(args.src, ["-DLRM_PHASE_MARKS"], os.path.join(tmp, "marked.s"))
    head = f"{'':<32}" + "".join(f"{c:>14}" for c in CLASSES) + f"{'VALU':>8}"
    print("static instruction counts, gfx950; classes: vop12_vgpr = VOP1/VOP2 with VGPR operands only; vop3_sgpr_lit = other VOP3 and")
    print("SGPR-operand / literal forms; trans_cvt = transcendental and conversion; VALU = the first five columns")
    if args.xtab:
        fm, fp = function(marked, XTAB[1]), function(plain, XTAB[1])
        common = table(XTAB[0] + ": one round of the loop", phases(fm), ("replay_", "rare_"), head)
        print(row("COMMON PATH (without rare_*)", common))
        whole(fm, fp)
        fm = function(marked, REPLAY[1])
        ph = {k: v for k, v in phases(fm).items() if k.startswith("replay_")}
        table(REPLAY[0] + ": one pass of 64 records", ph, ("\0",), head)
        fm, fp = function(marked, FIXUP[1]), function(plain, FIXUP[1])
        print(f"\n== {FIXUP[0]}: no marks inside ==")
        print(head)
        whole(fm, fp)
        return 0
    for title, tag in KERNELS:
        fm, fp = function(marked, tag), function(plain, tag)
        common = table(title + ": common path of one round of the loop", phases(fm), ("replay_", "rare_"), head)
        print(row("COMMON PATH (without rare_*)", common))
        whole(fm, fp)
    return 0


if __name__ == "__main__":
    sys.exit(main())
