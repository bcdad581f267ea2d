#!/usr/bin/env python3
"""Instruction counts of the board loop of k_equity<N> (pk_equity.hip), from hipcc's own assembly output with the library's build flags:
the innermost backward branch that spans the N inlined hand evaluations is the loop over a lane's boards (its common path: no carry into
an earlier card of the combination).  Per seat count: instructions, VALU, SALU and LDS instructions per board, VALU per evaluated hand
(all N seats live), registers and LDS of the kernel.  The streaming evaluator's figure to set it against is 124 VALU per hand.
usage: tools/equity_isa.py [N ...]      (default 2 6 9)
       tools/equity_isa.py --ev [N ...] the same for k_ev<N> (pk_equity_ev.hip; default every seat count): the loop holds the N evaluations AND the
                                        comparisons of a group of levels, so instr/board is the cost of a board with every level of the group compared"""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pokerl_amd import build


def main():
    ev = "--ev" in sys.argv[1:]
    seats = [int(a) for a in sys.argv[1:] if a != "--ev"] or (build.SEATS if ev else [2, 6, 9])
    src, label = ("pk_equity_ev.hip", "k_ev") if ev else ("pk_equity.hip", "k_equity")
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "e.s")
        subprocess.check_call([build.hipcc()] + build.COMPILE_FLAGS + ["--cuda-device-only", "-S", os.path.join(build.CSRC, src), "-o", asm])
        s = open(asm).read()
    print("kernel        instr/board  valu  salu  lds   valu/hand  vgpr  sgpr  lds_bytes  scratch")
    for n in seats:
        name = ("_Z4k_evILi%dEEvPKjN2pk6EvWorkEi" if ev else "_Z8k_equityILi%dEEvPKjN2pk6EqWorkENS2_5EqOutEi") % n
        a = s.index(name + ":")
        body = s[a:s.index(".Lfunc_end", a)].split("\n")
        labels, ins = {}, []
        for line in body:
            t = line.strip()
            m = re.match(r"^(\.LBB\d+_\d+):", t)
            if m:
                labels[m.group(1)] = len(ins)
            elif t and not t.startswith((".", ";", "//")) and not t.endswith(":"):
                ins.append(t.split(";")[0].strip())
        loops = []
        for i, t in enumerate(ins):
            m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", t)
            if m and m.group(1) in labels and labels[m.group(1)] <= i:
                loops.append((i - labels[m.group(1)] + 1, labels[m.group(1)], i))
        # the shortest loop that holds all N evaluations (each reads the table at least six times)
        size, lo, hi = min(l for l in loops if sum(1 for t in ins[l[1]:l[2] + 1] if t.startswith("ds_read")) >= 6 * n)
        seg = ins[lo:hi + 1]
        valu = sum(t.startswith("v_") for t in seg)
        meta = [blk for blk in s[s.index("amdhsa.kernels:"):].split("\n  - ") if re.search(r"\.name:\s+%s\n" % name, blk)][0]
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, meta).group(1))
        print("%-8s<%-2d>  %11d  %4d  %4d  %3d   %9.1f  %4d  %4d  %9d  %7d" % (
            label, n, size, valu, sum(t.startswith("s_") for t in seg), sum(t.startswith("ds_") for t in seg), valu / n,
            get("vgpr_count"), get("sgpr_count"), get("group_segment_fixed_size"), get("private_segment_fixed_size")))


if __name__ == "__main__":
    main()
