#!/usr/bin/env python3
"""Issue slots of the fused rollout kernels' main loop, from hipcc's own assembly output with the library's build flags.  At one wave per
SIMD every instruction -- a lane-mask AND on an SGPR pair, an s_nop, a branch -- costs the same issue slot as a v_add_f64
(profiles/r05_valu_rates.txt), so the loop is steered by the count of ALL its instructions, by region and by class:

  regions   betting passes   from the loop's header to the parking test (its two s_bcnt1 and the two scalar branches behind them)
            end_block        from there to the block the loop goes on with when end_block is skipped
            loop control     what is left of the loop (the latch, the path round end_block)
  classes   VALU, LDS, VMEM, SALU mask ops (64-bit lane-mask algebra), s_nop, branch + exec (branches, saveexec, writes to exec),
            s_waitcnt, other SALU

The counts are static: one per instruction in the region, whichever lanes or branches run.  Runs on the CPU.
usage: tools/loop_slots.py [--asm FILE --seats N] [kernel<N> ...]     (default: k_rollout<6> k_rollout_tab<6> k_rollout_allin_tab<9>)"""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pokerl_amd import build
from tools.isa_report import split_asm

CLASSES = ["VALU", "LDS", "VMEM", "SALU mask ops", "s_nop", "branch + exec", "s_waitcnt", "other SALU"]
MASK_OP = re.compile(r"^s_(and|or|xor|andn2|orn2|nand|nor|xnor|not|cselect|mov)_b64$")
INSN = re.compile(r"^\s+([a-z][a-z_0-9]+)(?:\s+([^;\n]*))?")


def classify(op, operands):
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    if op == "s_nop":
        return "s_nop"
    if op == "s_waitcnt":
        return "s_waitcnt"
    dst = operands.split(",")[0].strip() if operands else ""
    if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_endpgm", "s_barrier")) or "saveexec" in op or dst == "exec":
        return "branch + exec"
    if MASK_OP.match(op):
        return "SALU mask ops"
    return "other SALU"


def assembly(n):
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "t.s")
        r = subprocess.run([build.hipcc()] + build.table_flags(n) + ["-DPK_SEATS=%d" % n, "--cuda-device-only", "-S", os.path.join(build.CSRC, "pk_tables.hip"), "-o", asm],
                           capture_output=True, text=True)
        if r.returncode:
            sys.exit(r.stderr)
        return open(asm).read()


def main_loop(body):
    """(lines of the kernel, index of the main loop's header label, index one past the loop): the depth-1 loop with the most instructions."""
    lines = body.split("\n")
    label = re.compile(r"^(\.LBB\d+_\d+):\s*(;.*)?$")
    heads = [i for i, l in enumerate(lines) if label.match(l) and re.search(r"Loop Header: Depth=1\b", l)]
    best = None
    for h in heads:
        end = len(lines)
        for j in range(h + 1, len(lines)):
            m = label.match(lines[j])
            if m and (not m.group(2) or "Depth=" not in m.group(2) or re.search(r"Loop Header: Depth=1\b", lines[j])):
                end = j
                break
        size = sum(1 for l in lines[h:end] if INSN.match(l))
        if best is None or size > best[2]:
            best = (h, end, size)
    if best is None:
        raise SystemExit("no loop found")
    h, end, _ = best
    # blocks of the loop laid out in FRONT of its header (the path round end_block): labels that name this header
    name = label.match(lines[h]).group(1)[2:]       # ".LBB16_13" -> "BB16_13", as the block comments spell it
    start = h
    for j in range(h - 1, -1, -1):
        m = label.match(lines[j])
        if m:
            if m.group(2) and "Header=" + name + " " in m.group(2) + " ":
                start = j
            else:
                break
    return lines, start, h, end


def regions(body):
    lines, start, h, end = main_loop(body)
    # the parking test: the first two s_bcnt1 behind the header, then two branches on a scalar condition (leave the loop / skip end_block)
    seen_bcnt, seen_br, split, targets = 0, 0, None, []
    for j in range(h, end):
        m = INSN.match(lines[j])
        if not m:
            continue
        if m.group(1).startswith("s_bcnt1"):
            seen_bcnt += 1
        elif seen_bcnt >= 2 and re.match(r"s_cbranch_(vcc|scc)", m.group(1)):
            seen_br += 1
            targets.append(m.group(2).strip())
            if seen_br == 2:
                split = j + 1
                break
    if split is None:
        raise SystemExit("parking test not found")
    stop = end
    for j in range(split, end):
        m = re.match(r"^(\.LBB\d+_\d+):", lines[j])
        if m and m.group(1) in targets:
            stop = j
            break
    return lines, [("betting passes", [(h, split)]), ("end_block", [(split, stop)]), ("loop control", [(start, h), (stop, end)])]


def count(lines, spans):
    c, ops = dict.fromkeys(CLASSES, 0), {}
    for a, b in spans:
        for l in lines[a:b]:
            m = INSN.match(l)
            if not m or l.lstrip().startswith((".", ";")):
                continue
            k = classify(m.group(1), m.group(2) or "")
            c[k] += 1
            if k != "VALU":
                ops[m.group(1)] = ops.get(m.group(1), 0) + 1
    return c, ops


def report(kernel, body, out=sys.stdout):
    lines, regs = regions(body)
    print("==== %s" % kernel, file=out)
    print("%-16s %6s  %s" % ("region", "slots", "  ".join("%13s" % k for k in CLASSES)), file=out)
    total = dict.fromkeys(CLASSES, 0)
    detail = []
    for name, spans in regs:
        c, ops = count(lines, spans)
        for k in CLASSES:
            total[k] += c[k]
        print("%-16s %6d  %s" % (name, sum(c.values()), "  ".join("%13d" % c[k] for k in CLASSES)), file=out)
        detail.append((name, ops))
    print("%-16s %6d  %s" % ("loop", sum(total.values()), "  ".join("%13d" % total[k] for k in CLASSES)), file=out)
    for name, ops in detail:
        print("  %s, not VALU: %s" % (name, ", ".join("%d %s" % (n, o) for o, n in sorted(ops.items(), key=lambda kv: (-kv[1], kv[0])))), file=out)


if __name__ == "__main__":
    argv = sys.argv[1:]
    asm_file = seats_arg = None
    if "--asm" in argv:
        i = argv.index("--asm"); asm_file = argv[i + 1]; del argv[i:i + 2]
    if "--seats" in argv:
        i = argv.index("--seats"); seats_arg = int(argv[i + 1]); del argv[i:i + 2]
    want = argv or ["k_rollout<6>", "k_rollout_tab<6>", "k_rollout_allin_tab<9>"]
    by_seats = {}
    for k in want:
        by_seats.setdefault(int(re.search(r"<(\d+)>", k).group(1)), []).append(k)
    for n, kernels in by_seats.items():
        s = open(asm_file).read() if asm_file and (seats_arg in (None, n)) else assembly(n)
        funcs = split_asm(s)[0]
        names = {re.sub(r"\(.*", "", subprocess.run(["c++filt", m], capture_output=True, text=True).stdout.strip()).replace("void ", ""): m for m in funcs}
        for k in kernels:
            if k not in names:
                sys.exit("%s: no such kernel in the %d-seat object" % (k, n))
            report(k, funcs[names[k]].split(".amdhsa_")[0])
