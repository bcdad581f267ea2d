#!/usr/bin/env python3
"""Which GPU kernels does the working tree compile differently from <git-rev>?  Both trees' device code -- every translation unit of build.SOURCES as
build.py compiles it: pk_tables.hip per seat count, pk_equity_ranged.hip and pk_ev_ranged.hip per LDS size class (build.EQW_CLASSES), every other unit once -- goes to
assembly with the library's build flags and is compared per kernel (body and kernel descriptor) and per device constant object (g_nth,
g_env_transitions); function order, local label numbers and the __hip_cuid_* symbol do not count.  Exit status 1 on a difference.
usage: tools/isa_diff.py <git-rev> [N ...]      (default N = every seat count)"""
import os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pokerl_amd import build
from isa_report import split_asm

def symbols(tree, src, flags):
    if not os.path.exists(os.path.join(tree, "pokerl_amd", "csrc", src)):       # a translation unit <git-rev> does not have yet: all its symbols are new
        return None
    r = subprocess.run([build.hipcc()] + flags + ["--cuda-device-only", "-S", os.path.join(tree, "pokerl_amd", "csrc", src), "-o", "-"], capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr)
    funcs, objs = split_asm(re.sub(r"(\.L[A-Za-z_]+)\d+", r"\1", r.stdout))
    return {**funcs, **{k: v for k, v in objs.items() if not k.startswith("__hip_cuid_")}}

if __name__ == "__main__":
    rev, seats = sys.argv[1], [int(a) for a in sys.argv[2:]] or build.SEATS
    units = [("pk_tables.hip -DPK_SEATS=%d" % n, "pk_tables.hip", build.table_flags(n) + ["-DPK_SEATS=%d" % n]) for n in sorted(seats, reverse=True)]
    units += [("pk_equity_ranged.hip -DPK_EQW_CLASS=%d" % rc, "pk_equity_ranged.hip", build.COMPILE_FLAGS + ["-DPK_EQW_CLASS=%d" % rc]) for rc in build.EQW_CLASSES]
    units += [("pk_ev_ranged.hip -DPK_EVW_CLASS=%d" % rc, "pk_ev_ranged.hip", build.COMPILE_FLAGS + ["-DPK_EVW_CLASS=%d" % rc]) for rc in build.EQW_CLASSES]
    units += [(s, s, build.COMPILE_FLAGS) for s in build.SOURCES if s not in ("pk_tables.hip", "pk_equity_ranged.hip", "pk_ev_ranged.hip")]
    with tempfile.TemporaryDirectory() as old, ThreadPoolExecutor(int(os.environ.get("PK_BUILD_JOBS", "0")) or min(8, os.cpu_count() or 1)) as ex:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "pokerl_amd/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", old], input=tar, check=True)
        res = list(ex.map(lambda j: symbols(j[0], j[2], j[3]), [(tree,) + u for u in units for tree in (old, ROOT)]))
    compared = same = 0
    for (unit, _, _), a, b in zip(units, res[0::2], res[1::2]):
        if a is None:
            print("%-40s %3d symbols, new: %s does not have it" % (unit, len(b), rev))
            continue
        differ = sorted(k for k in a.keys() & b.keys() if a[k] != b[k])
        compared += len(a.keys() | b.keys()); same += len(a.keys() & b.keys()) - len(differ)
        print("%-40s %3d symbols, %3d identical" % (unit, len(a.keys() | b.keys()), len(a.keys() & b.keys()) - len(differ)))
        for tag, names in (("differs", differ), ("only in " + rev, sorted(a.keys() - b.keys())), ("only in the working tree", sorted(b.keys() - a.keys()))):
            for k in names:
                print("    %s: %s" % (tag, subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip()))
    print("%d kernels and constant objects compared, %d identical" % (compared, same))
    sys.exit(compared != same)
