#!/usr/bin/env python3
"""Records what the entry points of the equity family (the seven spot families in their four forms, the six clustering calls: 34 in all)
answer to bad arguments: the return code and the pk_last_error(NULL) text of every call, into equity_refusals.json next to this file.  Every
call listed here is refused before any device is looked at, so the script runs without a GPU, on the built library.
The parameter names come from include/pokerl_hip.h.  A call starts from arguments that would pass (every pointer a small zeroed buffer, no
handle, no stream) with one or two of them replaced.  Before each call the thread's error text is set to MARK by a call that is known to be
refused, so a call that returns without writing a text (a NULL handle) records MARK, whatever ran before it.
Fixture: {"mark": [fn, args], "calls": [{"fn", "args", "rc", "error"}]}; an argument is an integer, "buf" (the zeroed buffer) or null."""
import json
import os
import re
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

FAMILIES = ("equity", "equity_ev", "equity_sampled", "equity_ranged", "equity_range", "equity_rvr", "equity_hist")
CLUSTER = ("pk_hist_cluster_seed", "pk_hist_cluster_assign", "pk_hist_cluster")
MARK = ["pk_eval7_prefix", [0, 0, 0, 0, None, None]]          # "pk_eval7_prefix: bad argument"
BUF_BYTES = 4096                                                # (what the one check that reads an array reads: 4 rows of 4 bins)
BASE = {"device": 0, "num_players": 2, "m": 1, "n": 2, "nbins": 4, "K": 1, "iters": 1, "samples": 64, "seed": 1, "nonce": 0, "num_ranges": 0,
        "weights_per_spot": 0, "range_per_table": 0, "observer": 0, "h": None, "stream": None}


def parameters():
    """{entry point: [parameter name, ...]} with the device forms' _d suffix removed"""
    header = open(os.path.join(ROOT, "include", "pokerl_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint (pk_\w+)\s*\(([^)]*)\)\s*;", header):
        names = [re.search(r"(\w+)\s*$", a).group(1) for a in args.split(",")]
        out[name] = [n[:-2] if n.endswith("_d") and n[:-2] not in names else n for n in names]   # (samples_d beside samples keeps its name)
    return out


def cases():
    P = parameters()
    out = []

    def call(fn, **changed):
        assert set(changed) <= set(P[fn]), (fn, changed)
        out.append([fn, [changed[n] if n in changed else BASE.get(n, "buf") for n in P[fn]]])

    for fam in FAMILIES:
        seats = "num_players" in P["pk_" + fam]
        sampled = fam in ("equity_sampled", "equity_ranged")
        inputs = {"equity": ("holes", "board", "nboard", "live"), "equity_ev": ("holes", "board", "nboard", "live", "bets", "status"),
                  "equity_sampled": ("holes", "board", "nboard", "live"), "equity_ranged": ("holes", "board", "nboard", "live"),
                  "equity_range": ("hero", "board", "nboard"), "equity_rvr": ("board", "nboard"), "equity_hist": ("board", "nboard")}[fam]
        for fn in ("pk_%s_d" % fam, "pk_" + fam):
            if seats:
                for n in (1, 17, -3):
                    call(fn, num_players=n)
                call(fn, num_players=6, m=2 ** 31)
            else:
                call(fn, m=2 ** 31)
            for name in inputs:
                call(fn, **{name: None})
            # the 32-bit task bound
            if fam == "equity":
                for m in (131 * 10 ** 6, 2 ** 31 - 1):
                    call(fn, m=m)
            if fam == "equity_ev":
                call(fn, m=2 ** 31 - 1)
                call(fn, num_players=16, m=2 ** 27)
            if sampled:
                for samples in (0, 2 ** 24 + 1, 2 ** 32 - 1):
                    call(fn, num_players=6, samples=samples)
                call(fn, m=2 ** 14, samples=2 ** 24)
                call(fn, m=2 ** 31 - 1, samples=129)
            if fam == "equity_ranged":
                for ranges in (17, 2 ** 32 - 1):
                    call(fn, num_players=6, num_ranges=ranges)
                call(fn, num_players=6, num_ranges=4, weights=None)
            if fam == "equity_hist":
                for nbins in (0, 33, -1):
                    call(fn, nbins=nbins)
                call(fn, m=0, nbins=0, board=None, nboard=None)                  # (even with no spot)
        for fn in ("pk_table_%s_d" % fam, "pk_table_" + fam):                    # no handle: nothing else is looked at, no text is written
            call(fn, m=4)
            if "observer" in P[fn]:
                for observer in (-1, -2, -3, 16):
                    call(fn, m=4, observer=observer)
            call(fn, m=2 ** 31, **({"samples": 0} if sampled else {}), **({"nbins": 0} if fam == "equity_hist" else {}),
                 **({"num_ranges": 17} if fam == "equity_ranged" else {}), **({"status": None} if fam == "equity_ev" else {}))
    for base in CLUSTER:
        for fn in (base + "_d", base):
            for nbins in (0, 33):
                call(fn, nbins=nbins)
            for n in (0, 2 ** 31):
                call(fn, n=n)
            for K in (0, 4097):
                call(fn, K=K)
            if "assign" not in fn:
                call(fn, K=3)                                                    # more than the rows (assign labels any number of rows with any K)
            if "iters" in P[fn]:
                for iters in (0, 1025):
                    call(fn, iters=iters)
            for name in ("hist", "centroids") + (("label",) if "label" in P[fn] else ()):
                call(fn, **{name: None})
            if fn in ("pk_hist_cluster_seed", "pk_hist_cluster"):                # the host forms see the rows: the buffer's are all empty
                call(fn, n=4, K=1)
    return out


def run(lib, calls, mark=MARK):
    """[(rc, error text)] of the calls, each after the marking call"""
    import numpy as np
    L = lib.lib()
    buf = np.zeros(BUF_BYTES, np.uint8)

    def invoke(fn, args):
        return getattr(L, fn)(*[lib.ptr(buf) if a == "buf" else a for a in args])

    out = []
    for fn, args in calls:
        invoke(*mark)
        rc = invoke(fn, args)
        out.append((rc, L.pk_last_error(None).decode()))
    return out


if __name__ == "__main__":
    from pokerl_amd import _lib, build
    if not os.environ.get("POKERL_HIP_LIB"):                                     # (set: the library of another commit, recorded as it is)
        build.build_lib()
    todo = cases()
    got = run(_lib, todo)
    for (fn, args), (rc, err) in zip(todo, got):
        assert rc == _lib.PK_E_INVALID_ARG, (fn, args, rc, err)
    doc = {"mark": MARK, "calls": [{"fn": fn, "args": args, "rc": rc, "error": err} for (fn, args), (rc, err) in zip(todo, got)]}
    path = os.path.join(HERE, "equity_refusals.json")
    with open(path, "w") as f:
        f.write("{\"mark\": %s,\n \"calls\": [\n" % json.dumps(doc["mark"]))
        f.write(",\n".join("  " + json.dumps(c) for c in doc["calls"]))
        f.write("\n ]}\n")
    print("%s: %d calls, %d entry points, %d distinct texts" % (path, len(todo), len({c[0] for c in todo}), len({e for _, e in got})))
