#!/usr/bin/env python3
"""Exhaustive pin of the PARTIAL-hand evaluator: runs the REAL reference pokerl.judger.eval_hand (imported read-only from
/root/reference; build container only) on every hand of 0 .. 6 distinct cards (23 251 684 hands) and on the hands that repeat
cards, and writes position-sensitive digests to evaln_digest.json.  Which hands, in which order, and how the results are folded
is defined once, in tests/evaln_spec.py; the sibling of make_eval_digest.py (all seven-card hands).

    PROCS=16 python tests/golden/make_evaln_digest.py        # minutes; the output has no timestamps: a rerun is byte-identical
"""
import json
import multiprocessing as mp
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

import evaln_spec as S  # noqa: E402

SLICE = 50000          # hands per task


def ref_words(cards, k):
    from pokerl.cards import Card
    from pokerl.judger import eval_hand, get_kickers_value
    deck = {}
    out = np.zeros(len(cards), np.uint32)
    for i, row in enumerate(cards[:, :k].tolist()):
        rank, kick = eval_hand([deck.get(v) or deck.setdefault(v, Card(v)) for v in row])
        out[i] = (len(kick) << 24) | (int(rank) << 20) | get_kickers_value(kick)
    return out


_SETS = {}


def work(task):
    kind, k, a, lo, hi = task
    if kind == "distinct":
        cards = S.hands_of_first(k, a)[0] if k else np.full((1, 7), S.PAD, np.uint8)
    else:
        if not _SETS:
            _SETS.update((name, c) for name, _, c in S.multiset_sets())
        cards = _SETS[kind]
    return task, ref_words(cards[lo:hi], k)


def main():
    procs = int(os.environ.get("PROCS", "8"))
    tasks = [("distinct", 0, 0, 0, 1)]
    for k in S.DISTINCT_K:
        for a in range(52):
            n = S.count_of_first(k, a)
            tasks += [("distinct", k, a, lo, min(lo + SLICE, n)) for lo in range(0, n, SLICE)]
    sets = S.multiset_sets()
    for name, k, cards in sets:
        tasks += [(name, k, 0, lo, min(lo + SLICE, len(cards))) for lo in range(0, len(cards), SLICE)]
    tasks.sort(key=lambda t: t[3] - t[4])        # long tasks first
    acc = {k: S.Acc() for k in S.DISTINCT_K}
    per_first = {k: [0] * 52 for k in S.DISTINCT_K}
    macc = {name: S.Acc() for name, _, _ in sets}
    done = 0
    with mp.Pool(procs) as pool:
        for (kind, k, a, lo, hi), v in pool.imap_unordered(work, tasks, chunksize=1):
            if kind == "distinct":
                part = acc[k].add(v, S.offset_of_first(k, a) + lo)
                if k:
                    per_first[k][a] = (per_first[k][a] + part) % (1 << 64)
            else:
                macc[kind].add(v, lo)
            done += hi - lo
            print("\r%d hands" % done, end="", file=sys.stderr)
    out = dict(note="reference pokerl.judger.eval_hand; definition: tests/evaln_spec.py; made by tests/golden/make_evaln_digest.py",
               distinct={}, multiset={})
    for k in S.DISTINCT_K:
        rec = acc[k].record()
        rec["per_first_card"] = ["%016x" % x for x in per_first[k]]
        assert rec["hands"] == sum(S.count_of_first(k, a) for a in range(52)) + (k == 0)
        out["distinct"][str(k)] = rec
    for name, k, cards in sets:
        rec = macc[name].record()
        rec["ncards"] = k
        rec["repeat_share"] = round(S.repeat_share(cards, k), 6)
        assert rec["hands"] == len(cards)
        if name.startswith("gen"):
            assert rec["repeat_share"] >= 0.5, (name, rec["repeat_share"])   # the condition of the generated sets
        out["multiset"][name] = rec
    with open(os.path.join(HERE, "evaln_digest.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("\n" + " ".join("%s:%s" % (k, r["digest"]) for k, r in out["distinct"].items()))


if __name__ == "__main__":
    main()
