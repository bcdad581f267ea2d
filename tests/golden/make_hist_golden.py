#!/usr/bin/env python3
"""Expected strength histograms from the REAL reference: imports pokerl.judger.eval_hand / compare_rankings (read-only, from the reference
checkout given as argv[1] or $POKERL_REFERENCE; build container only) and, for a few small spots, decides every ordered pair of disjoint
holdings on every completion of the board exactly as the definition says (pokerl_hip.h "Strength histograms"): winners =
compare_rankings([eval_hand(board + completion + hero holding), eval_hand(board + completion + villain holding)]), the hero is index 0.
No sort, no comparison of ranking words.  below / equal / den are summed per (hero holding, completion) in Python integers and binned by the
integer rule.
Writes hist_ref.json next to this file: data only -- the recorded weight vectors and per spot the valid holding indices, and per weight
vector `void` and, per number of bins, the non-zero histogram cells as [position of the holding in `h`, bin, count]."""
import itertools
import json
import math
import os
import random
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("POKERL_REFERENCE", "")
if not os.path.isdir(os.path.join(REF, "pokerl")):
    sys.exit("usage: make_hist_golden.py <path of the reference checkout>")
sys.path.insert(0, REF)

from pokerl.cards import Card  # noqa: E402
from pokerl.judger import compare_rankings, eval_hand  # noqa: E402

CANON = [((c % 4) << 4) | (c // 4) for c in range(52)]
INDEX = {v: k for k, v in enumerate(CANON)}
BINS = (1, 2, 7, 32)


def hidx(a, b):
    return b * (b - 1) // 2 + a


def enumerate_spot(board, dead, ranges):
    """ranges: {name: [1326] weights}.  -> per name: void [n] and {bins: sparse cells}."""
    gone = {INDEX[c] for c in board} | set(dead)
    pool = [k for k in range(52) if k not in gone]
    k = 5 - len(board)
    known = [Card(c) for c in board]
    holdings = list(itertools.combinations(pool, 2))
    pos = {h: i for i, h in enumerate(holdings)}
    void = {name: [0] * len(holdings) for name in ranges}
    cells = {name: {b: {} for b in BINS} for name in ranges}
    for rest in itertools.combinations(pool, k):
        full = known + [Card(CANON[c]) for c in rest]
        live = [h for h in holdings if h[0] not in rest and h[1] not in rest]
        rank = {h: eval_hand(full + [Card(CANON[h[0]]), Card(CANON[h[1]])]) for h in live}   # every holding: once per completion
        for h in live:
            alone, both, met = [], [], []
            for v in live:
                if v[0] in h or v[1] in h:
                    continue
                winners = compare_rankings([rank[h], rank[v]])
                winners = winners[1] if isinstance(winners, tuple) else winners
                met.append(v)
                if list(winners) == [0]:
                    alone.append(v)
                elif len(winners) == 2:
                    both.append(v)
            assert met                                                # P >= k + 4: never empty by count
            for name, w in ranges.items():
                below, equal, den = (sum(w[hidx(*v)] for v in group) for group in (alone, both, met))
                if den == 0:
                    void[name][pos[h]] += 1
                    continue
                for b in BINS:
                    cell = (pos[h], min(b - 1, (b * (2 * below + equal)) // (2 * den)))
                    cells[name][b][cell] = cells[name][b].get(cell, 0) + 1
    completions = math.comb(len(pool) - 2, k)
    cases = {name: dict(void=void[name], hist={str(b): [[i, j, n] for (i, j), n in sorted(cells[name][b].items())] for b in BINS}) for name in ranges}
    for name in ranges:                                               # the row-sum invariant
        for b in BINS:
            total = list(void[name])
            for i, _, n in cases[name]["hist"][str(b)]:
                total[i] += n
            assert total == [completions] * len(holdings), (name, b)
    return dict(pool=len(pool), completions=completions, h=[hidx(*h) for h in holdings], cases=cases), pool


def cards(names):
    return [Card(c).value for c in names]


def leave(board, pool):
    """A dead mask that leaves `pool` cards: the first cards of the canonical order that the board does not use."""
    used = {INDEX[c] for c in board}
    free = [k for k in range(52) if k not in used]
    return free[:len(free) - pool]


def main():
    rnd = random.Random(0x48495354)
    weights = [rnd.randrange(65536) for _ in range(1326)]
    for i in rnd.sample(range(1326), 300):
        weights[i] = 0
    for i in rnd.sample(range(1326), 100):
        weights[i] = 65535
    ones = [1] * 1326
    spots = [
        ("the smallest river pool", cards(["5C", "6D", "QH", "QS", "AC"]), 4),
        ("a river with 10 pool cards", cards(["2S", "9C", "KD", "7H", "7S"]), 10),
        ("the smallest turn pool", cards(["5C", "6D", "QH", "QS"]), 5),
        ("a turn with 9 pool cards", cards(["7S", "8D", "AS", "2C"]), 9),
        ("the smallest flop pool", cards(["5C", "6D", "QH"]), 6),
        ("a flop with 8 pool cards", cards(["KS", "8D", "3H"]), 8),
        ("a flop with 10 pool cards, three to a flush", cards(["KS", "8S", "3S"]), 10),
    ]
    out = []
    for name, board, left in spots:
        dead = leave(board, left)
        # the range that dies: weight only on the holdings that hold the LAST pool card -- a hero who holds that card, and every hero on a
        # completion that deals it, meets no weight at all
        gone = {INDEX[c] for c in board} | set(dead)
        last = max(k for k in range(52) if k not in gone)
        dying = [0] * 1326
        for a in range(last):
            dying[hidx(a, last)] = 1 + a
        got, pool = enumerate_spot(board, dead, dict(ones=ones, random=weights, dying=dying))
        assert max(got["cases"]["dying"]["void"]) > 0 and max(got["cases"]["ones"]["void"]) == 0
        out.append(dict(name=name, board=board, dead=sum(1 << k for k in dead), dying_card=last, **got))
        print("%-50s P=%2d completions=%3d holdings=%3d" % (name, got["pool"], got["completions"], len(got["h"])), flush=True)
    assert [s["pool"] for s in out] == [4, 10, 5, 9, 6, 8, 10]
    with open(os.path.join(HERE, "hist_ref.json"), "w") as f:
        json.dump(dict(holdings=1326, bins=list(BINS), weights=weights, spots=out), f, separators=(",", ":"))


if __name__ == "__main__":
    main()
