#!/usr/bin/env python3
"""Expected range-vs-range sums from the REAL reference: imports pokerl.judger.eval_hand / compare_rankings (read-only, from the reference
checkout given as argv[1] or $POKERL_REFERENCE; build container only) and, for a few spots, decides every ordered pair of disjoint holdings
on every completion of the board exactly as the definition says (pokerl_hip.h "Range vs range"): winners = compare_rankings([eval_hand(board
+ hero holding), eval_hand(board + villain holding)]), the hero is index 0.  No sort, no comparison of ranking words.
Writes rvr_ref.json next to this file: data only -- per spot the valid holding indices and win / tie / tot under uniform weights and under
one recorded u16 weight vector."""
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
    sys.exit("usage: make_rvr_golden.py <path of the reference checkout>")
sys.path.insert(0, REF)

from pokerl.cards import Card  # noqa: E402
from pokerl.judger import compare_rankings, eval_hand  # noqa: E402

CANON = [((c % 4) << 4) | (c // 4) for c in range(52)]
INDEX = {v: k for k, v in enumerate(CANON)}


def hidx(a, b):
    return b * (b - 1) // 2 + a


def enumerate_spot(board, dead, weights):
    gone = {INDEX[c] for c in board} | set(dead)
    pool = [k for k in range(52) if k not in gone]
    k = 5 - len(board)
    known = [Card(c) for c in board]
    holdings = list(itertools.combinations(pool, 2))
    acc = {h: [0, 0, 0, 0] for h in holdings}                        # win, tie under ones; win, tie under `weights`
    for rest in itertools.combinations(pool, k):
        full = known + [Card(CANON[c]) for c in rest]
        live = [h for h in holdings if h[0] not in rest and h[1] not in rest]
        rank = {h: eval_hand(full + [Card(CANON[h[0]]), Card(CANON[h[1]])]) for h in live}   # every holding: once per completion
        for h in live:
            a = acc[h]
            for v in live:
                if v[0] in h or v[1] in h:
                    continue
                winners = compare_rankings([rank[h], rank[v]])
                winners = winners[1] if isinstance(winners, tuple) else winners
                w = weights[hidx(*v)]
                if list(winners) == [0]:
                    a[0] += 1
                    a[2] += w
                elif len(winners) == 2:
                    a[1] += 1
                    a[3] += w
    boards = math.comb(len(pool) - 4, k)
    tot = [boards * sum(1 for v in holdings if v[0] not in h and v[1] not in h) for h in holdings]
    tot_w = [boards * sum(weights[hidx(*v)] for v in holdings if v[0] not in h and v[1] not in h) for h in holdings]
    return dict(pool=len(pool), boards=boards, h=[hidx(*h) for h in holdings],
                win=[acc[h][0] for h in holdings], tie=[acc[h][1] for h in holdings], tot=tot,
                win_w=[acc[h][2] for h in holdings], tie_w=[acc[h][3] for h in holdings], tot_w=tot_w)


def cards(names):
    return [Card(c).value for c in names]


def leave(board, pool):
    """A dead mask that leaves `pool` cards: the first cards of the canonical order that the board does not use."""
    used = {INDEX[c] for c in board}
    free = [k for k in range(52) if k not in used]
    return free[:len(free) - pool]


def main():
    rnd = random.Random(0x525652)
    weights = [rnd.randrange(65536) for _ in range(1326)]
    for i in rnd.sample(range(1326), 200):
        weights[i] = 0
    for i in rnd.sample(range(1326), 100):
        weights[i] = 65535
    spots = [
        ("a full-pool river", cards(["2S", "9C", "KD", "7H", "4D"]), []),
        ("a river whose board is a royal flush", cards(["AS", "KS", "QS", "JS", "TS"]), []),
        ("a paired river board", cards(["2S", "9C", "KD", "7H", "7S"]), []),
        ("a turn with a dead mask that leaves 14 pool cards", cards(["7S", "8D", "AS", "2C"]), 14),
        ("a flop with a dead mask that leaves 10 pool cards", cards(["KS", "8D", "3H"]), 10),
        ("the smallest river pool", cards(["5C", "6D", "QH", "QS", "AC"]), 4),
        ("the smallest turn pool", cards(["5C", "6D", "QH", "QS"]), 5),
        ("the smallest flop pool", cards(["5C", "6D", "QH"]), 6),
    ]
    out = []
    for name, board, dead in spots:
        dead = leave(board, dead) if isinstance(dead, int) else dead
        got = enumerate_spot(board, dead, weights)
        out.append(dict(name=name, board=board, dead=sum(1 << k for k in dead), **got))
        print("%-55s P=%2d boards=%4d holdings=%4d" % (name, got["pool"], got["boards"], len(got["h"])), flush=True)
    assert [s["pool"] for s in out] == [47, 47, 47, 14, 10, 4, 5, 6]
    royal = out[1]
    assert max(royal["tie"]) > 500                                   # large groups of equal keys
    with open(os.path.join(HERE, "rvr_ref.json"), "w") as f:
        json.dump(dict(holdings=1326, weights=weights, spots=out), f, separators=(",", ":"))


if __name__ == "__main__":
    main()
