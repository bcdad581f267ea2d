#!/usr/bin/env python3
"""Expected showdown-equity counts from the REAL reference: imports pokerl.judger.eval_hand / compare_rankings (read-only, from the
reference checkout given as argv[1] or $POKERL_REFERENCE; build container only) and enumerates the boards of a few dozen small spots
(river, turn, flop; 2, 3, 6, 9, 16 seats; folded seats; unknown 0xFF hole cards) exactly as the definition says (pokerl_hip.h
"Showdown equity"): v[p] = eval_hand(board + hole[p]) for a live seat, (NONE, []) otherwise; winners = compare_rankings(v).
Writes equity_ref.json next to this file: data only.

At least three spots with >= 3 live seats must have counts that CHANGE if judger.py:148 (`kicker = best_kicker`) raised best_kicker
instead; the generator asserts it and marks those spots ("line148": true).
"""
import itertools
import json
import os
import random
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("POKERL_REFERENCE", "")
if not os.path.isdir(os.path.join(REF, "pokerl")):
    sys.exit("usage: make_equity_golden.py <path of the reference checkout>")
sys.path.insert(0, REF)

from pokerl.cards import Card  # noqa: E402
from pokerl.enums import HandRanking  # noqa: E402
from pokerl.judger import compare_rankings, eval_hand, get_kickers_value  # noqa: E402

SHARE_UNIT = 720720
UNKNOWN = 0xFF
CANON = [((c % 4) << 4) | (c // 4) for c in range(52)]


def fixed_compare(rankings):
    """compare_rankings with line 148 'fixed' (best_kicker raised): only to detect the spots that depend on the line as it is."""
    winners, best_rank, best_kicker = [], HandRanking.NONE, 0
    for idx, (rank, kickers) in enumerate(rankings):
        kicker = get_kickers_value(kickers)
        if rank < best_rank:
            best_rank, best_kicker, winners = rank, kicker, [idx]
        elif rank == best_rank:
            if kicker > best_kicker:
                best_kicker, winners = kicker, [idx]
            elif kicker == best_kicker:
                winners.append(idx)
    return winners


def enumerate_spot(holes, board, live, compare):
    n = len(holes)
    dead = set(board) | {c for h in holes for c in h if c != UNKNOWN}
    pool = [c for c in CANON if c not in dead]
    win, tie, share, boards = [0] * n, [0] * n, [0] * n, 0
    for rest in itertools.combinations(pool, 5 - len(board)):
        full = [Card(c) for c in board + list(rest)]
        v = [eval_hand(full + [Card(c) for c in holes[p]]) if (live >> p) & 1 else eval_hand([]) for p in range(n)]
        winners = compare(v)
        winners = winners[1] if isinstance(winners, tuple) else winners
        boards += 1
        for p in winners:
            if len(winners) == 1:
                win[p] += 1
            else:
                tie[p] += 1
            share[p] += SHARE_UNIT // len(winners)
    assert sum(share) == SHARE_UNIT * boards
    return dict(win=win, tie=tie, share=share, boards=boards)


def random_spot(rng, n, nb):
    deck = rng.sample(CANON, 5 + 2 * n)
    board, holes = deck[:nb], [deck[5 + 2 * p:7 + 2 * p] for p in range(n)]
    live = rng.randrange(1, 1 << n)
    if n >= 3 and bin(live).count("1") < 3 and rng.random() < 0.7:
        live |= rng.randrange(1, 1 << n) | rng.randrange(1, 1 << n)
    for p in range(n):
        if not (live >> p) & 1 and rng.random() < 0.5:
            holes[p] = [UNKNOWN, UNKNOWN]
    return holes, board, live


def main():
    rng = random.Random(0x45515549)
    spots, dependent = [], 0
    plan = [(n, nb) for n in (2, 3, 6, 9, 16) for nb in (5, 5, 4, 4, 3)] + [(3, 5)] * 6 + [(6, 5)] * 6 + [(9, 4)] * 2
    for n, nb in plan:
        holes, board, live = random_spot(rng, n, nb)
        got = enumerate_spot(holes, board, live, compare_rankings)
        dep = False
        if bin(live).count("1") >= 3:
            alt = enumerate_spot(holes, board, live, fixed_compare)
            dep = any(alt[k] != got[k] for k in ("win", "tie", "share"))
        dependent += dep
        spots.append(dict(n=n, holes=holes, board=board, live=live, line148=dep, **got))
    # hand-made: three live seats of one rank class, the first with the lowest kickers, the second the highest, the third in between --
    # the reference's loop lets the THIRD take the pot (best_kicker stays the first seat's)
    for board, holes in [(["2S", "7D", "9C", "JH", "KS"], [["3D", "4C"], ["AD", "QC"], ["AC", "5D"]]),
                         (["2S", "2D", "9C", "JH", "KS"], [["3D", "4C"], ["AD", "QC"], ["QD", "5D"], ["7H", "8H"]])]:
        b = [Card(c).value for c in board]
        h = [[Card(c).value for c in x] for x in holes]
        live = (1 << len(h)) - 1
        got = enumerate_spot(h, b, live, compare_rankings)
        alt = enumerate_spot(h, b, live, fixed_compare)
        dep = any(alt[k] != got[k] for k in ("win", "tie", "share"))
        assert dep, "the hand-made spots must depend on line 148"
        dependent += dep
        spots.append(dict(n=len(h), holes=h, board=b, live=live, line148=True, **got))
    assert dependent >= 3, "too few spots depend on judger.py:148 (%d)" % dependent
    with open(os.path.join(HERE, "equity_ref.json"), "w") as f:
        json.dump(dict(share_unit=SHARE_UNIT, spots=spots), f, separators=(",", ":"))
    print("%d spots, %d depend on line 148" % (len(spots), dependent))


if __name__ == "__main__":
    main()
