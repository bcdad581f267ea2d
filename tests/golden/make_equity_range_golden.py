#!/usr/bin/env python3
"""Expected range-equity counts from the REAL reference: imports pokerl.judger.eval_hand / compare_rankings (read-only, from the reference
checkout given as argv[1] or $POKERL_REFERENCE; build container only) and, for every valid holding of a few spots, enumerates the
completions of the board exactly as the definition says (pokerl_hip.h "Range equity"): v = [eval_hand(board + hero),
eval_hand(board + holding)], winners = compare_rankings(v), the hero is index 0.  The villain's hand is evaluated anew for every
(holding, completion) pair -- the sharing the device uses is what this fixture checks.
Writes equity_range_ref.json next to this file: data only, and only the valid holdings (index, win, tie per spot)."""
import itertools
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("POKERL_REFERENCE", "")
if not os.path.isdir(os.path.join(REF, "pokerl")):
    sys.exit("usage: make_equity_range_golden.py <path of the reference checkout>")
sys.path.insert(0, REF)

from pokerl.cards import Card  # noqa: E402
from pokerl.judger import compare_rankings, eval_hand  # noqa: E402

CANON = [((c % 4) << 4) | (c // 4) for c in range(52)]
INDEX = {v: k for k, v in enumerate(CANON)}


def enumerate_spot(hero, board, dead):
    gone = {INDEX[c] for c in hero + board} | set(dead)
    pool = [k for k in range(52) if k not in gone]
    k = 5 - len(board)
    known = [Card(c) for c in board]
    mine = [Card(c) for c in hero]
    hero_rank = {}
    hs, wins, ties, boards = [], [], [], None
    for a, b in itertools.combinations(pool, 2):
        theirs = [Card(CANON[a]), Card(CANON[b])]
        win = tie = n = 0
        for rest in itertools.combinations([c for c in pool if c != a and c != b], k):
            full = known + [Card(CANON[c]) for c in rest]
            if rest not in hero_rank:
                hero_rank[rest] = eval_hand(full + mine)
            winners = compare_rankings([hero_rank[rest], eval_hand(full + theirs)])
            winners = winners[1] if isinstance(winners, tuple) else winners
            n += 1
            win += list(winners) == [0]
            tie += len(winners) == 2
        assert boards in (None, n)
        boards = n
        hs.append(b * (b - 1) // 2 + a)
        wins.append(win)
        ties.append(tie)
    return dict(pool=len(pool), boards=boards, h=hs, win=wins, tie=ties)


def cards(names):
    return [Card(c).value for c in names]


def main():
    spots = [
        ("a full-pool river", cards(["9H", "9D"]), cards(["2S", "9C", "KD", "7H", "7S"]), []),
        ("a full-pool turn", cards(["AD", "QD"]), cards(["2D", "JD", "QS", "5C"]), []),
        # dead: the first 27 cards of the canonical order that the spot does not use -> P = 20
        ("a flop with a dead mask that leaves 20 pool cards", cards(["KH", "KC"]), cards(["KS", "8D", "3H"]), None),
        ("a turn with a dead mask", cards(["5S", "6S"]), cards(["7S", "8D", "AS", "2C"]),
         [INDEX[c] for c in cards(["KD", "KH", "2H", "9C", "QC", "3D", "JH", "4S"])]),
        ("a river whose board is a royal flush", cards(["2D", "3C"]), cards(["AS", "KS", "QS", "JS", "TS"]), []),
        ("a flop where the hero holds the nuts", cards(["AS", "KS"]), cards(["QS", "JS", "TS"]), []),
    ]
    out = []
    for name, hero, board, dead in spots:
        if dead is None:
            used = {INDEX[c] for c in hero + board}
            dead = [k for k in range(52) if k not in used][:27]
        assert not ({INDEX[c] for c in hero + board} & set(dead))
        got = enumerate_spot(hero, board, dead)
        out.append(dict(name=name, hero=hero, board=board, dead=sum(1 << k for k in dead), **got))
        print("%-60s P=%2d boards=%4d holdings=%4d" % (name, got["pool"], got["boards"], len(got["h"])), flush=True)
    assert out[2]["pool"] == 20
    # the royal-flush board: at poker every holding ties.  The reference does not say so for every holding: its straight-flush tracker ends on
    # the LOWEST run of the flush suit (judger.py:56-57), so a villain who adds low spades to the board's A-K-Q-J-T is ranked a mere flush
    # and loses.  The fixture records what the reference says; the hero, who plays the board, never loses.
    royal = out[4]
    assert all(w + t == 1 for w, t in zip(royal["win"], royal["tie"])) and 0 < sum(royal["tie"]) < 990
    print("royal-flush board: %d of %d holdings tie, the hero beats the others" % (sum(royal["tie"]), len(royal["tie"])))
    # ... and the same tracker makes the flopped royal flush less than the nuts on the boards that bring low spades: recorded as the reference has it
    nuts = out[5]
    full = sum(w == nuts["boards"] for w in nuts["win"])
    assert 0 < full and all(w + t <= nuts["boards"] for w, t in zip(nuts["win"], nuts["tie"]))
    print("flopped royal flush: the hero wins every board against %d of %d holdings" % (full, len(nuts["win"])))
    with open(os.path.join(HERE, "equity_range_ref.json"), "w") as f:
        json.dump(dict(holdings=1326, spots=out), f, separators=(",", ":"))


if __name__ == "__main__":
    main()
