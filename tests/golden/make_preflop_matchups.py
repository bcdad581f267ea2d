"""Writes tests/golden/preflop_matchups.json: pre-flop matchups counted on the CPU by tests/preflop_spec.py (oracle.loader.eval_hands and the
literal compare_rankings loop over all 1 712 304 boards of each; about 2 s per matchup).  No device code has any part in it.
    python tests/golden/make_preflop_matchups.py
Each entry: the two holdings as Card.value bytes and as indices h, o, and win[h][o], tie[h][o], win[o][h]."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import preflop_spec as PS        # noqa: E402

RANKS = "A23456789TJQK"          # the low nibble of the Card.value byte: ONE (the ace) = 0 .. KING = 12 (enums.CardRank)
SUITS = "SHDC"                   # suit numbers 0 .. 3 of the Card.value byte's high nibble


def v(card):
    return (SUITS.index(card[1]) << 4) | RANKS.index(card[0])


MATCHUPS = [
    ("witness 1: 54s v KQo, spades v hearts and diamonds", [0x04, 0x03], [0x1C, 0x2B]),
    ("witness 2: 54s v KQo, the suits renamed -- another result", [0x34, 0x33], [0x0C, 0x1B]),
    ("pair v pair: AA v KK", [v("AS"), v("AH")], [v("KS"), v("KH")]),
    ("pair v overcards: QQ v AKs", [v("QC"), v("QD")], [v("AH"), v("KH")]),
    ("dominated: AK v AQ", [v("AS"), v("KC")], [v("AD"), v("QH")]),
    ("dominated, suited: KQs v KJs", [v("KS"), v("QS")], [v("KH"), v("JH")]),
    ("adjacent holdings: h = 1224 {48, 49} v h = 1225 {0, 50}", PS.CANON_V[[48, 49]].tolist(), PS.CANON_V[[0, 50]].tolist()),
    ("adjacent holdings: h = 55 {0, 11} v h = 54 {9, 10}", PS.CANON_V[[0, 11]].tolist(), PS.CANON_V[[9, 10]].tolist()),
    ("holding 0 v holding 1325", PS.CANON_V[[0, 1]].tolist(), PS.CANON_V[[50, 51]].tolist()),
    ("holding 1325 v holding 0", PS.CANON_V[[50, 51]].tolist(), PS.CANON_V[[0, 1]].tolist()),
    ("the same ranks: AKs v AKo (mostly ties)", [v("AS"), v("KS")], [v("AH"), v("KD")]),
    ("the same ranks, four suits: 72o v 72o", [v("7S"), v("2C")], [v("7D"), v("2H")]),
    ("one-gapper below the 7 v pair: 64s v 55", [v("6D"), v("4D")], [v("5S"), v("5C")]),
    ("one-gapper below the 7, off suit: 53o v A2s", [v("5H"), v("3S")], [v("AC"), v("2C")]),
    ("wheel cards: A5s v 43s", [v("AD"), v("5D")], [v("4C"), v("3C")]),
    ("low pair v low connectors: 22 v 32o", [v("2S"), v("2H")], [v("3C"), v("2D")]),
]


def main():
    out = []
    for name, a, b in MATCHUPS:
        h, o = PS.holding_of_values(*a), PS.holding_of_values(*b)
        win, tie, lose = PS.pair_counts(h, o)
        assert win + tie + lose == PS.PAIR_BOARDS
        out.append(dict(name=name, hero=[int(x) for x in a], villain=[int(x) for x in b], h=h, o=o, win=win, tie=tie, lose=lose))
        print(out[-1], flush=True)
    with open(os.path.join(HERE, "preflop_matchups.json"), "w") as f:
        json.dump(dict(boards=PS.PAIR_BOARDS, matchups=out), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
