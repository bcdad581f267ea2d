#!/usr/bin/env python3
"""Range against range on one river board (pk_equity_rvr): what a solver's terminal node needs.  Two ranges over the fixed 1 326 holdings
(pokerl_amd.holding_index): the hero's range u and the opponent's range w, both uint16 weights.  One call gives, for EVERY holding h the hero
can have, win[h] / tie[h] / tot[h] = the weight of the opponent's range h beats / ties / meets (card removal included: an opponent holding
that shares a card with h is not met); strength[h] = (win + tie / 2) / tot is the per-holding value, and .against(u) the one number
"hero's range against the opponent's range".  Every holding is ranked once per completion of the board and ordered by a sort; the old way,
pokerl_amd.range_equity per hero holding, is checked against it for a few holdings.

    python examples/range_vs_range.py [board="KS 9D 7D 4C 2H"]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pokerl_amd  # noqa: E402

board = (sys.argv[1] if len(sys.argv) > 1 else "KS 9D 7D 4C 2H").split()
RANKS = "A23456789TJQK"


def name(h):
    return " ".join(RANKS[int(c) & 15] + "SHDC"[int(c) >> 4] for c in pokerl_amd.HOLDINGS[h])


def high(c):
    return (int(c) & 15) or 13                                       # rank0 0 = ace, high


# the hero: pairs and two cards ten or better; the opponent: anything, suited hands twice as often
hero = np.array([2 if high(a) == high(b) else int(min(high(a), high(b)) >= 9) for a, b in pokerl_amd.HOLDINGS], np.uint16)
villain = np.array([2 if (int(a) >> 4) == (int(b) >> 4) else 1 for a, b in pokerl_amd.HOLDINGS], np.uint16)
r = pokerl_amd.range_vs_range(board, weights=villain)
s = r.strength                                                       # nan where a holding is not possible on this board
mine = np.flatnonzero((hero > 0) & r.valid)
order = mine[np.argsort(-s[mine])]
print("board %s: %d holdings possible, %d of them in the hero's range" % (" ".join(board), int(r.valid.sum()), len(mine)))
for h in list(order[:5]) + list(order[-3:]):
    print("  %s  strength %.4f  (beats %d, ties %d of weight %d)" % (name(h), s[h], r.win[h], r.tie[h], r.tot[h]))
print("hero's range against the opponent's range: %.5f;  any two cards against it: %.5f" % (r.against(hero), r.against()))
for h in order[:3]:                                                  # the identity: row h is range_equity of hero = h
    one = pokerl_amd.range_equity([int(c) for c in pokerl_amd.HOLDINGS[h]], board, weights=villain)
    assert [int(x) for x in one.agg] == [int(r.win[h]), int(r.tie[h]), int(r.tot[h])]
