#!/usr/bin/env python3
"""A river subgame solved on the device (pk_solve_river): two ranges over the fixed 1 326 holdings, a betting tree built by
pokerl_amd.river_tree (pot 100, 400 behind, bets of half the pot and the pot, a bet and one raise), CFR+ in exact integers -- the same call
gives the same bytes on any grid.  Printed: each player's value in chips, how much a best response would gain against the strategy
(the exploitability) as the iterations grow, and what player 0 does at the root with a few holdings.

    python examples/river_solve.py [board="KS 9D 7D 4C 2H"]
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


# player 0 (first to act): pairs and two cards ten or better; player 1: anything, suited hands twice as often
first = np.array([2 if high(a) == high(b) else int(min(high(a), high(b)) >= 9) for a, b in pokerl_amd.HOLDINGS], np.uint16)
second = np.array([2 if (int(a) >> 4) == (int(b) >> 4) else 1 for a, b in pokerl_amd.HOLDINGS], np.uint16)
first, second = first * 30000, second * 30000                       # a reach is weight << 4 and every split rounds down: use the sixteen bits
tree = pokerl_amd.river_tree(100, 400)
print("board %s; %r" % (" ".join(board), tree))
for iters in (16, 64, 256):
    s = pokerl_amd.solve_river(board, [first, second], tree, iters)
    print("  %4d iterations: value %.3f / %.3f chips, exploitability %.4f chips" % ((iters,) + s.ev + (s.exploitability,)))
root = tree.decision_nodes[0]
kids = [int(c) for c in tree.child[root] if c != 0xFF]
p = s.probabilities(root)
mine = np.flatnonzero((first > 0) & s.valid)
order = mine[np.argsort(-s.value[0][mine])]
print("player 0 at the root: " + ", ".join(tree.label(c) for c in kids))
for h in list(order[:4]) + list(order[-3:]):
    print("  %s  %s" % (name(h), "  ".join("%.3f" % x for x in p[:, h])))
assert (s.strategy.astype(np.int64).sum(axis=1)[:, s.valid] == 32768).all() and (s.br >= s.value).all()
