#!/usr/bin/env python3
"""A turn subgame solved on the device (pk_solve_turn): two ranges over the fixed 1 326 holdings on a four-card board, a betting tree for
the turn and the river built by pokerl_amd.turn_tree (pot 100, 400 behind, pot-size bets, one bet a street), the river card a chance node,
CFR+ in exact integers -- the same call gives the same bytes on any grid.  Printed: each player's value in chips, the exploitability as
the iterations grow, what player 0 does at the root with a few holdings, and what it does on two river cards after check, check.

    python examples/turn_solve.py [board="KS 9D 7D 4C"] [river cards="2H 8D"]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pokerl_amd  # noqa: E402

board = (sys.argv[1] if len(sys.argv) > 1 else "KS 9D 7D 4C").split()
rivers = (sys.argv[2] if len(sys.argv) > 2 else "2H 8D").split()
RANKS = "A23456789TJQK"


def name(h):
    return " ".join(RANKS[int(c) & 15] + "SHDC"[int(c) >> 4] for c in pokerl_amd.HOLDINGS[h])


def high(c):
    return (int(c) & 15) or 13                                       # rank0 0 = ace, high


# player 0 (first to act): pairs and two cards ten or better; player 1: anything, suited hands twice as often
first = np.array([2 if high(a) == high(b) else int(min(high(a), high(b)) >= 9) for a, b in pokerl_amd.HOLDINGS], np.uint16)
second = np.array([2 if (int(a) >> 4) == (int(b) >> 4) else 1 for a, b in pokerl_amd.HOLDINGS], np.uint16)
first, second = first * 30000, second * 30000                       # a reach is weight << 1 and every split rounds down: use the sixteen bits
tree = pokerl_amd.turn_tree(100, 400, (1.0,), 1)
print("board %s; %r" % (" ".join(board), tree))
for iters in (16, 64, 256):
    s = pokerl_amd.solve_turn(board, [first, second], tree, iters, river_strategy=iters == 256)
    print("  %4d iterations: value %.3f / %.3f chips, exploitability %.4f chips" % ((iters,) + s.ev + (s.exploitability,)))
mine = np.flatnonzero((first > 0) & s.valid)
order = mine[np.argsort(-s.value[0][mine])]
show = list(order[:4]) + list(order[-3:])


def table(node, p):
    kids = [int(c) for c in tree.child[node] if c != 0xFF]
    print("    " + ", ".join(tree.label(c)[len(tree.label(node)):].strip() for c in kids))
    for h in show:
        if not np.isnan(p[0, h]):
            print("    %s  %s" % (name(h), "  ".join("%.3f" % x for x in p[:, h])))


root = tree.decision_nodes[0]
print("player 0 at the root:")
table(root, s.probabilities(root))
after = next(v for v in tree.river_decision_nodes if tree.label(v) == "0:check 1:check deal")
for card in rivers:
    print("player 0 after check, check and the %s:" % card)
    table(after, s.probabilities(after, river_card=card))
assert (s.strategy.astype(np.int64).sum(axis=1)[:, s.valid] == 32768).all() and (s.br >= s.value).all()
