#!/usr/bin/env python3
"""Starting-hand strength before the flop, exact (pk_preflop_matchups / pk_table_equity_preflop).  The device counts, once, every ordered pair
of holdings over every five-card board -- each holding ranked once per board, each pair compared on each board -- and keeps the two
[1326, 1326] count tables resident; from then on "how strong is the hand of the seat to act against a range?" is a row gather and a
weighted sum, at any turn (the board is not read: post-flop, VecGame.equity_range answers with the board).

The table is this project's own object: the evaluator it is bit-identical to is NOT invariant under a renaming of suits (a 2-3-4-5-6
straight is missed for some suit orders), so suit-isomorphic matchups differ.  The last lines print two spots that are both "five-four suited
against king-queen off suit" side by side.

    python examples/preflop_strength.py [tables=4096] [seats=6]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pokerl_amd  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
N = int(sys.argv[2]) if len(sys.argv) > 2 else 6
RANKS = "A23456789TJQK"


def name(h):
    return " ".join(RANKS[int(c) & 15] + "SHDC"[int(c) >> 4] for c in pokerl_amd.HOLDINGS[h])


def high(c):
    return (int(c) & 15) or 13                                       # rank nibble 0 = the ace, high


g = pokerl_amd.VecGame(T, num_players=N)
g.reset()
# the opponent's range: pairs and two cards nine or better, suited hands twice as often
villain = np.array([(2 if (int(a) >> 4) == (int(b) >> 4) else 1) * int(high(a) == high(b) or min(high(a), high(b)) >= 8)
                    for a, b in pokerl_amd.HOLDINGS], np.uint16)
any_two = g.equity_preflop()                                         # the seat to act of every table, against any two cards
ranged = g.equity_preflop(weights=villain)
deck, active = g.deck, g.active_player.astype(np.int64)
rows = np.arange(T)
hero = [pokerl_amd.holding_index(int(a), int(b)) for a, b in zip(deck[rows, 5 + 2 * active], deck[rows, 6 + 2 * active])]
order = np.argsort(-any_two.strength)
print("%d tables x %d seats, the seat to act before the flop (status non-zero on %d tables):" % (T, N, int((any_two.status != 0).sum())))
for t in list(order[:4]) + list(order[-3:]):
    print("  table %5d seat %d holds %s: %.4f against any two cards, %.4f against the range" % (t, active[t], name(hero[t]), any_two.strength[t], ranged.strength[t]))

every = pokerl_amd.preflop_range_vs_range(villain)                   # every starting hand against that range, one call
best = np.argsort(-every.strength)[:3]
print("against the range, the best starting hands: " + ", ".join("%s %.4f" % (name(h), every.strength[h]) for h in best))
assert all(abs(every.strength[hero[t]] - ranged.strength[t]) < 1e-15 for t in order[:4])

M = pokerl_amd.preflop_matchups()
print("two suit-isomorphic matchups, %d boards each (hero wins / ties / villain wins):" % M.boards)
for hero_cards, villain_cards in (([0x04, 0x03], [0x1C, 0x2B]), ([0x34, 0x33], [0x0C, 0x1B])):
    h, o = pokerl_amd.holding_index(*hero_cards), pokerl_amd.holding_index(*villain_cards)
    print("  %s v %s: %7d %6d %7d   equity %.6f" % (name(h), name(o), M.win[h, o], M.tie[h, o], M.win[o, h], M.equity[h, o]))
g.close()
