#!/usr/bin/env python3
"""Continual re-solving (pk_solve_turn_resolve, pk_solve_river_resolve): a turn spot is solved on a coarse tree; the river card falls; the
river subgame now in front of the players -- both checked the turn -- is re-solved on a FINER tree from what the turn solve computed at that
node: both players' reaches (node_reach) and, for safe re-solving, the opponent's best-response values there (node_br).  UNSAFE re-solving
is an ordinary solve from the reaches; SAFE re-solving puts the gadget of Burch, Johanson and Bowling (2014) on top of the subgame, in
which the opponent may take the value it was promised instead of playing on.  Printed for both: the exploitability of the re-solved
profile within the subgame, what the opponent's best response to the re-solved hero is worth there, and the opponent's EXCESS -- how much
more than it was promised it can take, per holding.  (The safe profile's opponent rows are the gadget's: trained from a flat reach and with
the way out, they are nobody's strategy, and most of that profile's exploitability is the hero's best response to them.  What re-solving
hands on is the hero's rows; the excess is their measure.)

    python examples/continual_resolve.py [board="KS 9D 7D 4C"] [river=2H]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pokerl_amd  # noqa: E402

board = (sys.argv[1] if len(sys.argv) > 1 else "KS 9D 7D 4C").split()
river = sys.argv[2] if len(sys.argv) > 2 else "2H"
HERO, OPPONENT, ITERS = 0, 1, 128


def high(c):
    return (int(c) & 15) or 13                                       # rank0 0 = ace, high


first = np.array([2 if high(a) == high(b) else int(min(high(a), high(b)) >= 9) for a, b in pokerl_amd.HOLDINGS], np.uint16) * 30000
second = np.array([2 if (int(a) >> 4) == (int(b) >> 4) else 1 for a, b in pokerl_amd.HOLDINGS], np.uint16) * 30000

# 1. the turn spot, on a coarse tree (one bet size a street), with the outputs at the river-level node both players reach by checking
coarse = pokerl_amd.turn_tree(100, 400, (1.0,), 1)
node = next(v for v in coarse.river_decision_nodes if coarse.put[v].max() == 0)
turn = pokerl_amd.solve_turn(board, [first, second], coarse, ITERS, at=node, at_card=river)

# 2. the river subgame there, on a finer tree: the same pot, nothing put in yet, three bet sizes and a raise more
fine = pokerl_amd.river_tree(coarse.pot, 400, (0.33, 0.66, 1.0), 2)
unsafe = pokerl_amd.resolve_river(board + [river], fine, turn.node_reach, ITERS, HERO)
safe = pokerl_amd.resolve_river(board + [river], fine, turn.node_reach, ITERS, HERO, opponent_values=turn.node_br[OPPONENT])


def excess(solution):
    """chips per holding the opponent takes beyond its promised values by best-responding to `solution`'s hero in the subgame"""
    played = pokerl_amd.solve_river(board + [river], None, fine, 0, reach=turn.node_reach, lock=np.ones(len(fine.decision_nodes), bool), locked=solution.strategy)
    over = np.maximum(0, played.br[OPPONENT] - turn.node_br[OPPONENT])[played.valid]
    best = sum(int(w) * int(b) for w, b in zip(turn.node_reach[OPPONENT], played.br[OPPONENT])) / (2 * played._pair_weight())
    return float(over.sum()) / (2.0 * float(turn.node_reach[HERO].sum()) * int(played.valid.sum())), played.exploitability, best


print("turn %s, river %s; %r; at node %d (%s); %d iterations each" % (" ".join(board), river, coarse, node, coarse.label(node), ITERS))
print("  the turn solve: exploitability %.4f chips" % turn.exploitability)
for name, solution in (("unsafe", unsafe), ("safe", safe)):
    e, x, best = excess(solution)
    print("  %-6s re-solve on %r: exploitability %.4f chips, the opponent's best response %.4f chips, its excess %.5f chips" % (name, fine, x, best, e))
assert unsafe.strategy.shape == safe.strategy.shape == (len(fine.decision_nodes), 4, 1326)
