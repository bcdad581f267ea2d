#!/usr/bin/env python3
"""Many river subgames of DIFFERENT pots in one call (pk_solve_river_trees): random boards, random ranges and a
pot per spot, as a generator of counterfactual-value training data would draw them.  pokerl_amd.river_trees builds one betting tree per
distinct (pot, stack) pair and the index of each spot's tree; solve_river_batch takes both and solves every spot with its own tree in
one launch.  Spot i's outputs are byte for byte what solve_river gives for it alone with that tree -- the last lines check one.
Printed per spot: pot, stack, its tree, each player's value in chips and the exploitability of the strategy.

    python examples/solve_many_pots.py [spots=12] [iterations=64]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pokerl_amd  # noqa: E402
from pokerl_amd import solver  # noqa: E402

m = int(sys.argv[1]) if len(sys.argv) > 1 else 12
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 64
rng = np.random.default_rng(2024)
CANON = [(i % 13) | ((i // 13) << 4) for i in range(52)]               # Card.value: rank0 in the low nibble, the suit above it
board = np.array([[CANON[c] for c in rng.permutation(52)[:5]] for _ in range(m)], np.uint8)
ranges = rng.integers(1, 65536, (m, 2, 1326)).astype(np.uint16)         # (a reach is weight << 4: weights that use the sixteen bits)
pots = rng.choice([40, 60, 100, 150, 240], m)                          # chips in the middle, and 1 000 chips a player at the hand's start
stacks = 500 - pots // 2

trees, tree_of = pokerl_amd.river_trees(pots, stacks)
print("%d spots, %d distinct trees of %s nodes" % (m, len(trees), sorted({t.n for t in trees})))
batch = solver.solve_river_batch(board, ranges, trees, iters, tree_of=tree_of)
for i in range(m):
    s = batch[i]                                                       # an ordinary single solution: its own tree, its own strategy rows
    print("  spot %2d: pot %3d, %3d behind, %r: value %8.3f / %8.3f chips, exploitability %.4f" % ((i, pots[i], stacks[i], s.tree) + s.ev + (s.exploitability,)))
alone = solver.solve_river_batch(board[:1], ranges[:1], trees[tree_of[0]], iters)[0]
same = all((np.asarray(getattr(alone, k)) == np.asarray(getattr(batch[0], k))).all() for k in ("strategy", "value", "br"))
print("spot 0 solved alone with its tree gives the same bytes: %s" % same)
