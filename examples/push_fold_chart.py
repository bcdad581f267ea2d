#!/usr/bin/env python3
"""Heads-up push / fold charts for stacks of 2 ... 20 big blinds in ONE call (pk_solve_preflop): the small blind
jams or folds, the big blind calls or folds, and a call is paid by the exact all-in equity of the two holdings over all 1 712 304 boards.
pokerl_amd.preflop_trees(..., push_fold=True) builds one five-node tree per stack and the index of each spot's tree; solve_preflop_batch
solves the nineteen games in one launch.  Printed per stack: how much of its range each player plays, the small blind's value and the
exploitability of the strategies in big blinds; then the jam and the call chart of one stack as 13 x 13 grids (by_class: suited above the
diagonal, off-suit below, percent of the class that jams / calls).  The charts are for the eye: the counts behind them are this
package's own and are not suit-symmetric, so the holdings of one class need not play alike.

    python examples/push_fold_chart.py [iterations=256] [chart_stack_bb=10]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pokerl_amd  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 256
show = int(sys.argv[2]) if len(sys.argv) > 2 else 10
SB, BB = 50, 100                                                        # chips: a stack of k big blinds is 100 k chips (at most 8 191)
depths = list(range(2, 21))
trees, tree_of = pokerl_amd.preflop_trees([BB * k for k in depths], SB, BB, push_fold=True)
ranges = np.full((len(depths), 2, 1326), 65535, np.uint16)              # every holding, equally likely (a reach is weight << 4)
batch = pokerl_amd.solve_preflop_batch(ranges, trees, iters, tree_of)
RANKS = "23456789TJQKA"


def chart(grid):
    """[13, 13] over rank indices (by_class: pairs on the diagonal, suited at (hi, lo), off-suit at (lo, hi)) as the usual chart: aces
    first, so that the suited classes come out right of the diagonal"""
    lines = ["    " + " ".join("%3s" % r for r in reversed(RANKS))]
    for i in reversed(range(13)):
        lines.append("  %s " % RANKS[i] + " ".join("%3.0f" % (100 * grid[i, j]) for j in reversed(range(13))))
    return "\n".join(lines)


print("%d iterations of CFR+, blinds %d / %d" % (iters, SB, BB))
for i, k in enumerate(depths):
    s = batch[i]
    jam, call = s.probabilities(0)[1].mean(), s.probabilities(2)[1].mean()
    print("  %2d bb: jam %5.1f %%, call %5.1f %%, small blind's value %+.4f bb, exploitability %.5f bb" % (k, 100 * jam, 100 * call, s.ev[0] / BB, s.exploitability / BB))
one = batch[depths.index(show)]
print("\njam, %d bb (suited right of the diagonal, off-suit left of it)\n%s" % (show, chart(one.by_class(0)[1])))
print("\ncall, %d bb\n%s" % (show, chart(one.by_class(2)[1])))
