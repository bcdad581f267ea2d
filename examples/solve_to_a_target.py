#!/usr/bin/env python3
"""Solve to a target (pk_solve_river_resume): nobody knows before the call how many iterations a spot needs, so solve_river_until runs the
solver in steps, the regrets and the average accumulators staying in device memory between the calls, and stops when the exploitability is
at or under the target -- the same bytes a single call with that many iterations gives.  Then the solution's state is a checkpoint: the
spot is solved on from it after the ranges moved a little (a warm start), and from nothing for comparison.

    python examples/solve_to_a_target.py [board="KS 9D 7D 4C 2H"] [target=0.5]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pokerl_amd  # noqa: E402

board = (sys.argv[1] if len(sys.argv) > 1 else "KS 9D 7D 4C 2H").split()
target = float(sys.argv[2]) if len(sys.argv) > 2 else 0.5


def high(c):
    return (int(c) & 15) or 13                                       # rank0 0 = ace, high


first = np.array([2 if high(a) == high(b) else int(min(high(a), high(b)) >= 9) for a, b in pokerl_amd.HOLDINGS], np.uint16) * 30000
second = np.array([2 if (int(a) >> 4) == (int(b) >> 4) else 1 for a, b in pokerl_amd.HOLDINGS], np.uint16) * 30000
tree = pokerl_amd.river_tree(100, 400)

# 1. until the target is met, 32 iterations a call
sol = pokerl_amd.solve_river_until(board, [first, second], tree, target, step=32, max_iters=1024)
print("river %s, %r: %d iterations in %d calls, state %.1f MB on the device" % (" ".join(board), tree, sol.iters, len(sol.trace), sol.state.nbytes / 1e6))
print("  exploitability after each call: " + " ".join("%.3f" % e for e in sol.trace))
once = pokerl_amd.solve_river(board, [first, second], tree, sol.iters)
assert once.strategy.tobytes() == sol.strategy.tobytes() and once.br.tobytes() == sol.br.tobytes()      # stopping and continuing costs no bit

# 2. the ranges move a little: player 1 drops a tenth of its suited hands.  Warm: on from the checkpoint.  Cold: from nothing
moved = second.copy()
moved[second == 60000] = 54000
warm = pokerl_amd.solve_river(board, [first, moved], tree, 32, state=sol.state)
cold = pokerl_amd.solve_river(board, [first, moved], tree, 32)
print("  after the ranges moved, 32 more iterations: warm %.3f chips (t = %d), cold %.3f chips" % (warm.exploitability, int(warm.state.t), cold.exploitability))
