"""Writes the turn solver's fixtures from tests/turn_solver_spec.py ALONE (no kernel, no library call beyond the host-side tree builder):
the pools at which the live spec is too slow for a test (about 45 s a spot: river_solver_spec.pairwise for each of up to 48 river cards).
    python tests/golden/turn_solver/make.py [name ...]        (default: every fixture; a few minutes each)
Each p<P>.npz / magnitude.npz holds the spot (board, dead, ranges), the tree's arguments (pot, stack: turn_tree(pot, stack, (1.0,), 1), nine
turn-level nodes, one bet size), iters, and the spec's strategy, value, br, status and the SHA-256 of river_strategy's bytes."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import rvr_spec as VS                   # noqa: E402
import turn_solver_spec as TS           # noqa: E402
from pokerl_amd.solver import turn_tree  # noqa: E402

ITERS = 2
# name -> (pool, seed, pot, stack, every weight 65535)
FIXTURES = {"p45": (45, 451, 100, 400, False), "p46": (46, 461, 100, 400, False), "p47": (47, 471, 100, 400, False), "p48": (48, 481, 100, 400, False),
            "magnitude": (48, 482, 2731, 5460, True)}         # pot + the largest put = 8191


def spot(name):
    pool, seed, pot, stack, full = FIXTURES[name]
    rng = np.random.default_rng(seed)
    board, _, dead = VS.random_boards(rng, 1, 4, pool)
    ranges = rng.integers(0, 65536, (2, TS.HOLDINGS)).astype(np.uint16)
    for row in ranges:
        row[rng.integers(0, TS.HOLDINGS, 200)] = 0
        row[rng.integers(0, TS.HOLDINGS, 100)] = 65535
    if full:
        ranges[:] = 65535
    return board[0, :4].copy(), np.uint64(dead[0]), ranges, pot, stack


def make(name):
    board, dead, ranges, pot, stack = spot(name)
    tree = turn_tree(pot, stack, (1.0,), 1)
    r = TS.solve_spot([int(x) for x in board], ranges, tree, ITERS, int(dead))
    assert r["status"] == 0 and r["P"] == FIXTURES[name][0]
    np.savez_compressed(os.path.join(HERE, name + ".npz"), board=board, dead=dead, ranges=ranges, pot=pot, stack=stack, iters=ITERS,
                        strategy=r["strategy"], value=r["value"], br=r["br"], status=np.uint8(r["status"]), regret_bits=r["regret_bits"],
                        river_sha256=hashlib.sha256(np.ascontiguousarray(r["river_strategy"]).tobytes()).hexdigest())
    print(name, "regret_bits", r["regret_bits"], flush=True)


if __name__ == "__main__":
    for name in sys.argv[1:] or list(FIXTURES):
        make(name)
