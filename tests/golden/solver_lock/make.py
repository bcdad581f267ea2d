"""Writes the locked turn solver's fixtures from tests/solver_lock_spec.py ALONE (no kernel, no library call beyond the host-side tree
builder): the pools at which the live spec is too slow for a test.
    python tests/golden/solver_lock/make.py [name ...]        (default: every fixture; a few minutes each)
Each <name>.npz holds the spec's strategy, value, br, status and the SHA-256 of river_strategy's bytes.  The INPUTS are not stored:
inputs(name) regenerates them from the fixture's seed -- the spot, the tree turn_tree(100, 400, (1.0,), 1), and the lock arrays: player 1's
turn-level rows and player 0's river-level rows locked to random weights with zeros among them, 0xFFFF in the action slots past nact."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import rvr_spec as VS                   # noqa: E402
import solver_lock_spec as LS           # noqa: E402
from pokerl_amd.solver import turn_tree  # noqa: E402

H = 1326
ITERS = 2
FIXTURES = {"turn_p33": (33, 3301), "turn_p48": (48, 4801)}        # name -> (pool, seed)


def inputs(name):
    """Everything a call takes, with the leading [1] of a one-spot batch"""
    pool, seed = FIXTURES[name]
    rng = np.random.default_rng(seed)
    board, _, dead = VS.random_boards(rng, 1, 4, pool)
    board = np.ascontiguousarray(board[:, :4])
    ranges = rng.integers(0, 65536, (1, 2, H)).astype(np.uint16)
    for row in ranges.reshape(-1, H):
        row[rng.integers(0, H, 200)] = 0
        row[rng.integers(0, H, 100)] = 65535
    tree = turn_tree(100, 400, (1.0,), 1)
    t1, _ = tree.rows_of(1)
    _, r0 = tree.rows_of(0)
    lock, river_lock = t1.astype(np.uint8)[None], r0.astype(np.uint8)[None]
    locked = rng.integers(0, 65536, (1, len(t1), 4, H)).astype(np.uint16)
    river_locked = rng.integers(0, 65536, (1, len(r0), 52, 4, H)).astype(np.uint16)
    locked[rng.random(locked.shape) < 0.1] = 0
    river_locked[rng.random(river_locked.shape) < 0.1] = 0
    for r, v in enumerate(tree.decision_nodes):
        locked[0, r, tree.num_actions(v):] = 0xFFFF
    for r, v in enumerate(tree.river_decision_nodes):
        river_locked[0, r, :, tree.num_actions(v):] = 0xFFFF
    return dict(board=board, dead=np.asarray(dead, np.uint64), ranges=ranges, tree=tree, iters=ITERS, lock=lock, locked=locked, river_lock=river_lock,
                river_locked=river_locked)


def make(name):
    x = inputs(name)
    r = LS.solve_turn_spot([int(c) for c in x["board"][0]], x["ranges"][0], x["tree"], ITERS, x["lock"][0], x["locked"][0], x["river_lock"][0],
                           x["river_locked"][0], int(x["dead"][0]))
    assert r["status"] == 0 and r["P"] == FIXTURES[name][0]
    np.savez_compressed(os.path.join(HERE, name + ".npz"), strategy=r["strategy"], value=r["value"], br=r["br"], status=np.uint8(r["status"]),
                        river_sha256=hashlib.sha256(np.ascontiguousarray(r["river_strategy"]).tobytes()).hexdigest())
    print(name, "done", flush=True)


if __name__ == "__main__":
    for name in sys.argv[1:] or list(FIXTURES):
        make(name)
