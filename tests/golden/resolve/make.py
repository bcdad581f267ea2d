"""Writes the re-solving fixtures from tests/resolve_spec.py ALONE (no kernel, no library call beyond the host-side tree builder): the
pool at which the live spec is too slow for a test.
    python tests/golden/resolve/make.py [name ...]        (default: every fixture; a few minutes each)
Each <name>.npz holds the spec's node_reach, node_value, node_br, value, br and status.  The INPUTS are not stored: inputs(name) regenerates
them from the fixture's seed -- the spot, the tree turn_tree(100, 400, (1.0,), 1), root reaches up to 2^17 - 1 with zeros among them
(0xFFFFFFFF at the invalid holdings, which are not read), `at` a river-level decision node and at_card a card from the middle of the pool."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import resolve_spec as RZ               # noqa: E402
import rvr_spec as VS                   # noqa: E402
from pokerl_amd.solver import turn_tree  # noqa: E402

H = 1326
ITERS = 2
FIXTURES = {"turn_p48": (48, 4816)}        # name -> (pool, seed)
KEYS = ("node_reach", "node_value", "node_br", "value", "br")


def inputs(name):
    """Everything a call takes, with the leading [1] of a one-spot batch"""
    pool, seed = FIXTURES[name]
    rng = np.random.default_rng(seed)
    board, _, dead = VS.random_boards(rng, 1, 4, pool)
    board = np.ascontiguousarray(board[:, :4])
    reach = rng.integers(0, RZ.TURN_LIM + 1, (1, 2, H)).astype(np.uint32)
    reach[rng.random(reach.shape) < 0.15] = 0
    _, gone = VS.check_spot([int(c) for c in board[0]], 4, int(dead[0]))
    reach[0][:, [h for h in range(H) if VS.PAIR_A[h] in gone or VS.PAIR_B[h] in gone]] = 0xFFFFFFFF
    tree = turn_tree(100, 400, (1.0,), 1)
    cards = [k for k in range(52) if k not in gone]
    at = np.array([tree.river_decision_nodes[1]], np.uint8)
    at_card = np.array([int(VS.CANON[cards[len(cards) // 2]])], np.uint8)
    return dict(board=board, dead=np.asarray(dead, np.uint64), reach=reach, tree=tree, iters=ITERS, at=at, at_card=at_card)


def make(name):
    x = inputs(name)
    r = RZ.solve_turn_spot([int(c) for c in x["board"][0]], None, x["tree"], ITERS, dead=int(x["dead"][0]), reach=x["reach"][0], at=int(x["at"][0]),
                           at_card=int(x["at_card"][0]))
    assert r["status"] == 0 and r["P"] == FIXTURES[name][0] and r["node_value"].any()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), status=np.uint8(r["status"]), **{k: r[k] for k in KEYS})
    print(name, "done", flush=True)


if __name__ == "__main__":
    for name in sys.argv[1:] or list(FIXTURES):
        make(name)
