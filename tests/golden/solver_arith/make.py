"""Writes turn_corner_p48.npz from tests/resume_spec.py ALONE (no kernel, no library call beyond the host-side tree builder): the turn
solver's bounds corner at the full pool, where the live restatement is too slow for a test.
    python tests/golden/solver_arith/make.py        (two to three minutes)
The spot is solver_rule_cases.corner_call(4, 48, "top"): turn_tree(2731, 5460, (1.0,), 1) (pot + put = 8191), every weight 65535, every
state entry at TURN_RMAX / TURN_AMAX, t0 = 4093 and 3 iterations.  The Python-integer witness (tests/solver_witness.py), which cannot wrap,
runs on the same spot first and must equal the restatement in every output and state entry, with every quantity below the header's figure
for it: nothing is written otherwise.  The file holds the spot (board, dead, the tree's arguments, the weight, t0, iters), strategy, value,
br and status, and SHA-256 digests of river_strategy and of the four state arrays (C order, the dtypes of the call: uint16 and int64)."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import solver_rule_cases as RC          # noqa: E402
import solver_witness as SW             # noqa: E402

DIGESTS = ("river_strategy", "regret", "average", "river_regret", "river_average")
KEYS = ("strategy", "river_strategy", "value", "br", "regret", "average", "river_regret", "river_average")


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def make():
    call = RC.corner_call(4, 48, "top")
    want = RC.spec_of(4, call)
    assert want["status"].tolist() == [0] and want["P"].tolist() == [48] and want["t"].tolist() == [4096]
    got, rec = SW.run_call(4, call)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and (got[k] == want[k]).all(), k
    SW.check_bounds(4, rec)
    print("below 2^x, x =", rec.bits(), flush=True)
    np.savez_compressed(os.path.join(HERE, "turn_corner_p48.npz"), board=call["board"][0], dead=np.uint64(call["dead"][0]),
                        tree_args=np.array([2731, 5460, 1], np.uint32), weight=np.uint16(65535), t0=np.uint32(4093), iters=np.uint32(3),
                        status=np.uint8(want["status"][0]), strategy=want["strategy"][0], value=want["value"][0], br=want["br"][0],
                        **{"sha256_" + k: np.array(digest(want[k][0])) for k in DIGESTS})
    print("turn_corner_p48 done", flush=True)


if __name__ == "__main__":
    make()
