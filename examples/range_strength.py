#!/usr/bin/env python3
"""Exact hand strength of the acting seat at every table of a 65 536 x 6 handle, against ONE hidden hand (pk_table_equity_range_d): once
against a uniform range -- the opponent holds any two of the cards the seat cannot see -- and once against a range that drops the weakest
third of holdings (a crude model of an opponent who folded those before the flop).  Every completion of the board is enumerated on the
device; the weights are one uint16 per holding in the fixed 1 326 index space (pokerl_amd.holding_index), the result three sums per table,
and strength = (agg0 + agg1 / 2) / agg2.  Pre-flop tables are refused (status PK_EQ_PREFLOP) and cost nothing.

    python examples/range_strength.py [tables=65536] [steps=37]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pokerl_amd  # noqa: E402
from pokerl_amd import _lib as L  # noqa: E402
from pokerl_amd.hipmem import DeviceBuffer  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 37
N = 6


def holding_score(c0, c1):
    """A crude pre-flop ordering of holdings: pairs first, then high cards, a bonus for suited and for connected cards."""
    r0, r1 = sorted(((int(c) & 15) or 13 for c in (c0, c1)), reverse=True)      # rank0 0 = ace, high
    if r0 == r1:
        return 40 + 2 * r0
    return 2 * r0 + r1 + (3 if (int(c0) >> 4) == (int(c1) >> 4) else 0) + (2 if r0 - r1 == 1 else 0)


score = np.array([holding_score(a, b) for a, b in pokerl_amd.HOLDINGS])
tight = (score > np.sort(score)[L.EQ_HOLDINGS // 3]).astype(np.uint16)              # weight 1 for the upper two thirds, 0 for the rest
game = pokerl_amd.VecGame(T, num_players=N)
game.reset()
game.rollout(steps)                                                                 # a natural mix of turns
w_d = DeviceBuffer(tight.nbytes).upload(tight)
agg = [DeviceBuffer(T * 24), DeviceBuffer(T * 24)]
status = DeviceBuffer(T)
game.sync()
t0 = time.perf_counter()
game.equity_range_d(observer='active', agg_d=agg[0], status_d=status)               # uniform: no weights
game.equity_range_d(observer='active', weights_d=w_d, agg_d=agg[1])                 # the tight range, shared by every table
game.sync()
dt = time.perf_counter() - t0
st = status.download(np.uint8, T)
ok = st == 0
assert ((st == 0) | (st == L.EQ_PREFLOP)).all()
a = [x.download(np.uint64, T * 3).reshape(T, 3).astype(np.float64) for x in agg]
strength = [np.divide(x[:, 0] + 0.5 * x[:, 1], x[:, 2], out=np.zeros(T), where=x[:, 2] > 0) for x in a]
print("%d tables, %d of them past the flop: exact strength of the acting seat against one hidden hand, two ranges, in %.1f ms; "
      "uniform range: mean %.4f, 10th / 90th percentile %.3f / %.3f; without the weakest third of holdings: mean %.4f (%.4f lower on average)"
      % (T, int(ok.sum()), dt * 1e3, strength[0][ok].mean(), np.percentile(strength[0][ok], 10), np.percentile(strength[0][ok], 90),
         strength[1][ok].mean(), (strength[0][ok] - strength[1][ok]).mean()))
for b in agg + [w_d, status]:
    b.free()
game.close()
