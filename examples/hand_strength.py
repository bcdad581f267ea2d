#!/usr/bin/env python3
"""A hand-strength feature that leaks nothing: every step's observation of the player to act gains that seat's SAMPLED showdown equity
(pk_table_equity_sampled_d, observer = each table's active seat) -- the other seats' hole cards and the board to come are drawn on the
device, never read.  Everything stays in HBM: the observation rows (pk_set_step_obs), the equity counts, the actions.  A network would
read `obs` and `share` (equity = share / (720720 * samples)); here the library's in-kernel random pick stands in for it.  A new nonce per
step gives independent draws; the counts of the steps a spot stays unchanged could be added up for a tighter estimate.
Where the flop is out, the EXACT strength of the same seat against one hidden hand (pk_table_equity_range, every holding and every board
enumerated) is printed beside it.  The two answer different questions -- every live opponent with the pot split among all winners, against
one opponent with a tie counted as a half -- and are the same quantity only heads-up.

    python examples/hand_strength.py [tables=65536] [steps=200] [samples=256]
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
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
S = int(sys.argv[3]) if len(sys.argv) > 3 else 256
N = 6
game = pokerl_amd.VecGame(T, num_players=N)
game.reset()
actions, flags, terr = DeviceBuffer(T * 4), DeviceBuffer(T), DeviceBuffer(T)
obs = DeviceBuffer(T * (17 + 3 * N) * 8)                       # dense StateView rows of the player to act
share = DeviceBuffer(T * N * 8)                                # uint64 [T, N]: the feature is row t, column active seat of t
status = DeviceBuffer(T)
L.check(L.lib().pk_get_obs_d(game._h, -1, obs.ptr), game._h)
game.set_step_obs(obs, None)                                   # every step_d writes the next rows itself
game.sync()
t0 = time.perf_counter()
for s in range(steps):
    game.equity_sampled_d(observer=pokerl_amd.OBSERVER_ACTIVE, samples=S, nonce=s, share_d=share, status_d=status)
    # <- your policy kernel goes here: it reads obs[t] and share[t, active seat] / (720720 * S), writes actions[t]
    game.pick_actions_d(actions, pokerl_amd.Policy.RANDOM)
    game.step_d(actions, flags, terr, auto_reset=True)
game.sync()
dt = time.perf_counter() - t0
assert not status.download(np.uint8, T).any() and not (terr.download(np.uint8, T) & L.TERR_INVALID_ACTION).any()
# one look at the last step's feature on the host (the loop itself never leaves the device)
game.equity_sampled_d(observer=pokerl_amd.OBSERVER_ACTIVE, samples=S, nonce=steps, share_d=share, status_d=status)
game.sync()
eq = share.download(np.uint64, T * N).reshape(T, N)[np.arange(T), game.active_player] / float(L.EQ_SHARE_UNIT * S)
print("%d tables x %d steps, each with a %d-sample equity of the acting seat, in %.3f s (%.1f us per step of the whole batch); "
      "acting seats' equity now: mean %.3f, 10th / 90th percentile %.3f / %.3f"
      % (T, steps, S, dt, dt / steps * 1e6, eq.mean(), np.percentile(eq, 10), np.percentile(eq, 90)))
exact = game.equity_range(observer='active')                   # post-flop tables only: the others report PK_EQ_PREFLOP
post = exact.status == 0
if post.any():
    print("the %d tables past the flop: sampled equity against every live opponent, mean %.3f; exact strength against ONE hidden hand, mean %.3f"
          % (int(post.sum()), eq[post].mean(), exact.strength[post].mean()))
game.set_step_obs(None, None)
for b in (actions, flags, terr, obs, share, status):
    b.free()
game.close()
