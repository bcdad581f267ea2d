#!/usr/bin/env python3
"""Monte Carlo action values for the player to act at ONE table, by determinized search on the device: the table is cloned into
65 536 slots with the cards its player cannot see redealt in every clone (pk_clone_tables_d with PK_OBSERVER_ACTIVE -- a plain copy
would share the future board and the opponents' hole cards, and the search would cheat), each valid action takes a slice of the
clones, the random agent plays the rest of the hand (pick_actions_d + step_d; a clone whose hand is over gets action -1, which leaves
it untouched), and the value of an action is the mean of the player's result over its slice: credits after the hand minus before.

    python examples/determinized_search.py [clones=65536] [seed=1]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pokerl_amd  # noqa: E402
from pokerl_amd import _lib as L  # noqa: E402
from pokerl_amd.enums import PokerMoves  # noqa: E402
from pokerl_amd.hipmem import DeviceBuffer  # noqa: E402

C = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
N = 6
config = dict(num_players=N, start_credits=100, big_blind=2, small_blind=1)

# the position to evaluate: a game a few random moves into its first hand
root = pokerl_amd.VecGame(1, seed=seed, **config)
root.reset()
rng = np.random.default_rng(seed)
for _ in range(4):
    onehot, _ = root.get_valid_actions()
    root.step(np.array([rng.choice(np.flatnonzero(onehot[0]))]))
seat = int(root.active_player[0])
valid = np.flatnonzero(root.get_valid_actions()[0][0])
credit0 = float(root.credits[0, seat])
print("table: hand %d, turn %d, seat %d to act; valid actions: %d (%s)" % (
    int(root.hand[0]), int(root.turn[0]), seat, len(valid), ", ".join(PokerMoves.as_string[a] for a in valid)))
print("valid actions: %d" % len(valid))

# 1. clone into C slots, redealing what the acting seat cannot see (nonce: a fresh deal per search)
sims = pokerl_amd.VecGame(C, seed=seed + 1, **config)
sims.clone_tables(np.arange(C), [0], src=root, observer='active', nonce=seed)
# 2. each valid action gets a slice of the clones
which = np.arange(C) % len(valid)
over, hand_over, _, terr = sims.step(valid[which].astype(np.int32), strict=False)
assert not terr.any()
done = hand_over.copy()
# 3. the rest of the hand with the random agent, on device buffers
actions, flags, terr_d = DeviceBuffer(C * 4), DeviceBuffer(C), DeviceBuffer(C)
for _ in range(200):
    if done.all():
        break
    sims.pick_actions_d(actions, pokerl_amd.Policy.RANDOM)
    a = actions.download(np.int32, C)
    a[done] = -1                                   # finished hands stay as they are
    actions.upload(a)
    sims.step_d(actions, flags, terr_d)
    sims.sync()
    done |= (flags.download(np.uint8, C) & L.FLAG_HAND_OVER) != 0
assert done.all()
# 4. the acting seat's result per action
result = sims.credits[:, seat] - credit0
for k, a in enumerate(valid):
    r = result[which == k]
    print("action %-10s value %+8.3f  (+- %.3f, %d clones)" % (PokerMoves.as_string[a], r.mean(), r.std() / np.sqrt(len(r)), len(r)))
for b in (actions, flags, terr_d):
    b.free()
