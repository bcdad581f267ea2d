#!/usr/bin/env python3
"""One-off confidence run (GPU box): Game.step with the caller's actions on DEVICE buffers -- pk_pick_actions_d + pk_step_auto_d
(the reset of a finished game inside the step's launch), on a twin handle pk_step_d + pk_reset_d(flags, GAME_OVER), and on a third one the
BOUNDED form pk_step_async_d (one or two hand ends per launch, reset inside; a table whose step rolls on stays in flight and is delivered by
a later call: its delivered flags / terr must be those the oracle returned when the step started, its state equal after a drain) -- against
the CPU oracle's step + reset over seeded odd configurations (every N, zero / fractional / oversized blinds, per-seat stacks
0.5 .. 1e6, any table-id base and dealer, batches from 65 to 4 097 tables: full and nearly empty waves).  This is the path on which a
step that rolls hand after hand is served by end_block's single-table paths (lone showdown, deck stock).  Every handle also has the step kernels
write the StateView row of the player to act (pk_set_step_obs: dense + packed / packed only / dense only): after every call the rows of the
tables whose step returned must be, byte for byte, the oracle's StateView fields (tests/seat_matrix.oracle_rows; the comparison with the
getter kernels pk_get_obs_d / pk_get_obs_packed_d, which this tool made until the drivers were shared, is tests/test_hip_views.py's).
The drivers are tests/seat_matrix.game_step (which also runs the host form, pk_step + pk_reset, not counted in the total, and compares
pot / high_bet / game_over at the snapshot points) and tests/seat_matrix.game_step_async.  One configuration in three (drawn from a
generator of its own, so the others are the ones this tool always ran) is played by the never-fold caller of oracle/rng_spec.py
(POLICY_DEEP: hands raised on every street that reach multi-way river showdowns); the device is then handed the oracle's actions.
usage: python tools/fuzz_step_d.py [configs] [seed]"""
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seat_matrix as M  # noqa: E402
from hip_backend import HipBackend as HB  # noqa: E402
from oracle import loader as O  # noqa: E402

n_cfg = int(sys.argv[1]) if len(sys.argv) > 1 else 150
rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 2027)
deep_rng = random.Random((int(sys.argv[2]) if len(sys.argv) > 2 else 2027) + 1)      # which configurations the deep caller plays
stacks = [0.5, 1, 2, 3, 5, 10, 37.5, 100, 1000, 1e6]
blinds = [0, 0.25, 0.5, 1, 2, 3, 7.5, 40]

tot = dict(steps=0, resets=0, async_steps=0, async_inflight=0, rows=0)
deep = 0
for i in range(n_cfg):
    N = 2 + i % 15
    start = [rng.choice(stacks) for _ in range(N)] if rng.random() < 0.5 else rng.choice(stacks)
    bb, sb = rng.choice(blinds), rng.choice(blinds)
    policy = 1 if rng.random() < 0.25 else 0
    seed, base, dealer = rng.getrandbits(63), rng.getrandbits(32) & 0xFFFFF000, rng.randrange(N)
    T = rng.choice([65, 128, 300, 1000, 4097])
    K = rng.choice([40, 90, 200])
    probe = O.OracleGame(16, N, start, bb, sb, seed=seed, table_id_base=base)
    probe.reset()
    t_probe = time.time()
    probe.rollout(K, policy, True)
    if deep_rng.random() < 1 / 3:
        policy = M.R.POLICY_DEEP
    if (time.time() - t_probe) * T / 16 > 20:        # blinds far above the stacks: steps that roll thousands of hands
        T = 65
    # (pk_step_auto_d resets with dealer 0, as Game.reset() does: the first reset uses dealer 0 as well)
    cfg = dict(kind="cfg %d" % i, T=T, N=N, start=start, bb=bb, sb=sb, seed=seed, base=base, dealer=0, policy=policy)
    deep += policy == M.R.POLICY_DEEP
    for st in (M.game_step(HB, cfg, K, views_every=40), M.game_step_async(HB, cfg, K, max_hands=1 + i % 2)):
        for k in tot:
            tot[k] += st.get(k, 0)
    if i % 25 == 24:
        print("%d configurations bit-exact so far" % (i + 1), flush=True)
print("fuzz: %d configurations (%d played by the never-fold caller), %d device-resident Game.steps, %d games reset inside a step's launch, all bit-exact vs the oracle; "
      "bounded launches: %d steps delivered, %d times a table's step was left in flight, every delivery and every drained state equal; "
      "%d observation rows written by the step kernels (pk_set_step_obs) equal to the oracle's StateView fields"
      % (n_cfg, deep, tot["steps"], tot["resets"], tot["async_steps"], tot["async_inflight"], tot["rows"]))
