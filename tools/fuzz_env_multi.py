#!/usr/bin/env python3
"""One-off confidence run (GPU box): pk_env_step_multi_d -- one agent per seat, some seats played by the caller -- against
the CPU oracle over seeded odd configurations (every N, odd blinds / stacks, random per-seat policies random / all-in /
call, a random subset of the opponent seats external and played on the host by the policy's own rule, bounded launches of
1..9 passes with auto-reset): per table the delivered (reward, done, hand, terr) sequence must equal the oracle's.
The driver is tests/seat_matrix.env_multi.
usage: python tools/fuzz_env_multi.py [configs] [seed] [only this configuration index]"""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seat_matrix as M  # noqa: E402

n_cfg = int(sys.argv[1]) if len(sys.argv) > 1 else 60
rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 11)
only = int(sys.argv[3]) if len(sys.argv) > 3 else None
cap = int(os.environ.get("PK_FUZZ_LAUNCH_CAP", "6000"))   # (calling stations at one pass per launch: 3 300 launches per env.step seen)
stacks = [2, 5, 10, 37.5, 100, 1000]
blinds = [0.5, 1, 2, 3, 7.5, 40]
delivered = yields = 0
for i in range(n_cfg):
    N = 2 + i % 15   # 2 ... 16 seats
    start = [rng.choice(stacks) for _ in range(N)] if rng.random() < 0.5 else rng.choice(stacks)
    bb, sb = rng.choice(blinds), rng.choice(blinds)
    # shoving or random opponents for the caller's seats: calling stations would play endless games once seat 0 is broke
    pols = [rng.choice([0, 0, 1, 2]) for _ in range(N - 1)]
    external = [s for s in range(1, N) if pols[s - 1] != 2 and rng.random() < 0.5]
    seed, base = rng.getrandbits(63), rng.getrandbits(32) & 0xFFFFF000
    T, K, passes = rng.choice([65, 300, 700]), rng.choice([8, 15, 25]), rng.randrange(1, 10)
    if only is not None and i != only:
        continue
    cfg = dict(kind="cfg %d" % i, T=T, N=N, start=start, bb=bb, sb=sb, seed=seed, base=base, dealer=0, policy=0)
    st = M.env_multi(cfg, pols, external, K, passes, cap=cap)
    delivered += st["delivered"]; yields += st["yields"]
    if only is not None:
        print("%s pols=%s external=%s K=%d passes=%d: %d launches" % (M.where_of(cfg), pols, external, K, passes, st["launches"]))
    if i % 10 == 9:
        print("%d configurations bit-exact so far" % (i + 1), flush=True)
print("fuzz: %d configurations, %d env.steps delivered, %d yields to caller-played seats, all equal to the oracle's sequences"
      % (n_cfg, delivered, yields))
