#!/usr/bin/env python3
"""One-off confidence run (GPU box): pk_env_step_async_d against pk_env_step_fused_d and the CPU oracle over seeded odd
configurations (every N, odd blinds / stacks, both opponent policies, pass budgets 1..9, half of them with the handle split
into 2..8 sub-batches by pk_set_env_batches): per table the delivered (reward, done, hand, obs row) sequence must equal the
synchronous one bit for bit.
The driver is tests/seat_matrix.env_step (which also runs the host form, pk_env_step + pk_env_reset).
usage: python tools/fuzz_env_async.py [configs] [seed]"""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seat_matrix as M  # noqa: E402

n_cfg = int(sys.argv[1]) if len(sys.argv) > 1 else 60
rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 7)
stacks = [1, 2, 5, 10, 37.5, 100, 1000]
blinds = [0.5, 1, 2, 3, 7.5, 40]
delivered = sub = 0
for i in range(n_cfg):
    N = 2 + i % 15   # 2 ... 16 seats
    start = [rng.choice(stacks) for _ in range(N)] if rng.random() < 0.5 else rng.choice(stacks)
    bb, sb = rng.choice(blinds), rng.choice(blinds)
    opp = 1 if rng.random() < 0.25 else 0
    seed, base = rng.getrandbits(63), rng.getrandbits(32) & 0xFFFFF000
    T, K, passes = rng.choice([65, 300, 1000]), rng.choice([8, 15, 25]), rng.randrange(1, 10)
    B = rng.choice([1, 1, 1, 2, 3, 4, 8])
    if os.environ.get("PK_FUZZ_ONLY") and i != int(os.environ["PK_FUZZ_ONLY"]):
        continue
    cfg = dict(kind="cfg %d" % i, T=T, N=N, start=start, bb=bb, sb=sb, seed=seed, base=base, dealer=0, policy=0)
    st = M.env_step(cfg, opp, K, passes, B=B, exact_batches=False)
    delivered += st["delivered"]; sub += st["sub"]
    if i % 20 == 19:
        print("%d configurations bit-exact so far" % (i + 1), flush=True)
print("fuzz: %d configurations (%d with sub-batches inside the handle), %d env.steps delivered asynchronously, all equal to the synchronous sequences"
      % (n_cfg, sub, delivered))
