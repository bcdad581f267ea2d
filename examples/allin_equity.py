#!/usr/bin/env python3
"""Showdown equity on the device: "if the cards still to come were dealt now, how often does each seat win?" -- every board enumerated,
exact counts (VecGame.equity / pokerl_amd.showdown_equity; winners as the reference's compare_rankings judges them).

(a) the table form on a live 6-seat batch: each table's equities beside its hole cards;
(b) the equity of the player to act AGAINST UNKNOWN HANDS: the table is cloned with everything that player cannot see redealt
    (clone_tables(observer='active')), and the mean of the clones' exact equities is the answer -- next to a plain Monte Carlo of the same
    quantity with ONE sampled board per clone (each clone judged on the board its redealt deck happens to hold: an all-in-now showdown,
    not a played-out rollout as in determinized_search.py), which needs far more clones for the same error.

    python examples/allin_equity.py [clones=4096] [seed=3]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pokerl_amd  # noqa: E402
from pokerl_amd import Card, showdown_equity_batch  # noqa: E402

C = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 3
N = 6
config = dict(num_players=N, start_credits=100, big_blind=2, small_blind=1)

# ---- (a) a live batch, a few steps into its hands
g = pokerl_amd.VecGame(8, seed=seed, **config)
g.reset()
g.rollout(9, policy=pokerl_amd.Policy.RANDOM, auto_reset=True)
eq = g.equity()
deck, states, turn = g.deck, g.player_states, g.turn
for t in range(g.num_tables):
    nb = 0 if turn[t] == 0 else min(int(turn[t]) + 2, 5)
    print("table %d  board %-16s %8d boards" % (t, " ".join(str(Card(int(v))) for v in deck[t, :nb]) or "-", eq.boards[t]))
    for p in range(N):
        cards = " ".join(str(Card(int(v))) for v in deck[t, 5 + 2 * p:7 + 2 * p])
        live = states[t, p] in (pokerl_amd.PlayerState.ACTIVE, pokerl_amd.PlayerState.CALLED, pokerl_amd.PlayerState.ALL_IN)
        print("    seat %d  %-7s %s" % (p, cards, "equity %.4f  (wins %d, ties %d)" % (eq.equity[t, p], eq.win[t, p], eq.tie[t, p]) if live else "folded"))
assert not eq.status.any()

# ---- (b) table 0's player to act against unknown hands
seat = int(g.active_player[0])
sims = pokerl_amd.VecGame(C, seed=seed + 1, **config)
sims.clone_tables(np.arange(C), [0], src=g, observer='active', nonce=seed)
exact = sims.equity().equity[:, seat]                      # exact per clone: only the opponents' hands are sampled
# one sampled board per clone: the clone's own redealt board, judged once (the explicit form with all five board cards known)
d = sims.deck
live = (((sims.player_states >= 1) & (sims.player_states <= 3)).astype(np.uint16) << np.arange(N, dtype=np.uint16)).sum(axis=1).astype(np.uint16)
one = showdown_equity_batch(d[:, 5:].reshape(C, N, 2), d[:, :5], np.full(C, 5, np.uint8), live).equity[:, seat]
print("\nseat %d of table 0 against unknown hands, %d clones:" % (seat, C))
print("    mean of exact equities   %.4f  (+- %.4f)" % (exact.mean(), exact.std() / np.sqrt(C)))
print("    one sampled board each   %.4f  (+- %.4f)" % (one.mean(), one.std() / np.sqrt(C)))
g.close()
sims.close()
