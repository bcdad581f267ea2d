#!/usr/bin/env python3
"""Facing two all-ins with a short stack in the middle: what is the hero paid, in chips, if they call?

The hero (seat 0) holds ace-king suited on a K-7-2 flop and would have 100 in the pot after calling.  Seat 1 is all in for only 20; seat 2
has put in 100.  The hero cannot see their hands, only believe something about them: the short stack shoves wide (the best half of all
holdings), the big stack is tight (the best eighth).  ranged_equity answers "how often do I win when all three hands are compared" -- the
main pot alone.  ranged_ev pays the pot out the way Game.end_hand does: a main pot of 60 that all three contest and a side pot of 160 that
only the hero and the tight range can win.  The two disagree by about fifteen chips here: equity x pot - bet charges the hero the whole pot
for every board the wide short stack wins, although the short stack can take only 60 of the 220 chips."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pokerl_amd  # noqa: E402
from pokerl_amd import _lib as L  # noqa: E402


def top_range(fraction):
    """uint16 [1326]: weight 1 on the best `fraction` of the holdings in a crude pre-flop order (pairs, then high cards, suited first)."""
    score = np.zeros(L.EQ_HOLDINGS)
    for b in range(52):
        for a in range(b):
            ra, rb = a // 4, b // 4
            score[b * (b - 1) // 2 + a] = 100 + rb if ra == rb else 2 * rb + ra + (3 if a % 4 == b % 4 else 0)
    w = np.zeros(L.EQ_HOLDINGS, np.uint16)
    w[np.argsort(-score, kind="stable")[:int(round(fraction * L.EQ_HOLDINGS))]] = 1
    return w


hands = [["AS", "KS"], None, None]
board = ["KD", "7C", "2H"]
bets = [100.0, 20.0, 100.0]
ranges = np.stack([top_range(0.50), top_range(0.125)])
range_of = [L.EQW_UNIFORM, 0, 1]            # the hero's own entry is not read

S = 1 << 18
eq = pokerl_amd.ranged_equity(hands, board=board, ranges=ranges, range_of=range_of, samples=S)
ev = pokerl_amd.ranged_ev(hands, board=board, bets=bets, ranges=ranges, range_of=range_of, samples=S)
more = pokerl_amd.ranged_ev(hands, board=board, bets=bets, ranges=ranges, range_of=range_of, samples=S, nonce=1)
both = ev.merged(more)                       # two nonces: the counts add, ev is re-formed from the sums
pot = float(np.sum(bets))
assert ev.accepted == eq.accepted            # the same attempts, card for card
print("attempts accepted: %d of %d (%.1f %%)" % (ev.accepted, S, 100 * ev.acceptance))
print("pot levels (seat visited, chips): %s" % ev.levels)
print("seat  main-pot equity  equity x pot - bet   EV in chips   expected payout")
for p in range(3):
    print("%4d  %15.4f  %18.2f  %12.2f  %16.2f" % (p, eq.equity[p], eq.equity[p] * pot - bets[p], ev.ev[p], ev.payout[p]))
print("the hero's call: main-pot equity says %+.2f chips, the side pots say %+.2f (%+.2f over %d accepted attempts)"
      % (eq.equity[0] * pot - bets[0], ev.ev[0], both.ev[0], both.accepted))
print("sum of EVs: %.6f (chips only move between the seats)" % float(np.sum(ev.ev)))
