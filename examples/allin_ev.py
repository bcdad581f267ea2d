#!/usr/bin/env python3
"""A short stack called by two bigger ones: main-pot equity against the EV in chips.

Seat 0 is all in for 20 with aces; seats 1 and 2 have put in 100 each with kings and queens.  showdown_equity answers "who wins when every
live seat is compared" -- the main pot.  showdown_ev pays the pot out the way Game.end_hand does: a main pot of 60 that all three contest
and a side pot of 160 that only seats 1 and 2 can win, each judged over every board still to come."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pokerl_amd  # noqa: E402

hands = [["AS", "AH"], ["KS", "KH"], ["QS", "QH"]]
board = ["2C", "7D", "9H"]
bets = [20.0, 100.0, 100.0]

eq = pokerl_amd.showdown_equity(hands, board=board)
ev = pokerl_amd.showdown_ev(hands, board=board, bets=bets)
pot = float(np.sum(bets))
print("boards enumerated: %d" % ev.boards)
print("pot levels (seat visited, chips): %s" % ev.levels)
print("seat  main-pot equity  equity x pot - bet   EV in chips   expected payout")
for p in range(3):
    print("%4d  %15.4f  %18.2f  %12.2f  %16.2f" % (p, eq.equity[p], eq.equity[p] * pot - bets[p], ev.ev[p], ev.payout[p]))
print("sum of EVs: %.6f (chips only move between the seats)" % float(np.sum(ev.ev)))
