#!/usr/bin/env python3
"""A six-seat table before the flop, seen from the big blind: its equity against five opponents whose hands are drawn uniformly
(pk_equity_sampled's model: "they could hold anything") and against the same five on position ranges -- the earlier the seat opened, the
tighter its range (ranged_equity).  The observer's equity moves, most for the hands that ranges dominate.

    python examples/ranged_equity.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pokerl_amd  # noqa: E402
from pokerl_amd import HOLDINGS, ranged_equity  # noqa: E402


def top_range(fraction):
    """uint16 [1326]: weight 1 on the best `fraction` of the holdings in a crude pre-flop order (pairs, then high cards, suited first)."""
    score = []
    for c0, c1 in HOLDINGS.tolist():                                  # HOLDINGS[h]: the two Card.value bytes (suit << 4 | rank) of holding h
        r0, r1 = sorted((c0 & 15, c1 & 15))
        score.append(100 + r1 if r0 == r1 else 2 * r1 + r0 + (3 if c0 >> 4 == c1 >> 4 else 0))
    order = np.argsort(-np.array(score), kind="stable")
    w = np.zeros(len(HOLDINGS), np.uint16)
    w[order[:int(round(fraction * len(HOLDINGS)))]] = 1
    return w


def main():
    if pokerl_amd.device_count() < 1:
        sys.exit("ranged_equity: no MI355X visible (no fallback)")
    # seats 0 .. 4: under the gun, middle, cut-off, button, small blind -- seat 5, the big blind, is the observer
    ranges = np.stack([top_range(f) for f in (0.12, 0.18, 0.25, 0.40, 0.50)])
    print("%-8s %10s %10s %10s" % ("hand", "uniform", "ranges", "accepted"))
    for hand in (["AS", "AD"], ["KH", "QH"], ["AC", "7D"], ["7S", "6S"], ["QD", "8C"]):
        seats = [None] * 5 + [hand]
        uniform = ranged_equity(seats, samples=1 << 16)
        ranged = ranged_equity(seats, ranges=ranges, range_of=[0, 1, 2, 3, 4, 0xFFFF], samples=1 << 18)
        print("%-8s %10.4f %10.4f %9.1f%%" % (" ".join(hand), uniform.equity[5], ranged.equity[5], 100 * ranged.acceptance))


if __name__ == "__main__":
    main()
