#!/usr/bin/env python3
"""Strength histograms on one flop (pk_equity_hist): what distribution-aware card abstraction, or a "hand potential" feature, needs.  One call
gives, for EVERY holding the hero can have, the histogram of its RIVER strength against the opponent's range over the 1 081 turn-and-river
cards still to come.  Three holdings that tell the mean apart from the distribution: a flush draw (mostly weak, sometimes the nuts), a
middle pair (mostly middling) and top pair -- their means, their histograms, and the earth mover's distances between them
(pokerl_amd.histogram_emd: the L1 distance of the CDFs, in bin units), which is what a clustering of holdings into buckets compares.

    python examples/strength_histogram.py [board="KS 9D 4D"] [bins=10]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pokerl_amd  # noqa: E402

board = (sys.argv[1] if len(sys.argv) > 1 else "KS 9D 4D").split()
bins = int(sys.argv[2]) if len(sys.argv) > 2 else 10
holdings = [("flush draw", ["AD", "5D"]), ("middle pair", ["9S", "8S"]), ("top pair", ["KH", "QC"])]

r = pokerl_amd.strength_histogram(board, bins=bins)                  # the opponent: any two cards
print("board %s: %d holdings possible, %d completions each, %d bins" % (" ".join(board), int(r.valid.sum()), int(r.completions), r.bins))
centres = (np.arange(bins) + 0.5) / bins
idx = [pokerl_amd.holding_index(*cards) for _, cards in holdings]
for (name, cards), h in zip(holdings, idx):
    assert r.valid[h] and int(r.hist[h].sum()) + int(r.void[h]) == int(r.completions)   # the row-sum invariant
    pdf = r.pdf[h]
    print("  %-11s %s  mean strength ~%.3f  %s" % (name, " ".join(cards), float((pdf * centres).sum()), " ".join("%4d" % c for c in r.hist[h])))
print("earth mover's distance, in bins (0 = the same distribution):")
for i in range(len(idx)):
    for j in range(i + 1, len(idx)):
        print("  %-11s - %-11s %.3f" % (holdings[i][0], holdings[j][0], pokerl_amd.histogram_emd(r.hist[idx[i]], r.hist[idx[j]])))
# the holding nearest to the flush draw in distribution
d = pokerl_amd.histogram_emd(r.hist, r.hist[idx[0]])
d[~r.valid] = np.inf
d[idx[0]] = np.inf
near = int(np.argmin(d))
print("nearest to the flush draw: %s (%.3f bins)" % (" ".join("A23456789TJQK"[int(c) & 15] + "SHDC"[int(c) >> 4] for c in pokerl_amd.HOLDINGS[near]), d[near]))
