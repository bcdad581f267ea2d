#!/usr/bin/env python3
"""The bucket of the hand of the seat to act, per step: centroids learned once from the strength histograms of a few boards
(strength_histogram_batch + cluster_histograms), then a table played by random agents, and at every post-flop decision the acting seat's
bucket from ONE call, g.bucket(centroids) -- pk_table_equity_hist_hero: the seat's own strength histogram (the cost of one range-equity
spot, not of the 1 326-row public form) and the nearest centroid, on the device.

    python examples/bucket_of_the_seat_to_act.py [K=8] [bins=10] [steps=40]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pokerl_amd  # noqa: E402
from pokerl_amd.cards import card_value  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 8
bins = int(sys.argv[2]) if len(sys.argv) > 2 else 10
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 40
train = ["KS 9D 4D 2C", "7H 8H 9C TS", "AS AD 5C 5H", "QC 6D 3S 2H", "JD TD 4S 2S 2D", "8C 8D 3H KD AC"]

board = np.zeros((len(train), 5), np.uint8)
nboard = np.zeros(len(train), np.uint8)
for i, t in enumerate(train):
    cards = [card_value(c) for c in t.split()]
    board[i, :len(cards)], nboard[i] = cards, len(cards)
hists = pokerl_amd.strength_histogram_batch(board, nboard, bins=bins)
clusters = pokerl_amd.cluster_histograms(hists.hist, K, iters=12, nonce=1)
centroids = clusters.centroids                                       # uint16 [K, bins]: quantised CDFs
mean = (bins - centroids.astype(np.float64).sum(axis=1) / 65535.0 + 0.5) / bins
print("%d boards -> %d buckets of %d-bin histograms; mean strength per bucket: %s" %
      (len(train), K, bins, " ".join("%.2f" % x for x in mean)))

g = pokerl_amd.Game(num_players=3, seed=7)
g.reset()
rng = np.random.default_rng(1)
street = {0: "pre-flop", 1: "flop", 2: "turn", 3: "river"}
for step in range(steps):
    v = g._v
    turn, seat = int(v.turn[0]), int(v.active_player[0])
    if turn == 0:
        what = "(pre-flop: no bucket)"
    else:
        r = g.equity_hist_hero(bins=bins, centroids=centroids)
        assert g.bucket(centroids) == int(r.label)                   # the label alone: the histogram stays on the device
        what = "bucket %d (mean strength ~%.2f, %.2f bins from its centroid), histogram %s" % (int(r.label), mean[int(r.label)], float(r.emd), r.hist.tolist())
    print("step %2d  %-8s seat %d  %s" % (step, street[turn], seat, what))
    onehot, _ = g.get_valid_actions()
    over, _, _ = g.step(int(rng.choice(np.flatnonzero(onehot))))
    if over:
        g.reset()
g.close()
