#!/usr/bin/env python3
"""Distribution-aware card abstraction on the device: the strength histograms of a few turn boards (pk_equity_hist_d), clustered into K buckets
by exact k-means under the earth mover's distance (pk_hist_cluster_seed_d + pk_hist_cluster_d), and a NEW board's holdings assigned to the
learned buckets (pk_hist_cluster_assign_d).  The histograms are written by one kernel family and read by the other in device memory: they
are never copied to the host -- only the centroids, the labels and the distances are, to print them.

    python examples/bucket_histograms.py [K=8] [bins=10]
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pokerl_amd  # noqa: E402
from pokerl_amd import hipmem  # noqa: E402
from pokerl_amd.cards import card_value  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 8
bins = int(sys.argv[2]) if len(sys.argv) > 2 else 10
H, ITERS = 1326, 12
train = ["KS 9D 4D 2C", "7H 8H 9C TS", "AS AD 5C 5H", "QC 6D 3S 2H"]
new = "JD TD 4S 2S"


def boards_d(texts):
    b = np.zeros((len(texts), 5), np.uint8)
    for i, t in enumerate(texts):
        b[i, :4] = [card_value(c) for c in t.split()]
    return hipmem.DeviceBuffer(b.nbytes).upload(b), hipmem.DeviceBuffer(len(texts)).upload(np.full(len(texts), 4, np.uint8))


hip = hipmem._lib()
stream = C.c_void_p()
assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
m, n = len(train), len(train) * H
b_d, nb_d = boards_d(train)
hist_d = hipmem.DeviceBuffer(n * bins * 2)                          # u16 [m][1326][bins]: stays on the device
pokerl_amd.strength_histogram_d(m, b_d.ptr, nb_d.ptr, bins=bins, hist_d=hist_d.ptr, stream=stream)
cen_d, label_d, dist_d = hipmem.DeviceBuffer(K * bins * 2), hipmem.DeviceBuffer(n * 2), hipmem.DeviceBuffer(n * 4)
inertia_d, changed_d = hipmem.DeviceBuffer((ITERS + 1) * 8), hipmem.DeviceBuffer(ITERS * 4)
pokerl_amd.seed_histogram_centroids_d(n, bins, hist_d.ptr, K, cen_d.ptr, nonce=1, stream=stream)
pokerl_amd.cluster_histograms_d(n, bins, hist_d.ptr, K, cen_d.ptr, ITERS, label_d.ptr, dist_d.ptr, inertia_d.ptr, changed_d.ptr, stream=stream)
assert hip.hipStreamSynchronize(stream) == 0
cen = cen_d.download(np.uint16, K * bins).reshape(K, bins)
labels, dist = label_d.download(np.uint16, n), dist_d.download(np.uint32, n)
inertia, changed = inertia_d.download(np.uint64, ITERS + 1), changed_d.download(np.uint32, ITERS)
live = labels != 0xFFFF                                             # PK_CL_NONE: a holding that shares a card with its board
print("%d turn boards x 1326 holdings = %d rows (%d possible), %d bins, K = %d, %d iterations: labels changed %s" %
      (m, n, int(live.sum()), bins, K, ITERS, changed.tolist()))
print("mean earth mover's distance to the bucket's centroid: %.3f bins before, %.3f after" %
      (float(inertia[0]) / 65535 / live.sum(), float(inertia[-1]) / 65535 / live.sum()))
# a centroid is a CDF in units of 1 / 65535: its mean strength is (bins - sum of the CDF) / bins, up to half a bin
mean = (bins - cen.astype(np.float64).sum(axis=1) / 65535.0 + 0.5) / bins
for c in np.argsort(mean):
    print("  bucket %2d: %5d holdings, mean strength ~%.3f" % (c, int((labels == c).sum()), mean[c]))
# a new board: its histograms, then the learned buckets
b2_d, nb2_d = boards_d([new])
hist2_d, label2_d, dist2_d = hipmem.DeviceBuffer(H * bins * 2), hipmem.DeviceBuffer(H * 2), hipmem.DeviceBuffer(H * 4)
pokerl_amd.strength_histogram_d(1, b2_d.ptr, nb2_d.ptr, bins=bins, hist_d=hist2_d.ptr, stream=stream)
pokerl_amd.assign_histograms_d(H, bins, hist2_d.ptr, K, cen_d.ptr, label2_d.ptr, dist2_d.ptr, stream=stream)
assert hip.hipStreamSynchronize(stream) == 0
l2, d2 = label2_d.download(np.uint16, H), dist2_d.download(np.uint32, H)
print("new board %s: holdings per learned bucket %s, mean distance %.3f bins" %
      (new, np.bincount(l2[l2 != 0xFFFF], minlength=K).tolist(), float(d2[l2 != 0xFFFF].mean()) / 65535))
for name, cards in (("flush draw", ["AD", "5D"]), ("top pair", ["JH", "9C"]), ("air", ["7C", "3H"])):
    h = pokerl_amd.holding_index(*cards)
    print("  %-10s %s -> bucket %d (mean strength ~%.3f)" % (name, " ".join(cards), int(l2[h]), mean[int(l2[h])]))
assert hip.hipStreamDestroy(stream) == 0
