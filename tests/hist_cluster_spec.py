"""Histogram clustering restated in numpy (TEST INFRASTRUCTURE -- never imported by the product): the quantised CDF, the assignment with its
smallest-index tie rule, the rounded-mean update, the iteration and the exact k-means++ seeding of include/pokerl_hip.h "Histogram
clustering" (DESIGN.md section 3.8).  Everything is an integer: the device must equal this bit for bit.  The row-by-centroid distance matrix
is built in chunks of rows so that it stays a few megabytes."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import rng_spec  # noqa: E402

NONE = 0xFFFF            # PK_CL_NONE
MAX_K = 4096             # PK_CL_MAX_K
MAX_BINS = 32            # PK_EQ_HIST_MAX_BINS
MAX_ITERS = 1024
STREAM_CLS = 0x434C5330  # 'CLS0'
ONE = 65535
CHUNK_CELLS = 1 << 22    # rows * K * nbins of one chunk of the distance matrix


def quant(hist):
    """hist [n, nbins] counts -> (q uint16 [n, nbins], empty bool [n]).  q = floor(65535 * running sum / mass); an empty row is all zeros."""
    hist = np.asarray(hist)
    assert hist.ndim == 2 and 1 <= hist.shape[1] <= MAX_BINS and hist.shape[0] >= 1
    h = hist.astype(np.int64)
    mass = h.sum(axis=1)
    empty = mass == 0
    cum = np.cumsum(h, axis=1)
    q = (ONE * cum) // np.where(empty, 1, mass)[:, None]
    q[empty] = 0
    assert (q[~empty, -1] == ONE).all() and (np.diff(q, axis=1) >= 0).all() and q.max(initial=0) <= ONE
    return q.astype(np.uint16), empty


def distances(q, C):
    """d(i, c) for every row and centroid: int64 [n, K] (small inputs only)."""
    return np.abs(q.astype(np.int64)[:, None, :] - np.asarray(C).astype(np.int64)[None, :, :]).sum(axis=2)


def assign(q, empty, C):
    """-> (label uint16 [n], dist uint32 [n]): the SMALLEST c among the minimisers (np.argmin returns the first), PK_CL_NONE / 0 for an empty row."""
    C = np.asarray(C)
    n, nb = q.shape
    K = C.shape[0]
    assert C.shape == (K, nb) and 1 <= K <= MAX_K
    label, dist = np.full(n, NONE, np.uint16), np.zeros(n, np.uint32)
    Ci = C.astype(np.int32)[None, :, :]
    step = max(1, CHUNK_CELLS // (K * nb))
    for a in range(0, n, step):
        d = np.abs(q[a:a + step].astype(np.int32)[:, None, :] - Ci).sum(axis=2, dtype=np.int64)
        c = np.argmin(d, axis=1)
        label[a:a + step] = c
        dist[a:a + step] = d[np.arange(len(c)), c]
    label[empty] = NONE
    dist[empty] = 0
    return label, dist


def update(q, label, C):
    """The rounded means; a cluster with no row keeps its centroid.  Asserts the last bin stays 65535 for a cluster that has rows (every
    summand is 65535) and the rows stay non-decreasing (rounded means of non-decreasing rows, the same n_c in every bin)."""
    C = np.asarray(C)
    K, nb = C.shape
    live = label != NONE
    lab = label[live].astype(np.int64)
    counts = np.bincount(lab, minlength=K)
    out = C.astype(np.int64).copy()
    has = counts > 0
    for b in range(nb):
        S = np.zeros(K, np.int64)
        np.add.at(S, lab, q[live, b].astype(np.int64))
        out[has, b] = (S[has] + counts[has] // 2) // counts[has]
    assert (out[has, -1] == ONE).all() and (np.diff(out[has], axis=1) >= 0).all()
    return out.astype(np.uint16), counts


def iterate(q, empty, C, iters):
    """EXACTLY `iters` iterations (assign, update) and one final assign -> dict(centroids, labels, dist, inertia uint64 [iters + 1], changed
    uint32 [iters])."""
    assert 1 <= iters <= MAX_ITERS
    C = np.asarray(C, np.uint16).copy()
    inertia, changed = np.zeros(iters + 1, np.uint64), np.zeros(iters, np.uint32)
    prev = None
    for t in range(iters):
        label, dist = assign(q, empty, C)
        inertia[t] = int(dist.sum(dtype=np.uint64))
        changed[t] = int((~empty).sum()) if prev is None else int((label != prev).sum())
        C, _ = update(q, label, C)
        prev = label
    label, dist = assign(q, empty, C)
    inertia[iters] = int(dist.sum(dtype=np.uint64))
    return dict(centroids=C, labels=label, dist=dist, inertia=inertia, changed=changed)


def draw(seed, nonce, j, W):
    """r = (x * W) >> 64 for round j: x = w0 | w1 << 32 of the Philox block (j, 0, 'CLS0', nonce) under the key of `seed` (as pk_create)."""
    w = rng_spec.philox4x32_10((j & 0xFFFFFFFF, 0, STREAM_CLS, nonce & 0xFFFFFFFF), rng_spec.seed_key(seed))
    return ((w[0] | (w[1] << 32)) * int(W)) >> 64


def pick(weights, r):
    """The smallest i whose inclusive prefix sum of the weights exceeds r."""
    cum = np.cumsum(np.asarray(weights, np.uint64), dtype=np.uint64)
    return int(np.searchsorted(cum, np.uint64(r), side="right"))


def seed(q, empty, K, seed_, nonce=0):
    """k-means++ with linear weights -> (centroids uint16 [K, nbins], the chosen rows).  ValueError when there is no non-empty row."""
    n, nb = q.shape
    assert 1 <= K <= MAX_K
    if empty.all():
        raise ValueError("no non-empty row")
    first = int(np.flatnonzero(~empty)[0])
    C, rows = np.zeros((K, nb), np.uint16), []
    mind = None
    for j in range(K):
        w = (~empty).astype(np.uint64) if j == 0 else mind
        W = int(w.sum(dtype=np.uint64))
        i = first if W == 0 else pick(w, draw(seed_, nonce, j, W))
        assert not empty[i]
        C[j] = q[i]
        rows.append(i)
        d = np.abs(q.astype(np.int64) - q[i].astype(np.int64)[None, :]).sum(axis=1).astype(np.uint64)
        d[empty] = 0
        mind = d if mind is None else np.minimum(mind, d)
    return C, rows


def latent_rows(rng, n, nbins, mass=46, shapes=12, empty_frac=0.1):
    """Synthetic rows of one mass drawn from a few latent shapes (multinomial), a fraction of them empty: uint16 [n, nbins]."""
    p = rng.dirichlet(np.full(nbins, 0.7), size=shapes)
    which = rng.integers(0, shapes, n)
    hist = np.zeros((n, nbins), np.uint16)
    for s in range(shapes):
        idx = np.flatnonzero(which == s)
        hist[idx] = rng.multinomial(mass, p[s], size=len(idx))
    hist[rng.random(n) < empty_frac] = 0
    return hist
