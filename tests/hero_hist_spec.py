"""The hero-strength-histogram definition restated in numpy (TEST INFRASTRUCTURE): include/pokerl_hip.h "Hero strength histogram" / DESIGN.md
section 3.9 on top of oracle.loader.eval_hands and equity_spec.winners_literal, per hero and per completion.  The hero's hand is evaluated
once per completion; every (completion, villain holding) pair that shares no card is a row of its own, evaluated and decided by
winners_literal; the weights the hero beats / ties / meets are summed per completion in int64 and the bin of each completion is computed in
PYTHON INTEGERS, one at a time.  There is no sort and no comparison of ranking words here, and hist_spec is not used.  The spot check is
equity_range_spec.check_spot: the two families share it."""
import itertools
import math

import numpy as np

import equity_range_spec as RS
import equity_spec as ES
from oracle import loader as O

HOLDINGS = RS.HOLDINGS
MAX_BINS = 32
CANON = RS.CANON


def bin_of(below, equal, den, nbins):
    """The bin rule in Python integers; None = void (den = 0)."""
    below, equal, den, nbins = int(below), int(equal), int(den), int(nbins)
    assert 1 <= nbins <= MAX_BINS and below >= 0 and equal >= 0 and below + equal <= den
    if den == 0:
        return None
    return min(nbins - 1, (nbins * (2 * below + equal)) // (2 * den))


def completion_terms(hero, board, nb, pool, w):
    """(below, equal, den) int64 [r, C(P, k)] of a good spot: per range of w [r, 1326] and per completion of the board from `pool`
    (canonical indices in canonical order, the hero's cards not among them), in itertools.combinations order."""
    p, k = len(pool), 5 - nb
    pool = np.asarray(pool, np.int64)
    pv = np.array([CANON[c] for c in pool], np.uint8)
    comps = np.array(list(itertools.combinations(range(p), k)), np.int64).reshape(math.comb(p, k), k)   # completions as pool slots
    hold = np.array(list(itertools.combinations(range(p), 2)), np.int64)                                  # holdings as pool slots a < b
    clash = np.zeros((len(comps), len(hold)), bool)
    for j in range(k):
        clash |= (comps[:, j, None] == hold[None, :, 0]) | (comps[:, j, None] == hold[None, :, 1])
    ci, hi = np.nonzero(~clash)                                      # every (completion, villain holding in V(c)): a row of its own
    hand = np.zeros((len(comps), 7), np.uint8)
    hand[:, :nb] = np.asarray(board[:nb], np.uint8)
    hand[:, nb:5] = pv[comps]
    hand[:, 5:] = np.asarray(hero, np.uint8)
    hr, hk, _ = O.eval_hands(hand)                                   # the hero: once per completion
    rows = np.zeros((len(ci), 7), np.uint8)
    rows[:, :5] = hand[ci, :5]
    rows[:, 5:] = pv[hold[hi]]
    vr, vk, _ = O.eval_hands(rows)                                   # the villain: once per (completion, holding)
    res = ES.winners_literal(np.stack([hr[ci], vr]), np.stack([hk[ci], vk]))
    hidx = pool[hold[:, 1]] * (pool[hold[:, 1]] - 1) // 2 + pool[hold[:, 0]]
    r = w.shape[0]
    below, equal, den = (np.zeros((r, len(comps)), np.int64) for _ in range(3))
    for i in range(r):
        wl = w[i, hidx[hi]]
        np.add.at(below[i], ci, wl * (res == 1))
        np.add.at(equal[i], ci, wl * (res == 3))
        np.add.at(den[i], ci, wl)
    return below, equal, den


def spot_hero_hist(hero, board, nb, dead=0, weights=None, bins=10):
    """One spot -> dict(hist uint16 [bins], void, completions, status).  weights: None (ones), [1326] integers, or [r, 1326] -- r ranges at
    once over the same decisions: hist / void are then [r, bins] / [r].  bins: an int, or a tuple of ints -- `hist` is then a dict
    {bins: array}."""
    many = weights is not None and np.ndim(weights) == 2
    w = np.ones((1, HOLDINGS), np.int64) if weights is None else np.atleast_2d(np.asarray(weights, np.int64))
    r = w.shape[0]
    blist = tuple(bins) if isinstance(bins, (tuple, list)) else (int(bins),)
    assert all(1 <= b <= MAX_BINS for b in blist)
    hist = {b: np.zeros((r, b), np.int64) for b in blist}
    void = np.zeros(r, np.int64)
    completions = 0
    status, gone = RS.check_spot(hero, board, nb, dead)
    if not status:
        nb = int(nb)
        pool = [k for k in range(52) if k not in gone]               # canonical indices, canonical order
        completions = math.comb(len(pool), 5 - nb)
        below, equal, den = completion_terms(hero, board, nb, pool, w)
        assert below.shape[1] == completions
        for i in range(r):
            for lo, eq, dn in zip(below[i].tolist(), equal[i].tolist(), den[i].tolist()):   # Python integers
                if dn == 0:
                    void[i] += 1
                    continue
                for b in blist:
                    hist[b][i, bin_of(lo, eq, dn, b)] += 1
    hist = {b: v.astype(np.uint16) for b, v in hist.items()}
    void = void.astype(np.uint16)
    if not many:
        hist, void = {b: v[0] for b, v in hist.items()}, void[0]
    if not isinstance(bins, (tuple, list)):
        hist = hist[blist[0]]
    return dict(hist=hist, void=void, completions=completions, status=status)


def batch_hero_hist(hero, board, nboard, dead=None, weights=None, bins=10):
    """The batch form -> dict of [m, bins] / [m] arrays (weights: None, [1326] or [m, 1326]; bins: an int)."""
    hero = np.asarray(hero, np.uint8)
    m = hero.shape[0]
    out = dict(hist=np.zeros((m, bins), np.uint16), void=np.zeros(m, np.uint16), completions=np.zeros(m, np.uint32), status=np.zeros(m, np.uint8))
    for i in range(m):
        w = None if weights is None else (np.asarray(weights)[i] if np.ndim(weights) == 2 else weights)
        r = spot_hero_hist(hero[i], [int(x) for x in board[i]], int(nboard[i]), 0 if dead is None else int(dead[i]), w, bins)
        for key in out:
            out[key][i] = r[key]
    return out
