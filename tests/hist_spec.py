"""The strength-histogram definition restated in numpy (TEST INFRASTRUCTURE): include/pokerl_hip.h "Strength histograms" / DESIGN.md section
3.5 on top of oracle.loader.eval_hands and equity_spec.winners_literal.  Per completion of the board every holding is evaluated once; every
ORDERED disjoint (hero, villain) pair is then decided by winners_literal as a row of its own, as rvr_spec.py does -- there is no sort and no
comparison of ranking words here -- and the weights below / equal / of all villains are summed per hero.  The bin of each (holding,
completion) is then computed in PYTHON INTEGERS, one at a time.  The spot check is rvr_spec.check_spot: the two families share it."""
import itertools
import math

import numpy as np

import equity_spec as ES
import rvr_spec as VS
from oracle import loader as O

HOLDINGS = VS.HOLDINGS
MAX_BINS = 32
CANON = VS.CANON


def bin_of(below, equal, den, nbins):
    """The bin rule in Python integers; None = void (den = 0)."""
    below, equal, den, nbins = int(below), int(equal), int(den), int(nbins)
    assert 1 <= nbins <= MAX_BINS and below >= 0 and equal >= 0 and below + equal <= den
    if den == 0:
        return None
    return min(nbins - 1, (nbins * (2 * below + equal)) // (2 * den))


def completion_terms(board, nb, pool, w):
    """For each completion of the board from `pool` (canonical indices in canonical order): (hidx [n], below [r, n], equal [r, n], den [r, n])
    over the n holdings in play, under each of the r ranges w [r, 1326] (int64)."""
    p, k = len(pool), 5 - nb
    pv = np.array([CANON[c] for c in pool], np.uint8)
    for comp in itertools.combinations(range(p), k):
        rest = [s for s in range(p) if s not in comp]
        hold = np.array(list(itertools.combinations(rest, 2)), np.int64)          # the holdings in play, as pool slots a < b
        n = len(hold)
        hand = np.zeros((n, 7), np.uint8)
        hand[:, :nb] = np.asarray(board[:nb], np.uint8)
        hand[:, nb:5] = pv[list(comp)]
        hand[:, 5:] = pv[hold]
        hr, hk, _ = O.eval_hands(hand)                                             # every holding: once per completion
        hidx = pool[hold[:, 1]] * (pool[hold[:, 1]] - 1) // 2 + pool[hold[:, 0]]
        share = (hold[:, None, 0] == hold[None, :, 0]) | (hold[:, None, 0] == hold[None, :, 1]) | \
                (hold[:, None, 1] == hold[None, :, 0]) | (hold[:, None, 1] == hold[None, :, 1])
        hi, vi = np.nonzero(~share)                                                # every ordered disjoint pair: a row of its own
        res = ES.winners_literal(np.stack([hr[hi], hr[vi]]), np.stack([hk[hi], hk[vi]]))
        alone, both = np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
        alone[hi, vi] = res == 1
        both[hi, vi] = res == 3
        wl = w[:, hidx]                                                            # [r, n]
        yield hidx, wl @ alone.T, wl @ both.T, wl @ (~share).astype(np.int64).T


def spot_hist(board, nb, dead=0, weights=None, bins=10):
    """One spot -> dict(hist uint16 [1326, bins], void uint16 [1326], valid [1326] bool, completions, status).  weights: None (ones), [1326]
    integers, or [r, 1326] -- r ranges at once over the same pairwise decisions: hist / void are then [r, 1326, bins] / [r, 1326].  bins: an
    int, or a tuple of ints -- `hist` is then a dict {bins: array}."""
    many = weights is not None and np.ndim(weights) == 2
    w = np.ones((1, HOLDINGS), np.int64) if weights is None else np.atleast_2d(np.asarray(weights, np.int64))
    r = w.shape[0]
    blist = tuple(bins) if isinstance(bins, (tuple, list)) else (int(bins),)
    assert all(1 <= b <= MAX_BINS for b in blist)
    hist = {b: np.zeros((r, HOLDINGS, b), np.int64) for b in blist}
    void = np.zeros((r, HOLDINGS), np.int64)
    valid = np.zeros(HOLDINGS, bool)
    completions = 0
    status, gone = VS.check_spot(board, nb, dead)
    if not status:
        nb = int(nb)
        pool = np.array([k for k in range(52) if k not in gone])     # canonical indices, canonical order
        completions = math.comb(len(pool) - 2, 5 - nb)
        for hidx, below, equal, den in completion_terms(board, nb, pool, w):
            valid[hidx] = True
            for i in range(r):
                for h, lo, eq, dn in zip(hidx.tolist(), below[i].tolist(), equal[i].tolist(), den[i].tolist()):   # Python integers
                    if dn == 0:
                        void[i, h] += 1
                        continue
                    for b in blist:
                        hist[b][i, h, bin_of(lo, eq, dn, b)] += 1
    assert all(int(v.max(initial=0)) < 65536 for v in hist.values())
    hist = {b: v.astype(np.uint16) for b, v in hist.items()}
    void = void.astype(np.uint16)
    if not many:
        hist, void = {b: v[0] for b, v in hist.items()}, void[0]
    if not isinstance(bins, (tuple, list)):
        hist = hist[blist[0]]
    return dict(hist=hist, void=void, valid=valid, completions=completions, status=status)


def batch_hist(board, nboard, dead=None, weights=None, bins=10):
    """The batch form -> dict of [m, 1326, bins] / [m, 1326] / [m] arrays (weights: None, [1326] or [m, 1326]; bins: an int)."""
    board = np.asarray(board, np.uint8)
    m = board.shape[0]
    out = dict(hist=np.zeros((m, HOLDINGS, bins), np.uint16), void=np.zeros((m, HOLDINGS), np.uint16), valid=np.zeros((m, HOLDINGS), bool),
               completions=np.zeros(m, np.uint32), status=np.zeros(m, np.uint8))
    for i in range(m):
        w = None if weights is None else (np.asarray(weights)[i] if np.ndim(weights) == 2 else weights)
        r = spot_hist([int(x) for x in board[i]], int(nboard[i]), 0 if dead is None else int(dead[i]), w, bins)
        for key in out:
            out[key][i] = r[key]
    return out


def one_hot_sum(win, tie, tot, live, bins):
    """The river decomposition's host side: win / tie / tot [n, 1326] = the pk_equity_rvr rows of the n completed river boards of a spot,
    live bool [n, 1326] = the holdings that share no card with each completion and are valid -> (hist [1326, bins], void [1326]) as the
    sum of the one-hot bins of those rows.  numpy int64 (every product < 2^32: the header's bound)."""
    win, tie, tot = (np.asarray(x).astype(np.int64) for x in (win, tie, tot))
    num, den2 = bins * (2 * win + tie), 2 * tot
    some = live & (tot > 0)
    b = np.minimum(bins - 1, num // np.where(den2 > 0, den2, 1))
    hist = np.zeros((HOLDINGS, bins), np.int64)
    rows, cols = np.nonzero(some)
    np.add.at(hist, (cols, b[rows, cols]), 1)
    void = (live & (tot == 0)).sum(axis=0)
    return hist.astype(np.uint16), void.astype(np.uint16)


def river_boards(board, nb, dead=0):
    """The completed river boards of a good spot: (boards uint8 [n, 5], live bool [n, 1326]) -- live[c, h]: holding h is valid and shares
    no card with completion c.  n = C(P, 5 - nb): every completion of the board from the pool."""
    status, gone = VS.check_spot(board, nb, dead)
    assert status == 0
    nb = int(nb)
    pool = [k for k in range(52) if k not in gone]
    combos = list(itertools.combinations(pool, 5 - nb))
    out = np.zeros((len(combos), 5), np.uint8)
    out[:, :nb] = np.asarray(board[:nb], np.uint8)
    free = np.zeros(52, bool)
    free[pool] = True
    live = np.zeros((len(combos), HOLDINGS), bool)
    for i, comp in enumerate(combos):
        out[i, nb:] = [CANON[c] for c in comp]
        f = free.copy()
        f[list(comp)] = False
        live[i] = f[VS.PAIR_A] & f[VS.PAIR_B]
    return out, live


def fixture_weights(ref, spot, case):
    """The weight vector of a fixture case (tests/golden/hist_ref.json): None for "ones", the recorded random vector, or the spot's dying
    range -- weight 1 + a on the holdings {a, dying_card}, a < dying_card, zero elsewhere (make_hist_golden.py)."""
    if case == "ones":
        return None
    if case == "random":
        return np.array(ref["weights"], np.uint16)
    assert case == "dying"
    w = np.zeros(HOLDINGS, np.uint16)
    last = spot["dying_card"]
    for a in range(last):
        w[last * (last - 1) // 2 + a] = 1 + a
    return w


def fixture_expected(spot, case, bins):
    """(hist uint16 [1326, bins], void uint16 [1326], valid bool [1326]) of a fixture case, from its sparse cells."""
    h = np.array(spot["h"])
    hist, void, valid = np.zeros((HOLDINGS, bins), np.uint16), np.zeros(HOLDINGS, np.uint16), np.zeros(HOLDINGS, bool)
    valid[h] = True
    void[h] = spot["cases"][case]["void"]
    for i, j, n in spot["cases"][case]["hist"][str(bins)]:
        hist[h[i], j] = n
    return hist, void, valid
