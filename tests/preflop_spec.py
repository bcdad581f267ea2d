"""The pre-flop matchup definition restated in numpy (TEST INFRASTRUCTURE): include/pokerl_hip.h "Pre-flop matchups" / DESIGN.md section 3.10
on top of oracle.loader.eval_hands and the LITERAL compare_rankings loop (equity_spec.winners_literal) -- not the device's order key.
Boards are the 5-subsets of the canonical card indices 0 .. 51 in itertools.combinations order; holdings h = b (b - 1) / 2 + a."""
import itertools
import math

import numpy as np

from oracle import loader as O
from equity_spec import CANON, winners_literal

HOLDINGS = 1326
ALL_BOARDS = math.comb(52, 5)          # 2 598 960
PAIR_BOARDS = math.comb(48, 5)         # 1 712 304
BAD_CARD, DUP_CARD = 1, 2
HOLD_A = np.array([a for b in range(52) for a in range(b)], np.int64)     # canonical indices of holding h: HOLD_A[h] < HOLD_B[h]
HOLD_B = np.array([b for b in range(52) for a in range(b)], np.int64)
HOLD_MASK = (np.uint64(1) << HOLD_A.astype(np.uint64)) | (np.uint64(1) << HOLD_B.astype(np.uint64))
CANON_V = np.array(CANON, np.uint8)    # canonical index -> Card.value


def holding_index(a, b):
    """canonical indices of two different cards (either order) -> h."""
    a, b = sorted((int(a), int(b)))
    return b * (b - 1) // 2 + a


def holding_of_values(v0, v1):
    """two Card.value bytes -> h."""
    k = lambda v: (int(v) & 15) * 4 + (int(v) >> 4)
    return holding_index(k(v0), k(v1))


def shared():
    """bool [1326, 1326]: the two holdings share a card (the diagonal included)."""
    return (HOLD_MASK[:, None] & HOLD_MASK[None, :]) != 0


def unrank(r):
    """The board of rank r: five ascending canonical indices (the combinatorial number system of the lexicographic order)."""
    out, x = [], 0
    for left in range(4, -1, -1):          # cards still to choose after this one
        while True:
            n = math.comb(51 - x, left)
            if r < n:
                break
            r -= n
            x += 1
        out.append(x)
        x += 1
    return out


def boards(first, n):
    """int64 [n, 5]: the boards of rank first .. first + n - 1."""
    assert 0 <= first and first + n <= ALL_BOARDS
    out = np.zeros((n, 5), np.int64)
    if n == 0:
        return out
    c = unrank(first)
    for i in range(n):
        out[i] = c
        j = 4                              # the successor in lexicographic order
        while j >= 0 and c[j] == 52 - 5 + j:
            j -= 1
        if j < 0:
            break
        c[j] += 1
        for t in range(j + 1, 5):
            c[t] = c[t - 1] + 1
    return out


_all = []


def all_boards():
    """int8 [2 598 960, 5], made once."""
    if not _all:
        _all.append(np.fromiter(itertools.chain.from_iterable(itertools.combinations(range(52), 5)), np.int8, count=ALL_BOARDS * 5).reshape(ALL_BOARDS, 5))
    return _all[0]


def counts(first, n):
    """(win, tie) uint32 [1326, 1326]: the partial counts over boards first .. first + n - 1, every ordered pair.  Per board the hands of
    the 1 081 holdings in play are evaluated, and the literal winners loop decides every pair of DISTINCT (rank, kickers) values once."""
    win, tie = np.zeros((HOLDINGS, HOLDINGS), np.uint32), np.zeros((HOLDINGS, HOLDINGS), np.uint32)
    for bd in boards(first, n):
        bmask = np.uint64(sum(1 << int(c) for c in bd))
        live = np.nonzero((HOLD_MASK & bmask) == 0)[0]
        hand = np.zeros((len(live), 7), np.uint8)
        hand[:, :5] = CANON_V[bd]
        hand[:, 5] = CANON_V[HOLD_A[live]]
        hand[:, 6] = CANON_V[HOLD_B[live]]
        rank, kick, _ = O.eval_hands(hand)
        val, cls = np.unique((rank.astype(np.int64) << 32) | kick.astype(np.int64), return_inverse=True)
        cr, ck = (val >> 32).astype(np.uint8), (val & 0xFFFFFFFF).astype(np.uint32)
        nc = len(val)
        w = winners_literal(np.stack([np.repeat(cr, nc), np.tile(cr, nc)]), np.stack([np.repeat(ck, nc), np.tile(ck, nc)])).reshape(nc, nc)
        pair = w[cls[:, None], cls[None, :]]
        win[np.ix_(live, live)] += (pair == 1).astype(np.uint32)
        tie[np.ix_(live, live)] += (pair == 3).astype(np.uint32)
    sh = shared()
    win[sh] = 0
    tie[sh] = 0
    return win, tie


def pair_counts(h, o, first=0, n=ALL_BOARDS):
    """(win[h][o], tie[h][o], win[o][h]) over boards first .. first + n - 1 by the literal loop; (0, 0, 0) where the two share a card."""
    if HOLD_MASK[h] & HOLD_MASK[o]:
        return 0, 0, 0
    bd = all_boards()[first:first + n] if n > 4096 else boards(first, n).astype(np.int8)
    dead = [int(HOLD_A[h]), int(HOLD_B[h]), int(HOLD_A[o]), int(HOLD_B[o])]
    keep = ~np.isin(bd, dead).any(axis=1)
    bd = bd[keep]
    hand = np.zeros((len(bd), 7), np.uint8)
    hand[:, :5] = CANON_V[bd.astype(np.int64)]
    rank, kick = np.zeros((2, len(bd)), np.uint8), np.zeros((2, len(bd)), np.uint32)
    for p, x in enumerate((h, o)):
        hand[:, 5], hand[:, 6] = CANON_V[HOLD_A[x]], CANON_V[HOLD_B[x]]
        rank[p], kick[p], _ = O.eval_hands(hand)
    w = winners_literal(rank, kick)
    return int(np.sum(w == 1)), int(np.sum(w == 3)), int(np.sum(w == 2))


def hero_status(hero):
    """The status of a pre-flop range-equity spot (explicit form): hero = two Card.value bytes."""
    status, seen = 0, []
    for c in [int(x) for x in hero]:
        if not (c < 0x40 and (c & 15) < 13):
            status |= BAD_CARD
        else:
            seen.append(c)
    if len(set(seen)) != len(seen):
        status |= DUP_CARD
    return status


def hero_equity(win, tie, hero, weights=None):
    """dict(win [1326], tie [1326], agg [3], boards, status) of one spot on the table (win, tie)."""
    status = hero_status(hero)
    if status:
        return dict(win=np.zeros(HOLDINGS, np.uint32), tie=np.zeros(HOLDINGS, np.uint32), agg=np.zeros(3, np.uint64), boards=0, status=status)
    h = holding_of_values(*hero)
    w = np.ones(HOLDINGS, np.uint64) if weights is None else np.asarray(weights, np.uint64)
    apart = (HOLD_MASK & HOLD_MASK[h]) == 0
    agg = np.array([np.sum(w * win[h].astype(np.uint64)), np.sum(w * tie[h].astype(np.uint64)), np.uint64(PAIR_BOARDS) * np.sum(w[apart])], np.uint64)
    return dict(win=win[h].copy(), tie=tie[h].copy(), agg=agg, boards=PAIR_BOARDS, status=0)


def rvr(win, tie, weights):
    """(win, tie, tot) uint64 [m, 1326] of pre-flop range vs range on the table: weights uint16 [m, 1326]."""
    w = np.asarray(weights, np.uint64)
    apart = (~shared()).astype(np.uint64)
    return (w @ win.astype(np.uint64).T, w @ tie.astype(np.uint64).T, np.uint64(PAIR_BOARDS) * (w @ apart.T))
