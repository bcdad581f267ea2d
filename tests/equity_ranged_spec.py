"""The ranged-sampled-equity definition restated in Python (TEST INFRASTRUCTURE): include/pokerl_hip.h "Ranged sampled equity" / DESIGN.md
section 3.6, literally, on top of oracle.rng_spec.philox4x32_10 (over all attempt indices at once), oracle.loader.eval_hands,
equity_spec.winners_literal (through equity_sampled_spec.count) and equity_sampled_spec.check_spot.  The holding is np.cumsum +
np.searchsorted(cum, u, side="right"), the rejection a Python set, the board `pool.pop(c)` -- not the device's LDS search and bit select."""
import numpy as np

import equity_sampled_spec as SS
import equity_spec as ES
from oracle import rng_spec as R

STREAM_EQW = 0x45515730          # 'EQW0'
HOLDINGS = 1326
MAX_RANGES = 16
UNIFORM = 0xFFFF
SAMPLES_MAX = 1 << 24
DEFAULT_SEED = R.DEFAULT_SEED
OBSERVER_NONE, OBSERVER_ACTIVE = -1, -2
KEYS = ("win", "tie", "share", "accepted", "status")
PAIR_A = [a for b in range(52) for a in range(b)]                   # holding h = b (b - 1) / 2 + a, canonical indices a < b
PAIR_B = [b for b in range(52) for a in range(b)]


def holding_index(c0, c1):
    """h of two Card.value bytes."""
    a, b = sorted((ES.CANON.index(int(c0)), ES.CANON.index(int(c1))))
    return b * (b - 1) // 2 + a


def as_ranges(weights):
    """None / [1326] / [R, 1326] -> uint16 [R, 1326]."""
    if weights is None:
        return np.zeros((0, HOLDINGS), np.uint16)
    w = np.asarray(weights, np.uint16)
    return w.reshape(1, HOLDINGS) if w.ndim == 1 else w


def check_spot(holes, board, nb, live, range_of, num_ranges):
    """(status, dead set, live mask, hidden seats ascending): equity_sampled_spec.check_spot plus this family's rules -- a live seat with
    exactly one 0xFF, and a range row >= R (other than 0xFFFF) at a hidden seat, are BAD_CARD."""
    holes = np.asarray(holes, np.uint8)
    n = holes.shape[0]
    status, dead, live, slots = SS.check_spot(holes, board, nb, live)
    hidden = []
    for p in range(n):
        if not (live >> p) & 1:
            continue
        unknown = [int(holes[p, b]) == ES.UNKNOWN for b in range(2)]
        if unknown[0] != unknown[1]:
            status |= ES.BAD_CARD
        if all(unknown):
            hidden.append(p)
            ro = UNIFORM if range_of is None else int(range_of[p])
            if ro != UNIFORM and ro >= num_ranges:
                status |= ES.BAD_CARD
    return status, dead, live, hidden


def words(key, ident, nonce, nwords, samples):
    """X[j] of every attempt, as (low, high) uint64 arrays of 32-bit halves: X[2b] = w0 | w1 << 32, X[2b + 1] = w2 | w3 << 32 of block b."""
    s = np.arange(samples, dtype=np.uint64)
    same = np.zeros(samples, np.uint64)
    x = []
    for b in range((nwords + 1) // 2):
        w = R.philox4x32_10((same + np.uint64(ident & R.MASK32), s, same + np.uint64((STREAM_EQW + b) & R.MASK32), same + np.uint64(nonce & R.MASK32)), key)
        x += [(w[0], w[1]), (w[2], w[3])]
    return x[:nwords]


def mulhi(x, t):
    """((x * t) >> 64, x * t mod 2^64 as halves) for x = (low, high) halves and t < 2^32: every product < 2^64."""
    t = np.uint64(t)
    a = x[0] * t
    b = x[1] * t + (a >> np.uint64(32))
    return (b >> np.uint64(32)).astype(np.int64), (a & np.uint64(R.MASK32), b & np.uint64(R.MASK32))


def attempts(holes, board, nb, live, weights, range_of, key, ident, nonce, samples):
    """The accepted attempts of a VALID spot: (hands uint8 [A, N, 7] = board + hole cards, live mask, the accepted attempt indices [A])."""
    holes = np.asarray(holes, np.uint8)
    n = holes.shape[0]
    w = as_ranges(weights)
    status, dead, live, hidden = check_spot(holes, board, nb, live, range_of, len(w))
    assert status == 0
    nb, hn = int(nb), len(hidden)
    cums = []
    for p in hidden:
        ro = UNIFORM if range_of is None else int(range_of[p])
        cums.append(np.arange(1, HOLDINGS + 1, dtype=np.uint32) if ro == UNIFORM else np.cumsum(w[ro].astype(np.uint32), dtype=np.uint32))
    x = words(key, ident, nonce, hn + 1, samples)
    if any(int(c[-1]) == 0 for c in cums):
        return np.zeros((0, n, 7), np.uint8), live, np.zeros(0, np.int64)
    hs = [np.searchsorted(c, mulhi(x[j], int(c[-1]))[0], side="right") for j, c in enumerate(cums)]     # the number of h with cum[h] <= u
    k = 5 - nb
    pool0 = [c for c in ES.CANON if c not in dead]
    cs, xb = [], x[hn]
    for i in range(k):
        c, xb = mulhi(xb, len(pool0) - 2 * hn - i)
        cs.append(c)
    hands, took = [], []
    for s in range(samples):
        gone, ok = set(dead), True
        cards = holes.copy()
        for j, p in enumerate(hidden):
            h = int(hs[j][s])
            pair = (ES.CANON[PAIR_A[h]], ES.CANON[PAIR_B[h]])
            if gone & set(pair):
                ok = False
                break
            gone |= set(pair)
            cards[p] = pair
        if not ok:
            continue
        pool = [c for c in ES.CANON if c not in gone]
        hand = np.zeros((n, 7), np.uint8)
        hand[:, :nb] = np.asarray(board[:nb], np.uint8)
        hand[:, 5:] = cards
        for i in range(k):
            hand[:, nb + i] = pool.pop(int(cs[i][s]))
        hands.append(hand)
        took.append(s)
    return (np.array(hands, np.uint8) if hands else np.zeros((0, n, 7), np.uint8)), live, np.array(took, np.int64)


def spot_equity(holes, board, nb, live, samples, weights=None, range_of=None, seed=DEFAULT_SEED, nonce=0, ident=0, key=None):
    """One spot -> dict(win [N], tie [N], share [N], accepted, status)."""
    holes = np.asarray(holes, np.uint8)
    n = holes.shape[0]
    zero = dict(win=np.zeros(n, np.uint32), tie=np.zeros(n, np.uint32), share=np.zeros(n, np.uint64), accepted=0)
    status = check_spot(holes, board, int(nb), live, range_of, len(as_ranges(weights)))[0]
    if status:
        return dict(zero, status=status)
    hands, lv, took = attempts(holes, board, int(nb), live, weights, range_of, key or R.seed_key(seed), ident, nonce, samples)
    if not len(took):
        return dict(zero, status=0)
    return dict(SS.count(hands, lv), accepted=len(took), status=0)


def batch_equity(holes, board, nboard, live, samples, weights=None, range_of=None, per_spot=False, seed=DEFAULT_SEED, nonce=0, ids=None, key=None):
    """The batch form: holes [m, N, 2], board [m, 5], nboard [m], live [m], range_of [N] (or [m, N] with per_spot), ids [m] or None (= i)."""
    holes = np.asarray(holes, np.uint8)
    m, n = holes.shape[:2]
    out = dict(win=np.zeros((m, n), np.uint32), tie=np.zeros((m, n), np.uint32), share=np.zeros((m, n), np.uint64),
               accepted=np.zeros(m, np.uint32), status=np.zeros(m, np.uint8))
    for i in range(m):
        ro = None if range_of is None else (np.asarray(range_of)[i] if per_spot else np.asarray(range_of))
        r = spot_equity(holes[i], [int(x) for x in board[i]], int(nboard[i]), int(live[i]), samples, weights, ro, seed, nonce,
                        i if ids is None else int(ids[i]), key)
        for k in out:
            out[k][i] = r[k]
    return out


def table_spots(deck, player_states, turn, active, observer):
    """The table form's spots: exactly equity_sampled_spec.table_spots for a seat or OBSERVER_ACTIVE."""
    assert observer != OBSERVER_NONE
    return SS.table_spots(deck, player_states, turn, active, observer)


def random_ranges(rng):
    """Four rows: dense random, about 40 holdings, a single holding, all zero."""
    w = np.zeros((4, HOLDINGS), np.uint16)
    w[0] = rng.integers(0, 1000, HOLDINGS)
    w[1, rng.choice(HOLDINGS, 40, replace=False)] = rng.integers(1, 65536, 40)
    w[2, int(rng.integers(HOLDINGS))] = 7
    return w


def random_spots(rng, n, m, nb=(0, 3, 4, 5)):
    """m valid random spots at n seats: all live seats hidden, one observer shown, nothing hidden, and a shown folded hand beside hidden seats."""
    holes, board, nboard, live = ES.random_spots(rng, n, m, unknown=False)
    for i in range(m):
        nboard[i] = nb[i % len(nb)]
        lv = [p for p in range(n) if (int(live[i]) >> p) & 1]
        kind = (i // len(nb)) % 4
        if kind == 0:
            holes[i] = ES.UNKNOWN                                     # (0xFF at a seat that is not live: in the pool)
        elif kind == 1:
            holes[i, lv[1:]] = ES.UNKNOWN
        elif kind == 3:
            if len(lv) > 1:
                live[i] = int(live[i]) & ~(1 << lv[-1])               # folds, its cards stay shown (dead)
                lv = lv[:-1]
            holes[i, lv] = ES.UNKNOWN
    return holes, board, nboard, live
