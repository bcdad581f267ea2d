"""The sampled-showdown-equity definition restated in Python (TEST INFRASTRUCTURE): include/pokerl_hip.h "Sampled showdown equity" /
DESIGN.md section 3.2 on top of oracle.rng_spec.philox4x32_10 (over all sample indices at once: its arithmetic is the same on uint64
arrays), oracle.loader.eval_hands and equity_spec's check_spot / winners_literal.  The draw is the LITERAL `pool.pop(c)` per sample and
slot -- not the device's bit select."""
import numpy as np

import equity_spec as ES
from oracle import loader as O
from oracle import rng_spec as R

STREAM_EQS = 0x45515330          # 'EQS0'
SAMPLES_MAX = 1 << 24
DEFAULT_SEED = R.DEFAULT_SEED
OBSERVER_NONE, OBSERVER_ACTIVE = -1, -2
KEYS = ("win", "tie", "share", "samples", "status")


def check_spot(holes, board, nb, live):
    """(status, dead set, live mask, hidden slots [(seat, byte)]): equity_spec.check_spot, except that a 0xFF hole byte at a live seat is
    legal.  The seats that hold one are taken out of the live mask for equity_spec's check, which then sees their 0xFF as "not known"."""
    holes = np.asarray(holes, np.uint8)
    n = holes.shape[0]
    live = int(live) & ((1 << n) - 1)
    hidden = [(p, b) for p in range(n) for b in range(2) if (live >> p) & 1 and int(holes[p, b]) == ES.UNKNOWN]
    shown = live
    for p, _ in hidden:
        shown &= ~(1 << p)
    status, dead, _ = ES.check_spot(holes, board, int(nb), shown)
    status &= ~ES.NO_LIVE
    if not live:
        status |= ES.NO_LIVE
    return status, dead, live, hidden


def draws(key, ident, nonce, pool_size, ndraws, samples):
    """c [samples, ndraws]: the chained bounded draws c_i in [0, P - i) of every sample s of stream `ident`."""
    s = np.arange(samples, dtype=np.uint64)
    same = np.zeros(samples, np.uint64)
    c = np.zeros((samples, ndraws), np.int64)
    x = []
    xlo = xhi = None
    for i in range(ndraws):
        if i % 18 == 0:
            w = R.philox4x32_10((same + np.uint64(ident & R.MASK32), s, same + np.uint64((STREAM_EQS + i // 18) & R.MASK32),
                                 same + np.uint64(nonce & R.MASK32)), key)
            x = [(w[0], w[1]), (w[2], w[3])]                   # X[2b] = w0 | w1 << 32, X[2b + 1] = w2 | w3 << 32, as (low, high) halves
        if i % 9 == 0:
            xlo, xhi = x[(i // 9) % 2]
        left = np.uint64(pool_size - i)                        # (x * left) >> 64 and x * left mod 2^64 from 32-bit halves: every product < 2^64
        a = xlo * left
        b = xhi * left + (a >> np.uint64(32))
        c[:, i] = (b >> np.uint64(32)).astype(np.int64)
        xlo, xhi = a & np.uint64(R.MASK32), b & np.uint64(R.MASK32)
    return c


def sample_cards(holes, board, nb, live, key, ident, nonce, samples):
    """The S dealt-out samples of a VALID spot: (hands uint8 [S, N, 7] = board + hole cards, live mask)."""
    holes = np.asarray(holes, np.uint8)
    n = holes.shape[0]
    status, dead, live, hidden = check_spot(holes, board, nb, live)
    assert status == 0
    pool0 = [c for c in ES.CANON if c not in dead]
    k = 5 - int(nb)
    c = draws(key, ident, nonce, len(pool0), k + len(hidden), samples)
    hands = np.zeros((samples, n, 7), np.uint8)
    hands[:, :, :int(nb)] = np.asarray(board[:int(nb)], np.uint8)
    hands[:, :, 5:] = holes
    for s in range(samples):
        pool = list(pool0)
        for j in range(k):
            hands[s, :, int(nb) + j] = pool.pop(int(c[s, j]))
        for j, (p, b) in enumerate(hidden):
            hands[s, p, 5 + b] = pool.pop(int(c[s, k + j]))
    return hands, live


def count(hands, live, first=0, last=None):
    """win / tie / share [N] over samples first .. last - 1 of sample_cards' hands."""
    hands = hands[first:last]
    s, n = hands.shape[:2]
    rank = np.full((n, s), ES.NONE_RANK, np.uint8)
    kick = np.zeros((n, s), np.uint32)
    for p in range(n):
        if (live >> p) & 1:
            rank[p], kick[p], _ = O.eval_hands(np.ascontiguousarray(hands[:, p]))
    win = ES.winners_literal(rank, kick)
    nw = np.zeros(s, np.int64)
    for p in range(n):
        nw += (win >> np.uint32(p)) & 1
    out = dict(win=np.zeros(n, np.uint32), tie=np.zeros(n, np.uint32), share=np.zeros(n, np.uint64))
    for p in range(n):
        inw = ((win >> np.uint32(p)) & 1).astype(bool)
        out["win"][p] = int(np.sum(inw & (nw == 1)))
        out["tie"][p] = int(np.sum(inw & (nw > 1)))
        out["share"][p] = int(np.sum(ES.SHARE_UNIT // nw[inw]))
    return out


def spot_equity(holes, board, nb, live, samples, seed=DEFAULT_SEED, nonce=0, ident=0, key=None):
    """One spot -> dict(win [N], tie [N], share [N], samples, status)."""
    holes = np.asarray(holes, np.uint8)
    n = holes.shape[0]
    status = check_spot(holes, board, int(nb), live)[0]
    if status:
        return dict(win=np.zeros(n, np.uint32), tie=np.zeros(n, np.uint32), share=np.zeros(n, np.uint64), samples=0, status=status)
    hands, lv = sample_cards(holes, board, int(nb), live, key or R.seed_key(seed), ident, nonce, samples)
    return dict(count(hands, lv), samples=samples, status=0)


def batch_equity(holes, board, nboard, live, samples, seed=DEFAULT_SEED, nonce=0, ids=None, key=None):
    """The batch form: holes [m, N, 2], board [m, 5], nboard [m], live [m], ids [m] or None (= i) -> dict of [m, N] / [m] arrays."""
    holes = np.asarray(holes, np.uint8)
    m, n = holes.shape[:2]
    out = dict(win=np.zeros((m, n), np.uint32), tie=np.zeros((m, n), np.uint32), share=np.zeros((m, n), np.uint64),
               samples=np.zeros(m, np.uint32), status=np.zeros(m, np.uint8))
    for i in range(m):
        r = spot_equity(holes[i], [int(x) for x in board[i]], int(nboard[i]), int(live[i]), samples, seed, nonce,
                        i if ids is None else int(ids[i]), key)
        for k in out:
            out[k][i] = r[k]
    return out


def table_spots(deck, player_states, turn, active, observer):
    """The table form's spots from the getters, as `observer` (a seat, OBSERVER_ACTIVE or OBSERVER_NONE) sees them: deck uint8
    [T, 5 + 2N], player_states [T, N], turn [T], active [T].  The observer's own hole cards stay; every other seat's become 0xFF (hidden
    if the seat is live, not known -- in the pool -- if it is not)."""
    holes, board, nboard, live = ES.table_spots(deck, player_states, turn)
    if observer == OBSERVER_NONE:
        return holes, board, nboard, live
    t, n = player_states.shape
    who = np.asarray(active, np.int64) if observer == OBSERVER_ACTIVE else np.full(t, int(observer), np.int64)
    seen = holes.copy()
    holes = np.full_like(seen, ES.UNKNOWN)
    rows = np.arange(t)
    holes[rows, who] = seen[rows, who]
    return holes, board, nboard, live


def random_spots(rng, n, m, nb=None):
    """m valid random spots at n seats with random hidden masks: among them nothing hidden, everything hidden and a single hidden byte."""
    holes, board, nboard, live = ES.random_spots(rng, n, m, nb=nb)
    for i in range(m):
        lv = [p for p in range(n) if (int(live[i]) >> p) & 1]
        kind = i % 4
        if kind == 1:
            holes[i, lv] = ES.UNKNOWN
        elif kind == 2:
            holes[i, lv[int(rng.integers(len(lv)))], int(rng.integers(2))] = ES.UNKNOWN
        elif kind == 3:
            mask = rng.integers(0, 2, (len(lv), 2)).astype(bool)
            sub = holes[i, lv]
            sub[mask] = ES.UNKNOWN
            holes[i, lv] = sub
    return holes, board, nboard, live
