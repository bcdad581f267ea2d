"""The range-vs-range definition restated in numpy (TEST INFRASTRUCTURE): include/pokerl_hip.h "Range vs range" / DESIGN.md section 3.4 on top
of oracle.loader.eval_hands and equity_spec.winners_literal.  Per completion of the board every holding is evaluated once; every ORDERED
disjoint (hero, villain) pair is then decided by winners_literal as a row of its own.  There is no sort and no comparison of ranking words
here: the ordering is exactly what the device result is tested against.  One completion at a time, so memory stays small."""
import itertools
import math

import numpy as np

import equity_spec as ES
from oracle import loader as O

HOLDINGS = 1326
BAD_CARD, DUP_CARD, BAD_NBOARD, IN_FLIGHT, BAD_TABLE, PREFLOP, SMALL_POOL = 1, 2, 8, 16, 32, 64, 128
CANON = ES.CANON
PAIR_A = np.array([a for b in range(52) for a in range(b)])          # holding h = b (b - 1) / 2 + a, canonical indices a < b
PAIR_B = np.array([b for b in range(52) for a in range(b)])


def canon_index(c):
    return (c & 15) * 4 + (c >> 4)


def check_spot(board, nb, dead=0):
    """(status, set of dead canonical indices).  There is no hero."""
    status, seen = 0, []
    nb, dead = int(nb), int(dead)
    if nb > 5:
        status |= BAD_NBOARD
        cards = []
    else:
        if nb < 3:
            status |= PREFLOP
        cards = [int(x) for x in board[:nb]]
    for c in cards:
        if not ES._is_card(c):
            status |= BAD_CARD
        else:
            seen.append(canon_index(c))
    if len(set(seen)) != len(seen):
        status |= DUP_CARD
    if dead >> 52:
        status |= BAD_CARD
    out = {k for k in range(52) if (dead >> k) & 1}
    if out & set(seen):
        status |= DUP_CARD
    gone = out | set(seen)
    if nb <= 5 and 52 - len(gone) < (5 - nb) + 4:                    # the board to come and TWO holdings
        status |= SMALL_POOL
    return status, gone


def spot_rvr(board, nb, dead=0, weights=None):
    """One spot -> dict(win, tie, tot uint64 [1326], valid [1326] bool, boards, status).  weights: None (ones), [1326] integers, or
    [r, 1326] -- r ranges at once over the same pairwise decisions: win / tie / tot are then [r, 1326]."""
    many = weights is not None and np.ndim(weights) == 2
    w = np.ones((1, HOLDINGS), np.int64) if weights is None else np.atleast_2d(np.asarray(weights, np.int64))
    r = w.shape[0]
    shape = (r, HOLDINGS) if many else (HOLDINGS,)
    zero = dict(win=np.zeros(shape, np.uint64), tie=np.zeros(shape, np.uint64), tot=np.zeros(shape, np.uint64), valid=np.zeros(HOLDINGS, bool), boards=0)
    status, gone = check_spot(board, nb, dead)
    if status:
        return dict(zero, status=status)
    nb = int(nb)
    pool = np.array([k for k in range(52) if k not in gone])         # canonical indices, canonical order
    p, k = len(pool), 5 - nb
    pv = np.array([CANON[c] for c in pool], np.uint8)
    boards = math.comb(p - 4, k)
    win, tie = np.zeros((r, HOLDINGS), np.int64), np.zeros((r, HOLDINGS), np.int64)
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
        win[:, hidx] += wl @ alone.T
        tie[:, hidx] += wl @ both.T
    hold = np.array(list(itertools.combinations(range(p), 2)), np.int64)
    hidx = pool[hold[:, 1]] * (pool[hold[:, 1]] - 1) // 2 + pool[hold[:, 0]]
    share = (hold[:, None, 0] == hold[None, :, 0]) | (hold[:, None, 0] == hold[None, :, 1]) | \
            (hold[:, None, 1] == hold[None, :, 0]) | (hold[:, None, 1] == hold[None, :, 1])
    tot = np.zeros((r, HOLDINGS), np.int64)
    tot[:, hidx] = boards * (w[:, hidx] @ (~share).astype(np.int64).T)
    valid = np.zeros(HOLDINGS, bool)
    valid[hidx] = True
    out = dict(win=win.astype(np.uint64), tie=tie.astype(np.uint64), tot=tot.astype(np.uint64))
    if not many:
        out = {key: v[0] for key, v in out.items()}
    return dict(out, valid=valid, boards=boards, status=0)


def batch_rvr(board, nboard, dead=None, weights=None):
    """The batch form -> dict of [m, 1326] / [m] arrays (weights: None, [1326] or [m, 1326])."""
    board = np.asarray(board, np.uint8)
    m = board.shape[0]
    out = dict(win=np.zeros((m, HOLDINGS), np.uint64), tie=np.zeros((m, HOLDINGS), np.uint64), tot=np.zeros((m, HOLDINGS), np.uint64),
               valid=np.zeros((m, HOLDINGS), bool), boards=np.zeros(m, np.uint32), status=np.zeros(m, np.uint8))
    for i in range(m):
        w = None if weights is None else (np.asarray(weights)[i] if np.ndim(weights) == 2 else weights)
        r = spot_rvr([int(x) for x in board[i]], int(nboard[i]), 0 if dead is None else int(dead[i]), w)
        for key in out:
            out[key][i] = r[key]
    return out


def random_boards(rng, m, nb, pool=None):
    """m valid random spots with nb board cards; pool: None = full, an int P or a callable i -> P = the pool size a random `dead` mask leaves."""
    board = np.zeros((m, 5), np.uint8)
    dead = np.zeros(m, np.uint64)
    for i in range(m):
        deck = [int(x) for x in rng.permutation(52)]
        board[i] = [CANON[c] for c in deck[:5]]
        want = pool(i) if callable(pool) else pool
        if want is not None:
            rest = deck[nb:]                                         # (the later streets' board bytes may be dead: they are not read)
            for c in rest[:len(rest) - want]:
                dead[i] |= np.uint64(1) << np.uint64(c)
    return board, np.full(m, nb, np.uint8), dead


def table_boards(deck, turn):
    """The table form's spots from the getters: deck uint8 [m, 5 + 2N], turn [m] -> board, nboard."""
    deck = np.asarray(deck, np.uint8)
    nboard = np.where(np.asarray(turn) == 0, 0, np.minimum(np.asarray(turn) + 2, 5)).astype(np.uint8)
    return deck[:, :5].copy(), nboard
