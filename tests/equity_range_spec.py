"""The range-equity definition restated in numpy (TEST INFRASTRUCTURE): include/pokerl_hip.h "Range equity" / DESIGN.md section 3.3 on top of
oracle.loader.eval_hands and equity_spec.winners_literal.  Every (holding, completion) pair is a row of its own: the villain's hand is
evaluated once PER PAIR, not once per seven-card set as the device does; the hero's word is evaluated once per completion and gathered."""
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


def holding_index(a, b):
    a, b = sorted((a, b))
    return b * (b - 1) // 2 + a


def canon_index(c):
    return (c & 15) * 4 + (c >> 4)


def check_spot(hero, board, nb, dead=0):
    """(status, set of dead canonical indices)."""
    status, seen = 0, []
    nb, dead = int(nb), int(dead)
    if nb > 5:
        status |= BAD_NBOARD
        cards = [int(x) for x in hero]
    else:
        if nb < 3:
            status |= PREFLOP
        cards = [int(x) for x in hero] + [int(x) for x in board[:nb]]
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
    if nb <= 5 and 52 - len(gone) < (5 - nb) + 2:
        status |= SMALL_POOL
    return status, gone


def spot_range(hero, board, nb, dead=0):
    """One spot -> dict(win [1326], tie [1326], valid [1326] bool, boards, status)."""
    zero = dict(win=np.zeros(HOLDINGS, np.uint32), tie=np.zeros(HOLDINGS, np.uint32), valid=np.zeros(HOLDINGS, bool), boards=0)
    status, gone = check_spot(hero, board, nb, dead)
    if status:
        return dict(zero, status=status)
    nb = int(nb)
    pool = [k for k in range(52) if k not in gone]                   # canonical indices, canonical order
    p, k = len(pool), 5 - nb
    pv = np.array([CANON[c] for c in pool], np.uint8)
    comps = np.array(list(itertools.combinations(range(p), k)), np.int64).reshape(math.comb(p, k), k)   # completions as pool slots
    hold = np.array(list(itertools.combinations(range(p), 2)), np.int64)                   # holdings as pool slots a < b
    clash = np.zeros((len(hold), len(comps)), bool)
    for j in range(k):
        clash |= (comps[None, :, j] == hold[:, 0, None]) | (comps[None, :, j] == hold[:, 1, None])
    hi, ci = np.nonzero(~clash)
    boards = math.comb(p - 2, k)
    assert len(hi) == boards * len(hold)
    hand = np.zeros((len(comps), 7), np.uint8)
    hand[:, :nb] = np.asarray(board[:nb], np.uint8)
    hand[:, nb:5] = pv[comps]
    hand[:, 5:] = np.asarray(hero, np.uint8)
    hr, hk, _ = O.eval_hands(hand)                                   # the hero: once per completion
    rows = np.zeros((len(hi), 7), np.uint8)
    rows[:, :5] = hand[ci, :5]
    rows[:, 5:] = pv[hold[hi]]
    vr, vk, _ = O.eval_hands(rows)                                   # the villain: once per (holding, completion)
    win = ES.winners_literal(np.stack([hr[ci], vr]), np.stack([hk[ci], vk]))
    ca, cb = np.array(pool)[hold[:, 0]], np.array(pool)[hold[:, 1]]   # canonical indices a < b (the pool is in canonical order)
    hidx = cb * (cb - 1) // 2 + ca
    out = dict(zero, boards=boards, status=0)
    out["win"] = np.bincount(hidx[hi], weights=(win == 1), minlength=HOLDINGS).astype(np.uint32)
    out["tie"] = np.bincount(hidx[hi], weights=(win == 3), minlength=HOLDINGS).astype(np.uint32)
    out["valid"] = np.zeros(HOLDINGS, bool)
    out["valid"][hidx] = True
    return out


def aggregate(r, weights=None):
    """agg [3] of one spot's result under `weights` ([1326] integers; None = ones), in Python integers."""
    w = np.ones(HOLDINGS, np.int64) if weights is None else np.asarray(weights, np.int64)
    return [int(np.sum(w * r["win"].astype(np.int64))), int(np.sum(w * r["tie"].astype(np.int64))), int(r["boards"]) * int(np.sum(w[r["valid"]]))]


def batch_range(hero, board, nboard, dead=None, weights=None):
    """The batch form -> dict of [m, 1326] / [m] / [m, 3] arrays (weights: None, [1326] or [m, 1326])."""
    hero = np.asarray(hero, np.uint8)
    m = hero.shape[0]
    out = dict(win=np.zeros((m, HOLDINGS), np.uint32), tie=np.zeros((m, HOLDINGS), np.uint32), valid=np.zeros((m, HOLDINGS), bool),
               boards=np.zeros(m, np.uint32), status=np.zeros(m, np.uint8), agg=np.zeros((m, 3), np.uint64))
    for i in range(m):
        r = spot_range(hero[i], [int(x) for x in board[i]], int(nboard[i]), 0 if dead is None else int(dead[i]))
        for key in ("win", "tie", "valid", "boards", "status"):
            out[key][i] = r[key]
        w = None if weights is None else (np.asarray(weights)[i] if np.ndim(weights) == 2 else weights)
        out["agg"][i] = aggregate(r, w)
    return out


def random_spots(rng, m, nb, pool=None):
    """m valid random spots with nb board cards; pool: None = full, an int P or a callable i -> P = the pool size a random `dead` mask leaves."""
    hero = np.zeros((m, 2), np.uint8)
    board = np.zeros((m, 5), np.uint8)
    dead = np.zeros(m, np.uint64)
    for i in range(m):
        deck = [int(x) for x in rng.permutation(52)]
        hero[i] = [CANON[c] for c in deck[:2]]
        board[i] = [CANON[c] for c in deck[2:7]]
        want = pool(i) if callable(pool) else pool
        if want is not None:
            rest = deck[2 + nb:]                                     # (the later streets' board bytes may be dead: they are not read)
            for c in rest[:len(rest) - want]:
                dead[i] |= np.uint64(1) << np.uint64(c)
    return hero, board, np.full(m, nb, np.uint8), dead


def table_spots(deck, turn, who):
    """The table form's spots from the getters: deck uint8 [m, 5 + 2N], turn [m], who [m] (the observer's seat) -> hero, board, nboard."""
    deck = np.asarray(deck, np.uint8)
    rows = np.arange(len(deck))
    who = np.asarray(who, np.int64)
    hero = np.stack([deck[rows, 5 + 2 * who], deck[rows, 6 + 2 * who]], axis=1)
    nboard = np.where(np.asarray(turn) == 0, 0, np.minimum(np.asarray(turn) + 2, 5)).astype(np.uint8)
    return hero, deck[:, :5].copy(), nboard
