"""The showdown-equity definition restated in numpy (TEST INFRASTRUCTURE): include/pokerl_hip.h "Showdown equity" / DESIGN.md section 3.1 on
top of oracle.loader.eval_hands.  Boards by itertools.combinations, the winners by the LITERAL compare_rankings loop (judger.py:111-158,
line 148 included) vectorised over boards -- not the device's closed form."""
import itertools
import math

import numpy as np

from oracle import loader as O

SHARE_UNIT = 720720
BAD_CARD, DUP_CARD, NO_LIVE, BAD_NBOARD, IN_FLIGHT, BAD_TABLE = 1, 2, 4, 8, 16, 32
UNKNOWN = 0xFF
NONE_RANK = 10
CANON = [((c % 4) << 4) | (c // 4) for c in range(52)]          # cards.py:77


def _is_card(c):
    return c < 0x40 and (c & 15) < 13


def check_spot(holes, board, nb, live):
    """(status, dead set, live mask restricted to the N seats)."""
    holes = np.asarray(holes, np.uint8)
    n = holes.shape[0]
    live = int(live) & ((1 << n) - 1)
    status = 0
    if nb > 5:
        return BAD_NBOARD | (0 if live else NO_LIVE) | _hole_status(holes, live), set(), live
    seen = []
    for c in [int(x) for x in board[:nb]]:
        if not _is_card(c):
            status |= BAD_CARD
        else:
            seen.append(c)
    for p in range(n):
        for c in [int(x) for x in holes[p]]:
            if c == UNKNOWN:
                if (live >> p) & 1:
                    status |= BAD_CARD
            elif not _is_card(c):
                status |= BAD_CARD
            else:
                seen.append(c)
    if len(set(seen)) != len(seen):
        status |= DUP_CARD
    if not live:
        status |= NO_LIVE
    return status, set(seen), live


def _hole_status(holes, live):
    """Status bits of the hole cards alone (a spot with nb > 5: its board is not read)."""
    status, seen = 0, []
    for p in range(holes.shape[0]):
        for c in [int(x) for x in holes[p]]:
            if c == UNKNOWN:
                if (live >> p) & 1:
                    status |= BAD_CARD
            elif not _is_card(c):
                status |= BAD_CARD
            else:
                seen.append(c)
    if len(set(seen)) != len(seen):
        status |= DUP_CARD
    return status


def winners_literal(rank, kick, fixed148=False):
    """rank uint8 [N, B], kick uint32 [N, B] -> winners bit mask uint32 [B]: the loop of judger.py:134-155, every board at once.
    fixed148: what the loop would do if line 148 raised best_kicker (only to show that a fixture depends on the line as it is)."""
    n, b = rank.shape
    best_rank = np.full(b, NONE_RANK, np.int64)
    best_kick = np.zeros(b, np.int64)
    win = np.zeros(b, np.uint32)
    for p in range(n):
        r, k = rank[p].astype(np.int64), kick[p].astype(np.int64)
        lt = r < best_rank
        eq = r == best_rank
        gt = eq & (k > best_kick)
        same = eq & (k == best_kick)
        win = np.where(lt | gt, np.uint32(1 << p), np.where(same, win | np.uint32(1 << p), win)).astype(np.uint32)
        best_kick = np.where(lt, k, best_kick)
        if fixed148:
            best_kick = np.where(gt, k, best_kick)
        best_rank = np.where(lt, r, best_rank)
    return win


def spot_equity(holes, board, nb, live, fixed148=False):
    """One spot -> dict(win [N], tie [N], share [N], boards, status)."""
    holes = np.asarray(holes, np.uint8)
    n = holes.shape[0]
    zero = dict(win=np.zeros(n, np.uint32), tie=np.zeros(n, np.uint32), share=np.zeros(n, np.uint64), boards=0)
    status, dead, live = check_spot(holes, board, int(nb), live)
    if status:
        return dict(zero, status=status)
    pool = [c for c in CANON if c not in dead]
    k = 5 - int(nb)
    b = math.comb(len(pool), k)
    combos = np.fromiter(itertools.chain.from_iterable(itertools.combinations(pool, k)), np.uint8, count=b * k).reshape(b, k)
    rank = np.full((n, b), NONE_RANK, np.uint8)               # eval_hand([]) = (NONE, []) for a seat that does not show down
    kick = np.zeros((n, b), np.uint32)
    hand = np.zeros((b, 7), np.uint8)
    hand[:, :int(nb)] = np.asarray(board[:int(nb)], np.uint8)
    hand[:, int(nb):5] = combos
    for p in range(n):
        if (live >> p) & 1:
            hand[:, 5:] = holes[p]
            rank[p], kick[p], _ = O.eval_hands(hand)
    win = winners_literal(rank, kick, fixed148)
    nw = np.zeros(b, np.int64)
    for p in range(n):
        nw += (win >> np.uint32(p)) & 1
    out = dict(zero, boards=b, status=0)
    for p in range(n):
        inw = ((win >> np.uint32(p)) & 1).astype(bool)
        out["win"][p] = int(np.sum(inw & (nw == 1)))
        out["tie"][p] = int(np.sum(inw & (nw > 1)))
        out["share"][p] = int(np.sum(SHARE_UNIT // nw[inw]))
    return out


def batch_equity(holes, board, nboard, live):
    """The batch form: holes [m, N, 2], board [m, 5], nboard [m], live [m] -> dict of [m, N] / [m] arrays."""
    holes = np.asarray(holes, np.uint8)
    m, n = holes.shape[:2]
    out = dict(win=np.zeros((m, n), np.uint32), tie=np.zeros((m, n), np.uint32), share=np.zeros((m, n), np.uint64),
               boards=np.zeros(m, np.uint32), status=np.zeros(m, np.uint8))
    for i in range(m):
        r = spot_equity(holes[i], [int(x) for x in board[i]], int(nboard[i]), int(live[i]))
        for key in out:
            out[key][i] = r[key]
    return out


def table_spots(deck, player_states, turn):
    """The table form's spots from the getters: deck uint8 [T, 5 + 2N], player_states [T, N] (PlayerState), turn [T]."""
    deck = np.asarray(deck, np.uint8)
    t, n = player_states.shape
    holes = deck[:, 5:5 + 2 * n].reshape(t, n, 2)
    nboard = np.where(np.asarray(turn) == 0, 0, np.minimum(np.asarray(turn) + 2, 5)).astype(np.uint8)
    ps = np.asarray(player_states)
    livebits = (ps == 1) | (ps == 2) | (ps == 3)                 # ACTIVE, CALLED, ALL_IN (enums.py)
    live = (livebits.astype(np.uint16) << np.arange(n, dtype=np.uint16)).sum(axis=1).astype(np.uint16)
    return holes, deck[:, :5].copy(), nboard, live


def random_spots(rng, n, m, nb=None, unknown=True):
    """m valid random spots at n seats: random live masks (at least one seat), some non-live seats unknown."""
    holes = np.zeros((m, n, 2), np.uint8)
    board = np.zeros((m, 5), np.uint8)
    nboard = np.zeros(m, np.uint8)
    live = np.zeros(m, np.uint16)
    for i in range(m):
        deck = rng.permutation(52)
        vals = np.array([CANON[c] for c in deck], np.uint8)
        board[i] = vals[:5]
        holes[i] = vals[5:5 + 2 * n].reshape(n, 2)
        nboard[i] = rng.integers(0, 6) if nb is None else nb
        mask = int(rng.integers(1, 1 << n))
        live[i] = mask
        if unknown:
            for p in range(n):
                if not (mask >> p) & 1 and rng.integers(0, 2):
                    holes[i, p] = UNKNOWN
    return holes, board, nboard, live
