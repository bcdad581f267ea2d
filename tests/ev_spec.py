"""The showdown-EV definition restated in numpy (TEST INFRASTRUCTURE): include/pokerl_hip.h "Showdown EV" / DESIGN.md section 3.7 on top of
tests/equity_spec.py (check_spot, winners_literal) and oracle.loader.eval_hands.  The levels by the literal loop of game.py:494-525 (stable
argsort, np.clip, np.sum), the winners of a level by the literal compare_rankings loop on the rankings with every seat outside the level's
remain set to (NONE, []), ev by the stated formula in binary64.  Nothing in it comes from a kernel."""
import itertools
import math

import numpy as np

import equity_spec as ES
from oracle import loader as O

SHARE_UNIT = ES.SHARE_UNIT
BAD_BET = 64
NO_LEVEL = 0xFF


def bad_bets(bets):
    b = np.asarray(bets, np.float64)
    return bool(np.any(~np.isfinite(b)) or np.any(b < 0))


def levels(bets, live):
    """[(seat, amount, remain mask, last)] in visiting order: bets float64 [N], live a seat mask."""
    bets = np.asarray(bets, np.float64)
    n = len(bets)
    order = [int(p) for p in np.argsort(bets, kind="stable") if (live >> int(p)) & 1]          # game.py:495-496
    work = bets.copy()
    remain = sum(1 << p for p in order)
    out = []
    for s in order:
        if np.all(work <= 0):                                                                  # :499
            break
        if bin(remain).count("1") == 1:                                                        # :500-505
            out.append((s, float(np.sum(work)), remain, True))
            break
        mb = np.clip(work, 0, work[s])                                                         # :508-509
        out.append((s, float(np.sum(mb)), remain, False))
        remain &= ~(1 << s)                                                                    # :522
        work = work - mb                                                                       # :523
    assert len(out) <= n
    return out


def spot_rankings(holes, board, nb, live, dead):
    """rank uint8 [N, B], kick uint32 [N, B] over the spot's boards in the definition's order (a seat that is not live: (NONE, []))."""
    n = holes.shape[0]
    pool = [c for c in ES.CANON if c not in dead]
    k = 5 - int(nb)
    b = math.comb(len(pool), k)
    combos = np.fromiter(itertools.chain.from_iterable(itertools.combinations(pool, k)), np.uint8, count=b * k).reshape(b, k)
    rank = np.full((n, b), ES.NONE_RANK, np.uint8)
    kick = np.zeros((n, b), np.uint32)
    hand = np.zeros((b, 7), np.uint8)
    hand[:, :int(nb)] = np.asarray(board[:int(nb)], np.uint8)
    hand[:, int(nb):5] = combos
    for p in range(n):
        if (live >> p) & 1:
            hand[:, 5:] = holes[p]
            rank[p], kick[p], _ = O.eval_hands(hand)
    return rank, kick


def level_winners(rank, kick, remain):
    """W_i per board (bit masks uint32 [B]): the literal loop on the rankings masked by `remain`."""
    r, k = rank.copy(), kick.copy()
    for p in range(rank.shape[0]):
        if not (remain >> p) & 1:
            r[p] = ES.NONE_RANK
            k[p] = 0
    return ES.winners_literal(r, k)


def ev_formula(amount, share, boards, bets):
    """acc = +0.0; for i ascending: acc = acc + (amount[i] * float(share[i][p])) / (720720.0 * float(boards)); ev[p] = acc - bets[p]."""
    n = len(bets)
    ev = np.zeros(n, np.float64)
    den = np.float64(720720.0) * np.float64(boards)
    for p in range(n):
        acc = np.float64(0.0)
        for i in range(n):
            acc = acc + (np.float64(amount[i]) * np.float64(int(share[i][p]))) / den
        ev[p] = acc - np.float64(bets[p])
    return ev


def spot_ev(holes, board, nb, live, bets):
    """One spot -> dict(share [N, N], level_seat [N], amount [N], ev [N], boards, status)."""
    holes = np.asarray(holes, np.uint8)
    n = holes.shape[0]
    bets = np.asarray(bets, np.float64)
    zero = dict(share=np.zeros((n, n), np.uint64), level_seat=np.full(n, NO_LEVEL, np.uint8), amount=np.zeros(n, np.float64),
                ev=np.zeros(n, np.float64), boards=0)
    status, dead, live = ES.check_spot(holes, board, int(nb), live)
    if bad_bets(bets):
        status |= BAD_BET
    if status:
        return dict(zero, status=status)
    lv = levels(bets, live)
    out = dict(zero, status=0)
    b = math.comb(52 - len(dead), 5 - int(nb))
    out["boards"] = b
    rank = kick = None
    for i, (s, amount, remain, last) in enumerate(lv):
        out["level_seat"][i] = s
        out["amount"][i] = amount
        if last:
            out["share"][i][s] = SHARE_UNIT * b
        elif amount > 0:
            if rank is None:
                rank, kick = spot_rankings(holes, board, nb, live, dead)
            win = level_winners(rank, kick, remain)
            nw = np.zeros(b, np.int64)
            for p in range(n):
                nw += (win >> np.uint32(p)) & 1
            for p in range(n):
                inw = ((win >> np.uint32(p)) & 1).astype(bool)
                out["share"][i][p] = int(np.sum(SHARE_UNIT // nw[inw]))
    out["ev"] = ev_formula(out["amount"], out["share"], b, bets)
    return out


def batch_ev(holes, board, nboard, live, bets):
    """The batch form: holes [m, N, 2], board [m, 5], nboard [m], live [m], bets [m, N] -> dict of [m, N, N] / [m, N] / [m] arrays."""
    holes = np.asarray(holes, np.uint8)
    m, n = holes.shape[:2]
    out = dict(share=np.zeros((m, n, n), np.uint64), level_seat=np.zeros((m, n), np.uint8), amount=np.zeros((m, n), np.float64),
               ev=np.zeros((m, n), np.float64), boards=np.zeros(m, np.uint32), status=np.zeros(m, np.uint8))
    for i in range(m):
        r = spot_ev(holes[i], [int(x) for x in board[i]], int(nboard[i]), int(live[i]), bets[i])
        for key in out:
            out[key][i] = r[key]
    return out


def check_against_reference(got_ev, s, what):
    """Complete boards: bit for bit.  The others: within 4 (L + 2) 2^-53 np.sum(bets), L the number of levels -- the roundings of the formula
    (two per term, L accumulations, one subtraction) plus those of the reference's per-board arithmetic (one division per level, L
    accumulations, one subtraction), each relative to at most the pot: (2 L + 5) u pot in all."""
    if "payoffs" in s:
        want = np.array([float.fromhex(x) for x in s["payoffs"]], np.float64)
        assert np.array_equal(np.asarray(got_ev, np.float64).view(np.uint64), want.view(np.uint64)), (what, got_ev, want)
    else:
        want = np.array([float.fromhex(x) for x in s["mean"]], np.float64)
        nlev = len(levels(np.array(s["bets"], np.float64), s["live"]))
        bound = 4 * (nlev + 2) * 2.0 ** -53 * float(np.sum(np.array(s["bets"], np.float64)))
        err = np.abs(np.asarray(got_ev, np.float64) - want)
        assert np.all(err <= bound), (what, err.max(), bound)


def assert_same(got, want, what=""):
    """Every output against the spec: integers equal, floating point bit for bit."""
    for key in ("status", "boards", "level_seat", "share"):
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape and np.array_equal(g.astype(np.uint64), w.astype(np.uint64)), (what, key, g, w)
    for key in ("amount", "ev"):
        g, w = np.ascontiguousarray(got[key], np.float64), np.ascontiguousarray(want[key], np.float64)
        assert g.shape == w.shape and np.array_equal(g.view(np.uint64), w.view(np.uint64)), (what, key, g, w)
