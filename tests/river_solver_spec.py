"""The river-solver definition restated in numpy int64 (TEST INFRASTRUCTURE): include/pokerl_hip.h "River solver" / DESIGN.md section 3.12.
The pairwise beats / ties matrices come from equity_spec.winners_literal on oracle.loader.eval_hands, one row per ORDERED disjoint pair of
holdings, exactly as rvr_spec.py builds them: there is no sort and no comparison of ranking words here.  Every sum is an integer sum, so no
result depends on its order.  float_exploitability, at the end, is a SEPARATE float64 best response written from the payoff of a showdown
and a fold; it shares no code with the integer passes."""
import itertools

import numpy as np

import equity_spec as ES
import rvr_spec as VS
from oracle import loader as O

HOLDINGS = 1326
ONE = 32768
P0, P1, FOLD0, FOLD1, SHOWDOWN = 0, 1, 2, 3, 4
NONE = 0xFF
BAD_CARD, DUP_CARD, SMALL_POOL = VS.BAD_CARD, VS.DUP_CARD, VS.SMALL_POOL


class Tree:
    """kind uint8 [n], child uint8 [n, 4], put uint32 [n, 2], pot: the arrays of pokerl_amd.RiverTree (anything with these attributes)."""

    def __init__(self, kind, child, put, pot):
        self.kind = [int(k) for k in kind]
        self.child = [[int(c) for c in row if int(c) != NONE] for row in np.asarray(child).reshape(-1, 4)]
        self.put = [[int(x) for x in row] for row in np.asarray(put).reshape(-1, 2)]
        self.pot, self.n = int(pot), len(self.kind)
        self.decisions = [i for i in range(self.n) if self.kind[i] <= 1]


def as_tree(t):
    return t if isinstance(t, Tree) else Tree(t.kind, t.child, t.put, t.pot)


def check_spot(board, dead=0):
    status, gone = VS.check_spot(board, 5, dead)
    return status & ~VS.PREFLOP, gone


def pairwise(board, gone):
    """The pool's holdings (fixed indices, in pool order) and three int64 [n, n] matrices over ordered pairs (h, h'): h beats h', ties it,
    loses to it; all zero where the two share a card."""
    pool = np.array([k for k in range(52) if k not in gone])
    p = len(pool)
    pv = np.array([VS.CANON[c] for c in pool], np.uint8)
    hold = np.array(list(itertools.combinations(range(p), 2)), np.int64)
    n = len(hold)
    hand = np.zeros((n, 7), np.uint8)
    hand[:, :5] = np.asarray(board[:5], np.uint8)
    hand[:, 5:] = pv[hold]
    hr, hk, _ = O.eval_hands(hand)
    hidx = pool[hold[:, 1]] * (pool[hold[:, 1]] - 1) // 2 + pool[hold[:, 0]]
    share = (hold[:, None, 0] == hold[None, :, 0]) | (hold[:, None, 0] == hold[None, :, 1]) | \
            (hold[:, None, 1] == hold[None, :, 0]) | (hold[:, None, 1] == hold[None, :, 1])
    hi, vi = np.nonzero(~share)
    res = ES.winners_literal(np.stack([hr[hi], hr[vi]]), np.stack([hk[hi], hk[vi]]))
    beats, ties, loses = (np.zeros((n, n), np.int64) for _ in range(3))
    beats[hi, vi] = res == 1
    ties[hi, vi] = res == 3
    loses[hi, vi] = res == 2
    return hidx, beats, ties, loses


def bitlen(x):
    """bit length of non-negative int64, element-wise"""
    out, t = np.zeros(x.shape, np.int64), x.copy()
    for s in (32, 16, 8, 4, 2, 1):
        big = (t >> s) > 0
        out += big * s
        t = np.where(big, t >> s, t)
    return out + (t > 0)


def strategy_from(X):
    """X int64 [nact, n] >= 0 -> sigma int64 [nact, n], every column summing to ONE."""
    nact = X.shape[0]
    mx = X.max(axis=0)
    sh = np.maximum(0, bitlen(mx) - 31)
    Xp = X >> sh
    S = Xp.sum(axis=0)
    sig = np.zeros_like(X)
    for a in range(1, nact):
        sig[a] = np.where(mx == 0, ONE // nact, (Xp[a] << 15) // np.where(S == 0, 1, S))
    sig[0] = ONE - sig[1:].sum(axis=0)
    return sig


def tree_pass(T, M, root, sigma, best=None):
    """One tree pass.  M = (beats, ties, loses); root = (r_0, r_1) int64 [n]; sigma[node] int64 [nact, n].  best = p: the best-response
    pass of player p (p's reach copied at p's nodes, the maximum on the way up; only u[p] of the result means anything).
    -> (r, u): r[p][node], u[p][node] int64 [n]."""
    beats, ties, loses = M
    disjoint = beats + ties + loses
    r = [{0: root[0]}, {0: root[1]}]
    u = [{}, {}]
    for n in range(T.n):
        k = T.kind[n]
        if k <= 1:
            for a, c in enumerate(T.child[n]):
                r[k][c] = r[k][n] if best == k else (r[k][n] * sigma[n][a]) >> 15
                r[1 - k][c] = r[1 - k][n]
        elif k == SHOWDOWN:
            c = T.put[n][0]
            for p in (0, 1):
                rq = r[1 - p][n]
                u[p][n] = 2 * (T.pot + c) * (beats @ rq) + T.pot * (ties @ rq) - 2 * c * (loses @ rq)
        else:
            f = k - FOLD0
            for p in (0, 1):
                S = disjoint @ r[1 - p][n]
                u[p][n] = -2 * T.put[n][f] * S if p == f else 2 * (T.pot + T.put[n][f]) * S
    for n in reversed(range(T.n)):
        k = T.kind[n]
        if k > 1:
            continue
        ch = T.child[n]
        if best == k:
            u[k][n] = np.max(np.stack([u[k][c] for c in ch]), axis=0)
        else:
            u[k][n] = sum(sigma[n][a] * u[k][c] for a, c in enumerate(ch)) // ONE      # the sum first, the floor once
        u[1 - k][n] = sum(u[1 - k][c] for c in ch)
    return r, u


def solve_spot(board, ranges, tree, iters, dead=0):
    """One spot -> dict(strategy uint16 [D, 4, 1326], value, br int64 [2, 1326], status, valid bool [1326], regret_bits)."""
    T = as_tree(tree)
    D = len(T.decisions)
    out = dict(strategy=np.zeros((D, 4, HOLDINGS), np.uint16), value=np.zeros((2, HOLDINGS), np.int64), br=np.zeros((2, HOLDINGS), np.int64),
               valid=np.zeros(HOLDINGS, bool), regret_bits=0)
    status, gone = check_spot(board, dead)
    if 52 - len(gone) < 4:
        status |= SMALL_POOL
    out["status"] = status
    if status:
        return out
    hidx, beats, ties, loses = pairwise(board, gone)
    M = (beats, ties, loses)
    w = np.asarray(ranges, np.int64).reshape(2, HOLDINGS)[:, hidx]
    root = (w[0] << 4, w[1] << 4)
    n = len(hidx)
    R = {d: np.zeros((len(T.child[d]), n), np.int64) for d in T.decisions}
    A = {d: np.zeros((len(T.child[d]), n), np.int64) for d in T.decisions}
    for t in range(1, int(iters) + 1):
        sigma = {d: strategy_from(R[d]) for d in T.decisions}
        r, u = tree_pass(T, M, root, sigma)
        for d in T.decisions:
            p = T.kind[d]
            for a, c in enumerate(T.child[d]):
                R[d][a] = np.maximum(0, R[d][a] + u[p][c] - u[p][d])
                A[d][a] += t * r[p][c]
            out["regret_bits"] = max(out["regret_bits"], int(R[d].max()).bit_length())
    sigma = {d: strategy_from(A[d]) for d in T.decisions}
    for row, d in enumerate(T.decisions):
        out["strategy"][row, :len(T.child[d]), hidx] = sigma[d].T
    _, u = tree_pass(T, M, root, sigma)
    for p in (0, 1):
        out["value"][p, hidx] = u[p][0]
        out["br"][p, hidx] = tree_pass(T, M, root, sigma, best=p)[1][p][0]
    out["valid"][hidx] = True
    return out


def solve_batch(board, ranges, tree, iters, dead=None):
    board = np.asarray(board, np.uint8)
    m = board.shape[0]
    res = [solve_spot([int(x) for x in board[i]], np.asarray(ranges)[i], tree, iters, 0 if dead is None else int(dead[i])) for i in range(m)]
    out = {k: np.stack([np.asarray(r[k]) for r in res]) for k in ("strategy", "value", "br", "status", "valid")}
    out["status"] = out["status"].astype(np.uint8)
    return out


def pair_weight(ranges, valid):
    """sum of w_0[h] w_1[h'] over the valid ordered pairs that share no card (a Python integer)."""
    w = np.asarray(ranges, np.int64).reshape(2, HOLDINGS) * valid
    c0, c1 = np.zeros(52, np.int64), np.zeros(52, np.int64)
    np.add.at(c0, VS.PAIR_A, w[0]); np.add.at(c0, VS.PAIR_B, w[0])
    np.add.at(c1, VS.PAIR_A, w[1]); np.add.at(c1, VS.PAIR_B, w[1])
    tot = int(w[0].sum()) * int(w[1].sum()) - sum(int(a) * int(b) for a, b in zip(c0, c1)) + sum(int(a) * int(b) for a, b in zip(w[0], w[1]))
    return tot


def ev(ranges, value, valid):
    """chips per player: sum_h w_p[h] value[p][h] / (32 sum_disjoint w_0 w_1)"""
    den = 32 * pair_weight(ranges, valid)
    w = np.asarray(ranges).reshape(2, HOLDINGS)
    return [sum(int(a) * int(b) for a, b in zip(w[p], value[p])) / den if den else float("nan") for p in (0, 1)]


def exploitability(ranges, value, br, valid):
    """sum_p (br_p - value_p) reduced the same way, in chips: Python integers, one division"""
    den = 32 * pair_weight(ranges, valid)
    w = np.asarray(ranges).reshape(2, HOLDINGS)
    num = sum(int(w[p][h]) * (int(br[p][h]) - int(value[p][h])) for p in (0, 1) for h in range(HOLDINGS))
    return num / den if den else float("nan")


# ------------------------------------------------------------------------------------------------ the float witness
def float_exploitability(board, ranges, tree, strategy, dead=0):
    """The exploitability of `strategy` (uint16 [D, 4, 1326]) in chips, in float64, from the payoffs of the game alone: a fold costs the
    folder what it put in and gives the other player the pot and that; a showdown gives the winner the pot and the loser's chips, costs the
    loser its own, and splits the pot on a tie.  A recursive walk per player over float reaches; no code shared with the integer passes."""
    T = as_tree(tree)
    _, gone = check_spot(board, dead)
    hidx, beats, ties, loses = pairwise(board, gone)
    sign = (beats - loses).astype(np.float64)                 # +1 / 0 / -1 on disjoint pairs
    meet = (beats + ties + loses).astype(np.float64)
    w = np.asarray(ranges, np.float64).reshape(2, HOLDINGS)[:, hidx]
    prob = {d: np.asarray(strategy)[row][:, hidx].astype(np.float64) / ONE for row, d in enumerate(T.decisions)}

    def payoff(p, n):
        """[n, n] chips player p (row: p's holding) collects at leaf n against the column holding: p gets the whole pot and the
        opponent's chips when it wins, loses its own when it loses, half the pot on a tie"""
        k = T.kind[n]
        if k == SHOWDOWN:
            c = float(T.put[n][0])
            return meet * (T.pot / 2.0) + sign * (T.pot / 2.0 + c)
        f = k - FOLD0
        return meet * (-float(T.put[n][f]) if p == f else float(T.pot + T.put[n][f]))

    def walk(p, n, rq, best):
        """the value of node n per holding of p, against the opponent's reach rq"""
        k = T.kind[n]
        if k > 1:
            return payoff(p, n) @ rq
        vals = [walk(p, c, rq if k == p else rq * prob[n][a], best) for a, c in enumerate(T.child[n])]
        if k != p:
            return np.sum(vals, axis=0)
        return np.max(vals, axis=0) if best else np.sum([prob[n][a] * v for a, v in enumerate(vals)], axis=0)

    den = float(w[0] @ meet @ w[1])
    gap = sum(float(w[p] @ (walk(p, 0, w[1 - p], True) - walk(p, 0, w[1 - p], False))) for p in (0, 1))
    return gap / den
