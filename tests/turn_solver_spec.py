"""The turn-solver definition restated in numpy int64 (TEST INFRASTRUCTURE): include/pokerl_hip.h "Turn solver" / DESIGN.md section 3.13.
Everything below a chance node is the river solver's definition on the board plus the river card: the beats / ties / loses matrices come from
river_solver_spec.pairwise, once per river card, so there is no sort and no comparison of ranking words here either.  Every sum is an
integer sum.  float_exploitability, at the end, is a SEPARATE float64 best response written from the payoffs of the game (chance divides by
P - 4, utilities in chips); it shares no code with the integer passes."""
import itertools

import numpy as np

import river_solver_spec as RS
import rvr_spec as VS

HOLDINGS, ONE = RS.HOLDINGS, RS.ONE
P0, P1, FOLD0, FOLD1, SHOWDOWN, CHANCE = 0, 1, 2, 3, 4, 5
BAD_CARD, DUP_CARD, SMALL_POOL = VS.BAD_CARD, VS.DUP_CARD, VS.SMALL_POOL


class Tree(RS.Tree):
    """RS.Tree plus river[n]: node n lies below a chance node."""

    def __init__(self, kind, child, put, pot):
        super().__init__(kind, child, put, pot)
        self.river = [False] * self.n
        for n in range(self.n):
            for c in self.child[n]:
                self.river[c] = self.river[n] or self.kind[n] == CHANCE
        self.turn_decisions = [d for d in self.decisions if not self.river[d]]
        self.river_decisions = [d for d in self.decisions if self.river[d]]


def as_tree(t):
    return t if isinstance(t, Tree) else Tree(t.kind, t.child, t.put, t.pot)


def check_spot(board, dead=0):
    status, gone = VS.check_spot(board, 4, dead)
    status &= ~VS.PREFLOP
    if not status and 52 - len(gone) < 5:
        status |= SMALL_POOL
    return status, gone


class Spot:
    """What one valid spot's passes share: the pool, the turn holdings (fixed indices hidx, in pool order), which of them share a card
    (disjoint int64 [nT, nT]) and, per river card k of the pool (a canonical index): where the holdings without k sit among the turn
    holdings (idx) and their pairwise result (res int8 [n, n]: 0 = share a card, 1 = beats, 2 = loses, 3 = ties)."""

    def __init__(self, board, gone):
        self.pool = [k for k in range(52) if k not in gone]
        self.P = len(self.pool)
        hold = np.array(list(itertools.combinations(range(self.P), 2)), np.int64)
        pc = np.array(self.pool, np.int64)
        self.hidx = pc[hold[:, 1]] * (pc[hold[:, 1]] - 1) // 2 + pc[hold[:, 0]]
        self.cards = pc[hold]                                                      # [nT, 2] canonical indices
        share = (hold[:, None, 0] == hold[None, :, 0]) | (hold[:, None, 0] == hold[None, :, 1]) | \
                (hold[:, None, 1] == hold[None, :, 0]) | (hold[:, None, 1] == hold[None, :, 1])
        self.disjoint = (~share).astype(np.int64)
        where = {int(h): i for i, h in enumerate(self.hidx)}
        self.river = []
        for k in self.pool:
            hidx, beats, ties, loses = RS.pairwise(list(board[:4]) + [int(VS.CANON[k])], set(gone) | {k})
            self.river.append((k, np.array([where[int(h)] for h in hidx], np.int64), (beats + 2 * loses + 3 * ties).astype(np.int8)))

    @staticmethod
    def matrices(res):
        return (res == 1).astype(np.int64), (res == 3).astype(np.int64), (res == 2).astype(np.int64)


_SPOTS = {}


def spot_of(board, gone):
    key = (tuple(int(x) for x in board[:4]), frozenset(gone))
    if key not in _SPOTS:
        if len(_SPOTS) > 8:
            _SPOTS.clear()
        _SPOTS[key] = Spot(board, gone)
    return _SPOTS[key]


def terminal(T, n, M, rq0, rq1):
    """River's terminal formulas at node n: (u_0, u_1) from the opponents' reaches (rq0 = r_1, rq1 = r_0)."""
    beats, ties, loses = M
    k, out = T.kind[n], []
    for p, rq in ((0, rq0), (1, rq1)):
        if k == SHOWDOWN:
            c = T.put[n][0]
            out.append(2 * (T.pot + c) * (beats @ rq) + T.pot * (ties @ rq) - 2 * c * (loses @ rq))
        else:
            f = k - FOLD0
            S = (beats + ties + loses) @ rq
            out.append(-2 * T.put[n][f] * S if p == f else 2 * (T.pot + T.put[n][f]) * S)
    return out


def tree_pass(T, sp, root, sigma, best=None):
    """One pass over the whole tree.  root = (r_0, r_1) int64 [nT]; sigma[d]: int64 [nact, nT] at a turn-level decision node, a list over
    the river cards of int64 [nact, n_c] at a river-level one.  best = p: p's best-response pass.
    -> (r, u): r[p][node], u[p][node]: an array at a turn-level node, a list of arrays (one per river card) at a river-level one."""
    K = sp.P - 4
    C = range(len(sp.river))
    r = [{0: root[0]}, {0: root[1]}]
    u = [{}, {}]
    for n in range(T.n):
        k = T.kind[n]
        if k <= 1:
            for a, c in enumerate(T.child[n]):
                if T.river[n]:
                    r[k][c] = [r[k][n][j] if best == k else (r[k][n][j] * sigma[n][j][a]) >> 15 for j in C]
                else:
                    r[k][c] = r[k][n] if best == k else (r[k][n] * sigma[n][a]) >> 15
                r[1 - k][c] = r[1 - k][n]
        elif k == CHANCE:
            c = T.child[n][0]
            for p in (0, 1):
                r[p][c] = [r[p][n][idx] for _, idx, _ in sp.river]                # (the holdings with the card are not among idx)
        elif T.river[n]:
            res = [terminal(T, n, sp.matrices(sp.river[j][2]), r[1][n][j], r[0][n][j]) for j in C]
            u[0][n], u[1][n] = [x[0] for x in res], [x[1] for x in res]
        else:                                                                     # a turn-level fold: every one of the K river cards
            f = k - FOLD0
            for p in (0, 1):
                S = sp.disjoint @ r[1 - p][n]
                u[p][n] = -2 * T.put[n][f] * K * S if p == f else 2 * (T.pot + T.put[n][f]) * K * S
    for n in reversed(range(T.n)):
        k = T.kind[n]
        if k == CHANCE:
            c = T.child[n][0]
            for p in (0, 1):
                tot = np.zeros(len(sp.hidx), np.int64)
                for j, (_, idx, _) in enumerate(sp.river):
                    tot[idx] += u[p][c][j]
                u[p][n] = tot
            continue
        if k > 1:
            continue
        ch = T.child[n]
        if T.river[n]:
            if best == k:
                u[k][n] = [np.max(np.stack([u[k][c][j] for c in ch]), axis=0) for j in C]
            else:
                u[k][n] = [sum(sigma[n][j][a] * u[k][c][j] for a, c in enumerate(ch)) // ONE for j in C]
            u[1 - k][n] = [sum(u[1 - k][c][j] for c in ch) for j in C]
        else:
            if best == k:
                u[k][n] = np.max(np.stack([u[k][c] for c in ch]), axis=0)
            else:
                u[k][n] = sum(sigma[n][a] * u[k][c] for a, c in enumerate(ch)) // ONE
            u[1 - k][n] = sum(u[1 - k][c] for c in ch)
    return r, u


def solve_spot(board, ranges, tree, iters, dead=0):
    """One spot -> dict(strategy uint16 [D_t, 4, 1326], river_strategy uint16 [D_r, 52, 4, 1326], value, br int64 [2, 1326], status,
    valid bool [1326], regret_bits, P)."""
    T = as_tree(tree)
    Dt, Dr = len(T.turn_decisions), len(T.river_decisions)
    out = dict(strategy=np.zeros((Dt, 4, HOLDINGS), np.uint16), river_strategy=np.zeros((Dr, 52, 4, HOLDINGS), np.uint16),
               value=np.zeros((2, HOLDINGS), np.int64), br=np.zeros((2, HOLDINGS), np.int64), valid=np.zeros(HOLDINGS, bool), regret_bits=0, P=0)
    status, gone = check_spot(board, dead)
    out["status"] = status
    if status:
        return out
    sp = spot_of(board, gone)
    out["P"] = sp.P
    nT = len(sp.hidx)
    w = np.asarray(ranges, np.int64).reshape(2, HOLDINGS)[:, sp.hidx]
    root = (w[0] << 1, w[1] << 1)

    def zeros(d):
        if T.river[d]:
            return [np.zeros((len(T.child[d]), len(idx)), np.int64) for _, idx, _ in sp.river]
        return np.zeros((len(T.child[d]), nT), np.int64)

    def rule(X, d):
        return [RS.strategy_from(x) for x in X[d]] if T.river[d] else RS.strategy_from(X[d])

    R = {d: zeros(d) for d in T.decisions}
    A = {d: zeros(d) for d in T.decisions}
    for t in range(1, int(iters) + 1):
        sigma = {d: rule(R, d) for d in T.decisions}
        r, u = tree_pass(T, sp, root, sigma)
        for d in T.decisions:
            p = T.kind[d]
            for a, c in enumerate(T.child[d]):
                if T.river[d]:
                    for j in range(sp.P):
                        R[d][j][a] = np.maximum(0, R[d][j][a] + u[p][c][j] - u[p][d][j])
                        A[d][j][a] += t * r[p][c][j]
                    out["regret_bits"] = max([out["regret_bits"]] + [int(x.max()).bit_length() for x in R[d]])
                else:
                    R[d][a] = np.maximum(0, R[d][a] + u[p][c] - u[p][d])
                    A[d][a] += t * r[p][c]
                    out["regret_bits"] = max(out["regret_bits"], int(R[d].max()).bit_length())
    sigma = {d: rule(A, d) for d in T.decisions}
    for row, d in enumerate(T.turn_decisions):
        out["strategy"][row, :len(T.child[d]), sp.hidx] = sigma[d].T
    for row, d in enumerate(T.river_decisions):
        for j, (k, idx, _) in enumerate(sp.river):
            out["river_strategy"][row, k, :len(T.child[d]), sp.hidx[idx]] = sigma[d][j].T
    _, u = tree_pass(T, sp, root, sigma)
    for p in (0, 1):
        out["value"][p, sp.hidx] = u[p][0]
        out["br"][p, sp.hidx] = tree_pass(T, sp, root, sigma, best=p)[1][p][0]
    out["valid"][sp.hidx] = True
    return out


KEYS = ("strategy", "river_strategy", "value", "br", "status", "valid", "P")


def solve_batch(board, ranges, tree, iters, dead=None):
    board = np.asarray(board, np.uint8)
    res = [solve_spot([int(x) for x in board[i]], np.asarray(ranges)[i], tree, iters, 0 if dead is None else int(dead[i])) for i in range(board.shape[0])]
    out = {k: np.stack([np.asarray(r[k]) for r in res]) for k in KEYS}
    out["status"] = out["status"].astype(np.uint8)
    out["regret_bits"] = max([r["regret_bits"] for r in res] + [0])
    return out


def ev(ranges, value, valid, P):
    """chips per player: sum_h w_p[h] value[p][h] / (4 (P - 4) sum_disjoint w_0 w_1)"""
    den = 4 * (int(P) - 4) * RS.pair_weight(ranges, valid)
    w = np.asarray(ranges).reshape(2, HOLDINGS)
    return [sum(int(a) * int(b) for a, b in zip(w[p], value[p])) / den if den else float("nan") for p in (0, 1)]


def exploitability(ranges, value, br, valid, P):
    """sum_p (br_p - value_p) reduced the same way, in chips: Python integers, one division"""
    den = 4 * (int(P) - 4) * RS.pair_weight(ranges, valid)
    w = np.asarray(ranges).reshape(2, HOLDINGS)
    num = sum(int(w[p][h]) * (int(br[p][h]) - int(value[p][h])) for p in (0, 1) for h in range(HOLDINGS))
    return num / den if den else float("nan")


# ------------------------------------------------------------------------------------------------ the float witness
def float_exploitability(board, ranges, tree, strategy, river_strategy, dead=0):
    """The exploitability of (strategy, river_strategy) in chips, in float64, from the payoffs of the game alone: a fold costs the folder
    what it put in and gives the other player the pot and that; a showdown gives the winner the pot and the loser's chips, costs the loser
    its own, and splits the pot on a tie; the river card is each of the P - 4 cards neither player holds with the same probability.  A
    recursive walk per player over float reaches; no code shared with the integer passes."""
    T = as_tree(tree)
    _, gone = check_spot(board, dead)
    sp = spot_of(board, gone)
    chance = 1.0 / (sp.P - 4)
    meet_t = sp.disjoint.astype(np.float64)
    w = np.asarray(ranges, np.float64).reshape(2, HOLDINGS)[:, sp.hidx]
    prob_t = {d: np.asarray(strategy)[row][:, sp.hidx].astype(np.float64) / ONE for row, d in enumerate(T.turn_decisions)}
    prob_r = {d: [np.asarray(river_strategy)[row, k][:, sp.hidx[idx]].astype(np.float64) / ONE for k, idx, _ in sp.river]
              for row, d in enumerate(T.river_decisions)}

    def payoff(p, n, j):
        """chips player p (row: p's holding) collects at leaf n against the column holding; j: the river card's number, None on the turn"""
        k = T.kind[n]
        if j is None:
            meet = meet_t
        else:
            res = sp.river[j][2]
            meet = (res != 0).astype(np.float64)
        if k == SHOWDOWN:
            sign = (res == 1).astype(np.float64) - (res == 2).astype(np.float64)
            return meet * (T.pot / 2.0) + sign * (T.pot / 2.0 + float(T.put[n][0]))
        f = k - FOLD0
        return meet * (-float(T.put[n][f]) if p == f else float(T.pot + T.put[n][f]))

    def walk(p, n, rq, best, j):
        k = T.kind[n]
        if k == CHANCE:
            tot = np.zeros(len(sp.hidx))
            for jj, (_, idx, _) in enumerate(sp.river):
                tot[idx] += chance * walk(p, T.child[n][0], rq[idx], best, jj)
            return tot
        if k > 1:
            return payoff(p, n, j) @ rq
        prob = prob_t[n] if j is None else prob_r[n][j]
        vals = [walk(p, c, rq if k == p else rq * prob[a], best, j) for a, c in enumerate(T.child[n])]
        if k != p:
            return np.sum(vals, axis=0)
        return np.max(vals, axis=0) if best else np.sum([prob[a] * v for a, v in enumerate(vals)], axis=0)

    den = float(w[0] @ meet_t @ w[1])
    gap = sum(float(w[p] @ (walk(p, 0, w[1 - p], True, None) - walk(p, 0, w[1 - p], False, None))) for p in (0, 1))
    return gap / den
