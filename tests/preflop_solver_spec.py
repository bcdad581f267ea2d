"""The pre-flop solver's definition restated in numpy int64 (TEST INFRASTRUCTURE): include/pokerl_hip.h "Pre-flop solver" / DESIGN.md section
3.18.  It is river_solver_spec's iteration with one terminal swapped: a spot has no board, every holding is valid, and a showdown is paid by a
matchup table (win, tie uint32 [1326, 1326]) that every function here TAKES AS AN ARGUMENT -- the device's own table on the GPU, a synthetic one
on the CPU.  Nothing here assumes anything of the table: E sums over all 1 326 columns, whatever they hold; S sums over the holdings that share
no card.  Every sum is an integer sum, so no result depends on its order.  float_exploitability, at the end, is a SEPARATE float64 best
response written from the game's payoffs; it shares no code with the integer passes."""
import numpy as np

import river_solver_spec as RVS

HOLDINGS = 1326
ONE = 32768
BOARDS = 1712304            # PK_PREFLOP_BOARDS = C(48, 5)
P0, P1, FOLD0, FOLD1, SHOWDOWN = 0, 1, 2, 3, 4
BAD_TREE = 32
PAIR_A = np.array([a for b in range(52) for a in range(b)])
PAIR_B = np.array([b for b in range(52) for a in range(b)])
SHARE = (PAIR_A[:, None] == PAIR_A[None, :]) | (PAIR_A[:, None] == PAIR_B[None, :]) | (PAIR_B[:, None] == PAIR_A[None, :]) | (PAIR_B[:, None] == PAIR_B[None, :])
DISJOINT = (~SHARE).astype(np.int64)

Tree, as_tree, strategy_from = RVS.Tree, RVS.as_tree, RVS.strategy_from


def synthetic_table(seed):
    """A table with the real one's structure and made-up counts: 0 where two holdings share a card; on a disjoint pair tie symmetric and
    win[h][o] + win[o][h] + tie[h][o] = BOARDS, the split following a random strength per holding."""
    rng = np.random.default_rng(seed)
    s = rng.integers(1, 1 << 20, HOLDINGS).astype(np.int64)
    t = rng.integers(0, 60000, (HOLDINGS, HOLDINGS)).astype(np.int64)
    tie = np.triu(t, 1)
    tie = tie + tie.T
    up = ((BOARDS - tie) * s[:, None]) // (s[:, None] + s[None, :])
    win = np.triu(up, 1) + np.tril(BOARDS - tie - up.T, -1)
    return (win * DISJOINT).astype(np.uint32), (tie * DISJOINT).astype(np.uint32)


def weight_matrix(table):
    """G = 2 win + tie, int64 [1326, 1326]"""
    win, tie = table
    return 2 * np.asarray(win, np.int64) + np.asarray(tie, np.int64)


def showdown(G, pot, c, rq, record=None):
    """u[h] = floor((pot + 2c) E[h] / B) - 2c S[h], the product formed as (pot + 2c) (E div B) + ((pot + 2c) (E mod B)) div B"""
    E, S, chips = G @ rq, DISJOINT @ rq, pot + 2 * c
    if record is not None:
        record["E"] = max(record.get("E", 0), int(E.max()))
    return chips * (E // BOARDS) + (chips * (E % BOARDS)) // BOARDS - 2 * c * S


def tree_pass(T, G, root, sigma, best=None, record=None):
    """One tree pass, river_solver_spec.tree_pass with the pre-flop terminals.  -> (r, u): r[p][node], u[p][node] int64 [1326]."""
    r = [{0: root[0]}, {0: root[1]}]
    u = [{}, {}]
    for n in range(T.n):
        k = T.kind[n]
        if k <= 1:
            for a, c in enumerate(T.child[n]):
                r[k][c] = r[k][n] if best == k else (r[k][n] * sigma[n][a]) >> 15
                r[1 - k][c] = r[1 - k][n]
        elif k == SHOWDOWN:
            for p in (0, 1):
                u[p][n] = showdown(G, T.pot, T.put[n][0], r[1 - p][n], record)
        else:
            f = k - FOLD0
            for p in (0, 1):
                S = DISJOINT @ r[1 - p][n]
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


def solve_spot(table, ranges, tree, iters, state=None, G=None):
    """One spot -> dict(strategy uint16 [D, 4, 1326], value, br int64 [2, 1326], status, valid).  state = (R, A, t0), R and A dicts
    {decision node: int64 [nact, 1326]}: the iterations run t0 + 1 .. t0 + iters from them (the witness's corner; the device starts from
    nothing).  G: weight_matrix(table) where the caller has it already."""
    T = as_tree(tree)
    G = weight_matrix(table) if G is None else G
    D = len(T.decisions)
    out = dict(strategy=np.zeros((D, 4, HOLDINGS), np.uint16), value=np.zeros((2, HOLDINGS), np.int64), br=np.zeros((2, HOLDINGS), np.int64),
               valid=np.ones(HOLDINGS, bool), status=0)
    w = np.asarray(ranges, np.int64).reshape(2, HOLDINGS)
    root = (w[0] << 4, w[1] << 4)
    R = {d: np.zeros((len(T.child[d]), HOLDINGS), np.int64) for d in T.decisions}
    A = {d: np.zeros((len(T.child[d]), HOLDINGS), np.int64) for d in T.decisions}
    t0 = 0
    if state is not None:
        R, A, t0 = {d: np.array(state[0][d], np.int64) for d in T.decisions}, {d: np.array(state[1][d], np.int64) for d in T.decisions}, int(state[2])
    for t in range(t0 + 1, t0 + int(iters) + 1):
        sigma = {d: strategy_from(R[d]) for d in T.decisions}
        r, u = tree_pass(T, G, root, sigma)
        for d in T.decisions:
            p = T.kind[d]
            for a, c in enumerate(T.child[d]):
                R[d][a] = np.maximum(0, R[d][a] + u[p][c] - u[p][d])
                A[d][a] += t * r[p][c]
    sigma = {d: strategy_from(A[d]) for d in T.decisions}
    for row, d in enumerate(T.decisions):
        out["strategy"][row, :len(T.child[d])] = sigma[d]
    _, u = tree_pass(T, G, root, sigma)
    for p in (0, 1):
        out["value"][p] = u[p][0]
        out["br"][p] = tree_pass(T, G, root, sigma, best=p)[1][p][0]
    return out


def solve_batch(table, ranges, trees, iters, tree_of=None):
    """m spots, a tree per spot as pk_solve_preflop takes them: trees a tree or a list, tree_of None (tree 0 everywhere) or integers [m].
    strategy has the call's stride Dmax; a spot whose tree_of names no tree: BAD_TREE and zeros."""
    trees = list(trees) if isinstance(trees, (list, tuple)) else [trees]
    ranges = np.asarray(ranges)
    m = ranges.shape[0]
    G = weight_matrix(table)
    Dmax = max(len(as_tree(t).decisions) for t in trees)
    out = dict(strategy=np.zeros((m, Dmax, 4, HOLDINGS), np.uint16), value=np.zeros((m, 2, HOLDINGS), np.int64), br=np.zeros((m, 2, HOLDINGS), np.int64),
               status=np.zeros(m, np.uint8), valid=np.zeros((m, HOLDINGS), bool))
    for i in range(m):
        k = 0 if tree_of is None else int(tree_of[i])
        if k >= len(trees):
            out["status"][i] = BAD_TREE
            continue
        r = solve_spot(table, ranges[i], trees[k], iters, G=G)
        out["strategy"][i, :r["strategy"].shape[0]] = r["strategy"]
        out["value"][i], out["br"][i], out["valid"][i] = r["value"], r["br"], r["valid"]
    return out


def ev(ranges, value):
    return RVS.ev(ranges, value, np.ones(HOLDINGS, bool))


def exploitability(ranges, value, br):
    """sum_p (br_p - value_p) / (32 sum over disjoint pairs of w_0 w_1), in chips: Python integers, one division"""
    return RVS.exploitability(ranges, value, br, np.ones(HOLDINGS, bool))


# ------------------------------------------------------------------------------------------------ the float witness
def float_exploitability(table, ranges, tree, strategy):
    """The exploitability of `strategy` (uint16 [D, 4, 1326]) in chips, in float64, from the payoffs of the game alone: a fold costs the
    folder what it put in and gives the other player the pot and that; a showdown is the all-in equity of the two holdings -- on the share
    of boards it wins a player collects the pot and the opponent's chips, on the share it ties half the pot, on the rest it loses its
    own.  A recursive walk per player over float reaches; no code shared with the integer passes."""
    T = as_tree(tree)
    win, tie = (np.asarray(x, np.float64) / BOARDS for x in table)
    meet = (~SHARE).astype(np.float64)
    lose = meet - win - tie
    w = np.asarray(ranges, np.float64).reshape(2, HOLDINGS)
    prob = {d: np.asarray(strategy)[row].astype(np.float64) / ONE for row, d in enumerate(T.decisions)}

    def payoff(p, n):
        """[1326, 1326] chips player p (row: p's holding) collects at leaf n against the column holding"""
        k = T.kind[n]
        if k == SHOWDOWN:
            c = float(T.put[n][0])
            return win * (T.pot + c) + tie * (T.pot / 2.0) - lose * c
        f = k - FOLD0
        return meet * (-float(T.put[n][f]) if p == f else float(T.pot + T.put[n][f]))

    def walk(p, n, rq, best):
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
