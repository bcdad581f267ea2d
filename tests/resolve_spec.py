"""The re-solving definition restated in numpy int64 (TEST INFRASTRUCTURE): include/pokerl_hip.h "Re-solving" / DESIGN.md section 3.16.
solver_lock_spec (and through it river_solver_spec / turn_solver_spec) is imported, not edited.  A re-solving call differs from the locked
call in what the definition says and in nothing else: the root reaches may come from `reach` (min(reach, LIM), no shift), a river tree may
hold one terminal of kind 6 whose values are clamp(given), and the reaches, values and best-response values of the final pass are reported
at node `at` (turn: of a river-level node under river card at_card).  The river pass is written out here because river_solver_spec's knows
no kind 6; the turn pass is turn_solver_spec's.  excess, at the end, is a SEPARATE float64 best response from the payoffs of the game."""
import numpy as np

import river_solver_spec as RS
import solver_lock_spec as LS
import turn_solver_spec as TS

HOLDINGS, ONE = RS.HOLDINGS, RS.ONE
GIVEN = 6
RIVER_LIM, TURN_LIM = (1 << 20) - 1, (1 << 17) - 1
GIVEN_LIM = (1 << 45) - 1
BAD_CARD, BAD_TREE = RS.BAD_CARD, 32
NODE_KEYS = ("node_reach", "node_value", "node_br")


def canon_of(card):
    """a card code (as on the board) -> its canonical index, None for no card"""
    card = int(card)
    return None if card >= 0x40 or (card & 15) >= 13 else (card & 15) * 4 + (card >> 4)


def river_pass(T, M, root, sigma, given=None, best=None):
    """river_solver_spec.tree_pass with the given terminal: u_p = given[p] there, whatever the reaches, in every kind of pass."""
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
        elif k == GIVEN:
            for p in (0, 1):
                u[p][n] = given[p]
        elif k == RS.SHOWDOWN:
            c = T.put[n][0]
            for p in (0, 1):
                rq = r[1 - p][n]
                u[p][n] = 2 * (T.pot + c) * (beats @ rq) + T.pot * (ties @ rq) - 2 * c * (loses @ rq)
        else:
            f = k - RS.FOLD0
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


def _root(ranges, reach, hidx, shift, lim):
    if reach is not None:
        w = np.minimum(np.asarray(reach).astype(np.int64).reshape(2, HOLDINGS)[:, hidx], lim)
        return (w[0], w[1])
    w = np.asarray(ranges, np.int64).reshape(2, HOLDINGS)[:, hidx]
    return (w[0] << shift, w[1] << shift)


def _empty_nodes(out):
    out["node_reach"] = np.zeros((2, HOLDINGS), np.uint32)
    out["node_value"], out["node_br"] = np.zeros((2, HOLDINGS), np.int64), np.zeros((2, HOLDINGS), np.int64)


def solve_river_spot(board, ranges, tree, iters, lock=None, locked=None, dead=0, reach=None, given=None, at=None):
    """One river spot of pk_solve_river_resolve -> solver_lock_spec's dict plus node_reach uint32 / node_value / node_br int64 [2, 1326]
    (zeros where at is None)."""
    T = RS.as_tree(tree)
    D = len(T.decisions)
    out = dict(strategy=np.zeros((D, 4, HOLDINGS), np.uint16), value=np.zeros((2, HOLDINGS), np.int64), br=np.zeros((2, HOLDINGS), np.int64),
               valid=np.zeros(HOLDINGS, bool))
    _empty_nodes(out)
    status, gone = RS.check_spot(board, dead)
    if 52 - len(gone) < 4:
        status |= RS.SMALL_POOL
    if not status and at is not None and int(at) >= T.n:
        status |= BAD_TREE
    out["status"] = status
    if status:
        return out
    hidx, beats, ties, loses = RS.pairwise(board, gone)
    M = (beats, ties, loses)
    root = _root(ranges, reach, hidx, 4, RIVER_LIM)
    g = None
    if GIVEN in T.kind:
        g = np.clip(np.asarray(given).astype(np.int64).reshape(2, HOLDINGS)[:, hidx], -GIVEN_LIM, GIVEN_LIM)
    n = len(hidx)
    flags = LS._flags(lock, D)
    fixed = {d: RS.strategy_from(np.asarray(locked)[row, :len(T.child[d])][:, hidx].astype(np.int64))
             for row, d in enumerate(T.decisions) if flags[row]}
    R = {d: np.zeros((len(T.child[d]), n), np.int64) for d in T.decisions}
    A = {d: np.zeros((len(T.child[d]), n), np.int64) for d in T.decisions}
    for t in range(1, int(iters) + 1):
        sigma = {d: fixed[d] if d in fixed else RS.strategy_from(R[d]) for d in T.decisions}
        r, u = river_pass(T, M, root, sigma, g)
        for d in T.decisions:
            if d in fixed:
                continue
            p = T.kind[d]
            for a, c in enumerate(T.child[d]):
                R[d][a] = np.maximum(0, R[d][a] + u[p][c] - u[p][d])
                A[d][a] += t * r[p][c]
    sigma = {d: fixed[d] if d in fixed else RS.strategy_from(A[d]) for d in T.decisions}
    for row, d in enumerate(T.decisions):
        out["strategy"][row, :len(T.child[d]), hidx] = sigma[d].T
    r, u = river_pass(T, M, root, sigma, g)
    for p in (0, 1):
        ub = river_pass(T, M, root, sigma, g, best=p)[1][p]
        out["value"][p, hidx] = u[p][0]
        out["br"][p, hidx] = ub[0]
        if at is not None:
            out["node_reach"][p, hidx] = r[p][int(at)]
            out["node_value"][p, hidx] = u[p][int(at)]
            out["node_br"][p, hidx] = ub[int(at)]
    out["valid"][hidx] = True
    return out


def solve_turn_spot(board, ranges, tree, iters, lock=None, locked=None, river_lock=None, river_locked=None, dead=0, reach=None, at=None, at_card=None):
    """One turn spot of pk_solve_turn_resolve -> solver_lock_spec's dict plus the node outputs."""
    T = TS.as_tree(tree)
    Dt, Dr = len(T.turn_decisions), len(T.river_decisions)
    out = dict(strategy=np.zeros((Dt, 4, HOLDINGS), np.uint16), river_strategy=np.zeros((Dr, 52, 4, HOLDINGS), np.uint16),
               value=np.zeros((2, HOLDINGS), np.int64), br=np.zeros((2, HOLDINGS), np.int64), valid=np.zeros(HOLDINGS, bool), P=0)
    _empty_nodes(out)
    status, gone = TS.check_spot(board, dead)
    card = None
    if not status and at is not None:
        if int(at) >= T.n:
            status |= BAD_TREE
        elif T.river[int(at)]:
            card = None if at_card is None else canon_of(at_card)
            if card is None or card in gone:
                status |= BAD_CARD
    out["status"] = status
    if status:
        return out
    sp = TS.spot_of(board, gone)
    out["P"] = sp.P
    nT = len(sp.hidx)
    root = _root(ranges, reach, sp.hidx, 1, TURN_LIM)
    tf, rf = LS._flags(lock, Dt), LS._flags(river_lock, Dr)
    fixed = {}
    for row, d in enumerate(T.turn_decisions):
        if tf[row]:
            fixed[d] = RS.strategy_from(np.asarray(locked)[row, :len(T.child[d])][:, sp.hidx].astype(np.int64))
    for row, d in enumerate(T.river_decisions):
        if rf[row]:
            fixed[d] = [RS.strategy_from(np.asarray(river_locked)[row, k, :len(T.child[d])][:, sp.hidx[idx]].astype(np.int64)) for k, idx, _ in sp.river]

    def zeros(d):
        if T.river[d]:
            return [np.zeros((len(T.child[d]), len(idx)), np.int64) for _, idx, _ in sp.river]
        return np.zeros((len(T.child[d]), nT), np.int64)

    def rule(X, d):
        if d in fixed:
            return fixed[d]
        return [RS.strategy_from(x) for x in X[d]] if T.river[d] else RS.strategy_from(X[d])

    R = {d: zeros(d) for d in T.decisions}
    A = {d: zeros(d) for d in T.decisions}
    for t in range(1, int(iters) + 1):
        sigma = {d: rule(R, d) for d in T.decisions}
        r, u = TS.tree_pass(T, sp, root, sigma)
        for d in T.decisions:
            if d in fixed:
                continue
            p = T.kind[d]
            for a, c in enumerate(T.child[d]):
                if T.river[d]:
                    for j in range(sp.P):
                        R[d][j][a] = np.maximum(0, R[d][j][a] + u[p][c][j] - u[p][d][j])
                        A[d][j][a] += t * r[p][c][j]
                else:
                    R[d][a] = np.maximum(0, R[d][a] + u[p][c] - u[p][d])
                    A[d][a] += t * r[p][c]
    sigma = {d: rule(A, d) for d in T.decisions}
    for row, d in enumerate(T.turn_decisions):
        out["strategy"][row, :len(T.child[d]), sp.hidx] = sigma[d].T
    for row, d in enumerate(T.river_decisions):
        for j, (k, idx, _) in enumerate(sp.river):
            out["river_strategy"][row, k, :len(T.child[d]), sp.hidx[idx]] = sigma[d][j].T
    r, u = TS.tree_pass(T, sp, root, sigma)
    for p in (0, 1):
        ub = TS.tree_pass(T, sp, root, sigma, best=p)[1][p]
        out["value"][p, sp.hidx] = u[p][0]
        out["br"][p, sp.hidx] = ub[0]
        if at is None:
            continue
        v = int(at)
        if not T.river[v]:
            where, pick = sp.hidx, lambda x: x
        else:
            j = [k for k, _, _ in sp.river].index(card)
            where, pick = sp.hidx[sp.river[j][1]], lambda x: x[j]
        out["node_reach"][p, where] = pick(r[p][v])
        out["node_value"][p, where] = pick(u[p][v])
        out["node_br"][p, where] = pick(ub[v])
    out["valid"][sp.hidx] = True
    return out


def _refuse(spot, keys):
    for key in keys:
        spot[key] = np.zeros_like(spot[key])
    spot["status"] |= BAD_TREE


def _pick(x, i):
    return None if x is None else x[i]


def solve_river_batch(board, ranges, trees, tree_of, iters, lock=None, locked=None, dead=None, reach=None, given=None, at=None):
    """A call: as solver_lock_spec.solve_river_batch, with reach / given [m, 2, 1326] and at [m] or None; tree_of None: every spot tree 0."""
    Dmax = max(len(RS.as_tree(t).decisions) for t in trees)
    res = []
    for i in range(len(board)):
        k = 0 if tree_of is None else int(tree_of[i])
        spot = solve_river_spot([int(x) for x in board[i]], _pick(ranges, i), trees[min(k, len(trees) - 1)], iters, _pick(lock, i), _pick(locked, i),
                                0 if dead is None else int(dead[i]), _pick(reach, i), _pick(given, i), _pick(at, i))
        if k >= len(trees):
            # (the tree is judged before the node: a spot whose tree does not exist reports that alone)
            spot["status"] &= ~BAD_TREE
            _refuse(spot, ("strategy", "value", "br", "valid") + NODE_KEYS)
        spot["strategy"] = LS._pad(spot["strategy"], Dmax)
        res.append(spot)
    out = {k: np.stack([np.asarray(r[k]) for r in res]) for k in ("strategy", "value", "br", "status", "valid") + NODE_KEYS}
    out["status"] = out["status"].astype(np.uint8)
    return out


def solve_turn_batch(board, ranges, trees, tree_of, iters, lock=None, locked=None, river_lock=None, river_locked=None, dead=None, reach=None, at=None,
                     at_card=None):
    """As solve_river_batch, with both levels' strides."""
    Dt = max(len(TS.as_tree(t).turn_decisions) for t in trees)
    Dr = max(len(TS.as_tree(t).river_decisions) for t in trees)
    res = []
    for i in range(len(board)):
        k = 0 if tree_of is None else int(tree_of[i])
        if k >= len(trees):
            # (no tree: the node is not judged; the spot's own faults and BAD_TREE are all its status holds)
            spot = solve_turn_spot([int(x) for x in board[i]], _pick(ranges, i), trees[0], 0, dead=0 if dead is None else int(dead[i]), reach=_pick(reach, i))
            _refuse(spot, ("strategy", "river_strategy", "value", "br", "valid") + NODE_KEYS)
            spot["P"] = 0
        else:
            spot = solve_turn_spot([int(x) for x in board[i]], _pick(ranges, i), trees[k], iters, _pick(lock, i), _pick(locked, i), _pick(river_lock, i),
                                   _pick(river_locked, i), 0 if dead is None else int(dead[i]), _pick(reach, i), _pick(at, i), _pick(at_card, i))
        spot["strategy"], spot["river_strategy"] = LS._pad(spot["strategy"], Dt), LS._pad(spot["river_strategy"], Dr)
        res.append(spot)
    out = {k: np.stack([np.asarray(r[k]) for r in res]) for k in ("strategy", "river_strategy", "value", "br", "status", "valid", "P") + NODE_KEYS}
    out["status"] = out["status"].astype(np.uint8)
    return out


# ------------------------------------------------------------------------------------------------ the float witness
def excess(board, tree, reach, strategy, q, promised, dead=0):
    """How much more than it was promised the opponent q can take from the subgame `tree` (no given node) when the other player plays
    `strategy` (uint16 [D, 4, 1326], tree's rows) from the reaches `reach` [2, 1326] at its root:
        sum over q's valid holdings h of max(0, br'_q[h] - promised[h] / 2)  /  (the other player's total reach * the number of those h),
    in chips: br'_q[h] is q's best-response counterfactual value in chips times reach, promised the solver's half-chips times reach.
    float64, from the payoffs of the game alone, as river_solver_spec.float_exploitability's walk: a fold costs the folder what it put in
    and gives the other player the pot and that; a showdown gives the winner the pot and the loser's chips, costs the loser its own, and
    splits the pot on a tie.  No code shared with the integer passes."""
    T = RS.as_tree(tree)
    _, gone = RS.check_spot(board, dead)
    hidx, beats, ties, loses = RS.pairwise(board, gone)
    sign = (beats - loses).astype(np.float64)
    meet = (beats + ties + loses).astype(np.float64)
    hero = 1 - int(q)
    w = np.asarray(reach).astype(np.float64).reshape(2, HOLDINGS)[hero, hidx]
    prob = {d: np.asarray(strategy)[row][:, hidx].astype(np.float64) / ONE for row, d in enumerate(T.decisions)}

    def payoff(n):
        k = T.kind[n]
        if k == RS.SHOWDOWN:
            return meet * (T.pot / 2.0) + sign * (T.pot / 2.0 + float(T.put[n][0]))
        f = k - RS.FOLD0
        return meet * (-float(T.put[n][f]) if int(q) == f else float(T.pot + T.put[n][f]))

    def walk(n, rq):
        k = T.kind[n]
        if k > 1:
            return payoff(n) @ rq
        vals = [walk(c, rq if k == int(q) else rq * prob[n][a]) for a, c in enumerate(T.child[n])]
        return np.max(vals, axis=0) if k == int(q) else np.sum(vals, axis=0)

    over = np.maximum(0.0, walk(0, w) - np.asarray(promised).astype(np.float64).reshape(HOLDINGS)[hidx] / 2.0)
    den = float(w.sum()) * len(hidx)
    return float(over.sum()) / den if den else float("nan")
