"""The locked-node definition restated in numpy int64 (TEST INFRASTRUCTURE): include/pokerl_hip.h "Locked nodes" / DESIGN.md section 3.15.
river_solver_spec / turn_solver_spec are imported, not edited: pairwise, strategy_from, tree_pass and spot_of are theirs.  A locked solve
differs from their solve_spot in three places: sigma of a locked row comes from strategy_from(locked), the R / A update is skipped there,
and the final sigma at a locked row is taken from the same source.  br is the ordinary best-response pass: it ignores the locks."""
import numpy as np

import river_solver_spec as RS
import turn_solver_spec as TS

HOLDINGS, ONE = RS.HOLDINGS, RS.ONE


def _flags(lock, D):
    return np.zeros(D, bool) if lock is None else np.asarray(lock).reshape(-1)[:D] != 0


def solve_river_spot(board, ranges, tree, iters, lock=None, locked=None, dead=0):
    """One river spot.  lock: [>= D] flags (None: nothing locked), locked: integers [>= D, 4, 1326] -> river_solver_spec.solve_spot's dict."""
    T = RS.as_tree(tree)
    D = len(T.decisions)
    out = dict(strategy=np.zeros((D, 4, HOLDINGS), np.uint16), value=np.zeros((2, HOLDINGS), np.int64), br=np.zeros((2, HOLDINGS), np.int64),
               valid=np.zeros(HOLDINGS, bool))
    status, gone = RS.check_spot(board, dead)
    if 52 - len(gone) < 4:
        status |= RS.SMALL_POOL
    out["status"] = status
    if status:
        return out
    hidx, beats, ties, loses = RS.pairwise(board, gone)
    M = (beats, ties, loses)
    w = np.asarray(ranges, np.int64).reshape(2, HOLDINGS)[:, hidx]
    root = (w[0] << 4, w[1] << 4)
    n = len(hidx)
    flags = _flags(lock, D)
    fixed = {d: RS.strategy_from(np.asarray(locked)[row, :len(T.child[d])][:, hidx].astype(np.int64))
             for row, d in enumerate(T.decisions) if flags[row]}
    R = {d: np.zeros((len(T.child[d]), n), np.int64) for d in T.decisions}
    A = {d: np.zeros((len(T.child[d]), n), np.int64) for d in T.decisions}
    for t in range(1, int(iters) + 1):
        sigma = {d: fixed[d] if d in fixed else RS.strategy_from(R[d]) for d in T.decisions}
        r, u = RS.tree_pass(T, M, root, sigma)
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
    _, u = RS.tree_pass(T, M, root, sigma)
    for p in (0, 1):
        out["value"][p, hidx] = u[p][0]
        out["br"][p, hidx] = RS.tree_pass(T, M, root, sigma, best=p)[1][p][0]
    out["valid"][hidx] = True
    return out


def solve_turn_spot(board, ranges, tree, iters, lock=None, locked=None, river_lock=None, river_locked=None, dead=0):
    """One turn spot.  lock / locked: the turn-level rows; river_lock [>= D_r] / river_locked [>= D_r, 52, 4, 1326]: the river-level rows
    -> turn_solver_spec.solve_spot's dict."""
    T = TS.as_tree(tree)
    Dt, Dr = len(T.turn_decisions), len(T.river_decisions)
    out = dict(strategy=np.zeros((Dt, 4, HOLDINGS), np.uint16), river_strategy=np.zeros((Dr, 52, 4, HOLDINGS), np.uint16),
               value=np.zeros((2, HOLDINGS), np.int64), br=np.zeros((2, HOLDINGS), np.int64), valid=np.zeros(HOLDINGS, bool), P=0)
    status, gone = TS.check_spot(board, dead)
    out["status"] = status
    if status:
        return out
    sp = TS.spot_of(board, gone)
    out["P"] = sp.P
    nT = len(sp.hidx)
    w = np.asarray(ranges, np.int64).reshape(2, HOLDINGS)[:, sp.hidx]
    root = (w[0] << 1, w[1] << 1)
    tf, rf = _flags(lock, Dt), _flags(river_lock, Dr)
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
    _, u = TS.tree_pass(T, sp, root, sigma)
    for p in (0, 1):
        out["value"][p, sp.hidx] = u[p][0]
        out["br"][p, sp.hidx] = TS.tree_pass(T, sp, root, sigma, best=p)[1][p][0]
    out["valid"][sp.hidx] = True
    return out


def _pad(a, rows):
    """a [D, ...] -> [rows, ...], zeros behind (the call's row stride)"""
    out = np.zeros((rows,) + a.shape[1:], a.dtype)
    out[:a.shape[0]] = a
    return out


def solve_river_batch(board, ranges, trees, tree_of, iters, lock=None, locked=None, dead=None):
    """A call: trees a list, tree_of [m] (an index >= len(trees): status BAD_TREE, zeros), lock [m, Dmax] / locked [m, Dmax, 4, 1326] or
    None -> dict of stacked arrays with the call's row stride Dmax."""
    Dmax = max(len(RS.as_tree(t).decisions) for t in trees)
    res = []
    for i in range(len(board)):
        k = int(tree_of[i])
        spot = solve_river_spot([int(x) for x in board[i]], ranges[i], trees[min(k, len(trees) - 1)], iters, None if lock is None else lock[i],
                                None if locked is None else locked[i], 0 if dead is None else int(dead[i]))
        if k >= len(trees):
            for key in ("strategy", "value", "br", "valid"):
                spot[key] = np.zeros_like(spot[key])
            spot["status"] |= 32
        spot["strategy"] = _pad(spot["strategy"], Dmax)
        res.append(spot)
    out = {k: np.stack([np.asarray(r[k]) for r in res]) for k in ("strategy", "value", "br", "status", "valid")}
    out["status"] = out["status"].astype(np.uint8)
    return out


def solve_turn_batch(board, ranges, trees, tree_of, iters, lock=None, locked=None, river_lock=None, river_locked=None, dead=None):
    """As solve_river_batch, with both levels' strides."""
    Dt = max(len(TS.as_tree(t).turn_decisions) for t in trees)
    Dr = max(len(TS.as_tree(t).river_decisions) for t in trees)
    res = []
    for i in range(len(board)):
        k = int(tree_of[i])
        pick = lambda x: None if x is None else x[i]
        spot = solve_turn_spot([int(x) for x in board[i]], ranges[i], trees[min(k, len(trees) - 1)], iters, pick(lock), pick(locked), pick(river_lock),
                               pick(river_locked), 0 if dead is None else int(dead[i]))
        if k >= len(trees):
            for key in ("strategy", "river_strategy", "value", "br", "valid"):
                spot[key] = np.zeros_like(spot[key])
            spot["status"] |= 32
            spot["P"] = 0
        spot["strategy"], spot["river_strategy"] = _pad(spot["strategy"], Dt), _pad(spot["river_strategy"], Dr)
        res.append(spot)
    out = {k: np.stack([np.asarray(r[k]) for r in res]) for k in ("strategy", "river_strategy", "value", "br", "status", "valid", "P")}
    out["status"] = out["status"].astype(np.uint8)
    return out


def gap(ranges, value, br, p):
    """sum_h w_p[h] (br_p[h] - value_p[h]): player p's unnormalised gap, a Python integer"""
    w = np.asarray(ranges).reshape(2, HOLDINGS)
    return sum(int(a) * (int(b) - int(c)) for a, b, c in zip(w[p], br[p], value[p]))
