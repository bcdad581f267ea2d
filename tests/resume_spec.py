"""The resuming definition restated in numpy int64 (TEST INFRASTRUCTURE): include/pokerl_hip.h "Resuming a solve" / DESIGN.md section 3.17.
resolve_spec (and through it the other restatements) is imported, not edited.  solve_river_spot and solve_turn_spot differ from resolve_spec's in what the
definition says and in nothing else: R and A start from the caller's state, clamped, where t0 > 0; iteration j of the call is number
t0 + j; and the state comes back -- R and A at the entries that are read, zeros (t0 = 0) or the caller's own bytes (t0 > 0) at every other
entry, the caller's own bytes everywhere for a refused spot."""
import numpy as np

import resolve_spec as RZ
import river_solver_spec as RS
import solver_lock_spec as LS
import turn_solver_spec as TS

HOLDINGS = RS.HOLDINGS
BAD_ITER, MAX_ITERS = 16, 4096
RIVER_RMAX, RIVER_AMAX = (1 << 58) - 1, (1 << 44) - 1
TURN_RMAX, TURN_AMAX = (1 << 60) - 1, (1 << 41) - 1
STATE_KEYS = ("regret", "average")
TURN_STATE_KEYS = ("regret", "average", "river_regret", "river_average")


def solve_river_spot(board, ranges, tree, iters, lock=None, locked=None, dead=0, reach=None, given=None, at=None, t0=0, regret=None, average=None):
    """One river spot of pk_solve_river_resume -> resolve_spec's dict plus regret / average int64 [rows, 4, 1326] (rows: those of the arrays
    passed, at least the tree's D; None passed: D rows of zeros, which only t0 = 0 makes sense with) and t (t0 + iters, 0 for a refused spot)."""
    T = RS.as_tree(tree)
    D = len(T.decisions)
    t0, iters = int(t0), int(iters)
    state = [np.zeros((D, 4, HOLDINGS), np.int64) if x is None else np.array(x, np.int64) for x in (regret, average)]
    out = dict(strategy=np.zeros((D, 4, HOLDINGS), np.uint16), value=np.zeros((2, HOLDINGS), np.int64), br=np.zeros((2, HOLDINGS), np.int64),
               valid=np.zeros(HOLDINGS, bool), regret=state[0], average=state[1], t=0)
    RZ._empty_nodes(out)
    status, gone = RS.check_spot(board, dead)
    if 52 - len(gone) < 4:
        status |= RS.SMALL_POOL
    if not status and at is not None and int(at) >= T.n:
        status |= RZ.BAD_TREE
    if not status and t0 + iters > MAX_ITERS:
        status |= BAD_ITER
    out["status"] = status
    if status:
        return out                                   # (the state: the caller's own bytes)
    hidx, beats, ties, loses = RS.pairwise(board, gone)
    M = (beats, ties, loses)
    root = RZ._root(ranges, reach, hidx, 4, RZ.RIVER_LIM)
    g = None
    if RZ.GIVEN in T.kind:
        g = np.clip(np.asarray(given).astype(np.int64).reshape(2, HOLDINGS)[:, hidx], -RZ.GIVEN_LIM, RZ.GIVEN_LIM)
    n = len(hidx)
    flags = LS._flags(lock, D)
    fixed = {d: RS.strategy_from(np.asarray(locked)[row, :len(T.child[d])][:, hidx].astype(np.int64))
             for row, d in enumerate(T.decisions) if flags[row]}
    R = {d: np.zeros((len(T.child[d]), n), np.int64) for d in T.decisions}
    A = {d: np.zeros((len(T.child[d]), n), np.int64) for d in T.decisions}
    if t0 > 0:
        for row, d in enumerate(T.decisions):
            if d not in fixed:
                R[d] = np.clip(state[0][row, :len(T.child[d])][:, hidx], 0, RIVER_RMAX)
                A[d] = np.clip(state[1][row, :len(T.child[d])][:, hidx], 0, RIVER_AMAX)
    for t in range(t0 + 1, t0 + iters + 1):
        sigma = {d: fixed[d] if d in fixed else RS.strategy_from(R[d]) for d in T.decisions}
        r, u = RZ.river_pass(T, M, root, sigma, g)
        for d in T.decisions:
            if d in fixed:
                continue
            p = T.kind[d]
            for a, c in enumerate(T.child[d]):
                R[d][a] = np.maximum(0, R[d][a] + u[p][c] - u[p][d])
                A[d][a] += t * r[p][c]
    if t0 == 0:
        state[0][:], state[1][:] = 0, 0
    for row, d in enumerate(T.decisions):
        if d not in fixed:
            for a in range(len(T.child[d])):
                state[0][row, a, hidx], state[1][row, a, hidx] = R[d][a], A[d][a]
    out["t"] = t0 + iters
    sigma = {d: fixed[d] if d in fixed else RS.strategy_from(A[d]) for d in T.decisions}
    for row, d in enumerate(T.decisions):
        out["strategy"][row, :len(T.child[d]), hidx] = sigma[d].T
    r, u = RZ.river_pass(T, M, root, sigma, g)
    for p in (0, 1):
        ub = RZ.river_pass(T, M, root, sigma, g, best=p)[1][p]
        out["value"][p, hidx] = u[p][0]
        out["br"][p, hidx] = ub[0]
        if at is not None:
            out["node_reach"][p, hidx] = r[p][int(at)]
            out["node_value"][p, hidx] = u[p][int(at)]
            out["node_br"][p, hidx] = ub[int(at)]
    out["valid"][hidx] = True
    return out


def solve_river_batch(board, ranges, trees, tree_of, iters, lock=None, locked=None, dead=None, reach=None, given=None, at=None, t0=None, regret=None,
                      average=None):
    """A call: as resolve_spec.solve_river_batch, with t0 [m] or None and regret / average [m, Dmax, 4, 1326] or None (both: zeros, which come
    back as the state of a fresh solve).  The arrays passed are not changed: the dict holds the state after the call."""
    Dmax = max(len(RS.as_tree(t).decisions) for t in trees)
    m = len(board)
    if regret is None:
        regret, average = np.zeros((m, Dmax, 4, HOLDINGS), np.int64), np.zeros((m, Dmax, 4, HOLDINGS), np.int64)
    res = []
    pick = RZ._pick
    for i in range(m):
        k = 0 if tree_of is None else int(tree_of[i])
        spot = solve_river_spot([int(x) for x in board[i]], pick(ranges, i), trees[min(k, len(trees) - 1)], iters, pick(lock, i), pick(locked, i),
                                0 if dead is None else int(dead[i]), pick(reach, i), pick(given, i), pick(at, i), 0 if t0 is None else int(t0[i]),
                                regret[i], average[i])
        if k >= len(trees):
            # (the tree is judged first: a spot whose tree does not exist reports that alone, and its state is the caller's own bytes)
            spot["status"] &= ~(RZ.BAD_TREE | BAD_ITER)
            RZ._refuse(spot, ("strategy", "value", "br", "valid") + RZ.NODE_KEYS)
            spot["regret"], spot["average"], spot["t"] = np.array(regret[i], np.int64), np.array(average[i], np.int64), 0
        spot["strategy"] = LS._pad(spot["strategy"], Dmax)
        res.append(spot)
    out = {k: np.stack([np.asarray(r[k]) for r in res]) for k in ("strategy", "value", "br", "status", "valid", "t") + RZ.NODE_KEYS + STATE_KEYS}
    out["status"], out["t"] = out["status"].astype(np.uint8), out["t"].astype(np.uint32)
    return out


def solve_turn_spot(board, ranges, tree, iters, lock=None, locked=None, river_lock=None, river_locked=None, dead=0, reach=None, at=None, at_card=None, t0=0,
                    regret=None, average=None, river_regret=None, river_average=None):
    """One turn spot of pk_solve_turn_resume -> resolve_spec's dict plus regret / average int64 [rows, 4, 1326], river_regret / river_average
    int64 [rows, 52, 4, 1326] and t, as solve_river_spot."""
    T = TS.as_tree(tree)
    Dt, Dr = len(T.turn_decisions), len(T.river_decisions)
    t0, iters = int(t0), int(iters)
    shapes = ((Dt, 4, HOLDINGS), (Dt, 4, HOLDINGS), (Dr, 52, 4, HOLDINGS), (Dr, 52, 4, HOLDINGS))
    state = [np.zeros(sh, np.int64) if x is None else np.array(x, np.int64) for x, sh in zip((regret, average, river_regret, river_average), shapes)]
    out = dict(strategy=np.zeros((Dt, 4, HOLDINGS), np.uint16), river_strategy=np.zeros((Dr, 52, 4, HOLDINGS), np.uint16),
               value=np.zeros((2, HOLDINGS), np.int64), br=np.zeros((2, HOLDINGS), np.int64), valid=np.zeros(HOLDINGS, bool), P=0, t=0,
               regret=state[0], average=state[1], river_regret=state[2], river_average=state[3])
    RZ._empty_nodes(out)
    status, gone = TS.check_spot(board, dead)
    card = None
    if not status and at is not None:
        if int(at) >= T.n:
            status |= RZ.BAD_TREE
        elif T.river[int(at)]:
            card = None if at_card is None else RZ.canon_of(at_card)
            if card is None or card in gone:
                status |= RZ.BAD_CARD
    if not status and t0 + iters > MAX_ITERS:
        status |= BAD_ITER
    out["status"] = status
    if status:
        return out                                   # (the state: the caller's own bytes)
    sp = TS.spot_of(board, gone)
    out["P"] = sp.P
    nT = len(sp.hidx)
    root = RZ._root(ranges, reach, sp.hidx, 1, RZ.TURN_LIM)
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
    if t0 > 0:
        for row, d in enumerate(T.turn_decisions):
            if d not in fixed:
                R[d] = np.clip(state[0][row, :len(T.child[d])][:, sp.hidx], 0, TURN_RMAX)
                A[d] = np.clip(state[1][row, :len(T.child[d])][:, sp.hidx], 0, TURN_AMAX)
        for row, d in enumerate(T.river_decisions):
            if d not in fixed:
                R[d] = [np.clip(state[2][row, k, :len(T.child[d])][:, sp.hidx[idx]], 0, TURN_RMAX) for k, idx, _ in sp.river]
                A[d] = [np.clip(state[3][row, k, :len(T.child[d])][:, sp.hidx[idx]], 0, TURN_AMAX) for k, idx, _ in sp.river]
    for t in range(t0 + 1, t0 + iters + 1):
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
    if t0 == 0:
        for x in state:
            x[:] = 0
    for row, d in enumerate(T.turn_decisions):
        if d not in fixed:
            for a in range(len(T.child[d])):
                state[0][row, a, sp.hidx], state[1][row, a, sp.hidx] = R[d][a], A[d][a]
    for row, d in enumerate(T.river_decisions):
        if d not in fixed:
            for j, (k, idx, _) in enumerate(sp.river):
                for a in range(len(T.child[d])):
                    state[2][row, k, a, sp.hidx[idx]], state[3][row, k, a, sp.hidx[idx]] = R[d][j][a], A[d][j][a]
    out["t"] = t0 + iters
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


def solve_turn_batch(board, ranges, trees, tree_of, iters, lock=None, locked=None, river_lock=None, river_locked=None, dead=None, reach=None, at=None,
                     at_card=None, t0=None, regret=None, average=None, river_regret=None, river_average=None):
    """As solve_river_batch, with both levels' strides and state arrays."""
    Dt = max(len(TS.as_tree(t).turn_decisions) for t in trees)
    Dr = max(len(TS.as_tree(t).river_decisions) for t in trees)
    m = len(board)
    if regret is None:
        regret, average = np.zeros((m, Dt, 4, HOLDINGS), np.int64), np.zeros((m, Dt, 4, HOLDINGS), np.int64)
        river_regret, river_average = np.zeros((m, Dr, 52, 4, HOLDINGS), np.int64), np.zeros((m, Dr, 52, 4, HOLDINGS), np.int64)
    res = []
    pick = RZ._pick
    for i in range(m):
        k = 0 if tree_of is None else int(tree_of[i])
        own = (regret[i], average[i], river_regret[i], river_average[i])
        if k >= len(trees):
            # (no tree: neither the node nor the iterations are judged; the state is the caller's own bytes)
            spot = solve_turn_spot([int(x) for x in board[i]], pick(ranges, i), trees[0], 0, dead=0 if dead is None else int(dead[i]), reach=pick(reach, i))
            RZ._refuse(spot, ("strategy", "river_strategy", "value", "br", "valid") + RZ.NODE_KEYS)
            spot["P"], spot["t"] = 0, 0
            for key, x in zip(TURN_STATE_KEYS, own):
                spot[key] = np.array(x, np.int64)
        else:
            spot = solve_turn_spot([int(x) for x in board[i]], pick(ranges, i), trees[k], iters, pick(lock, i), pick(locked, i), pick(river_lock, i),
                                   pick(river_locked, i), 0 if dead is None else int(dead[i]), pick(reach, i), pick(at, i), pick(at_card, i),
                                   0 if t0 is None else int(t0[i]), *own)
        spot["strategy"], spot["river_strategy"] = LS._pad(spot["strategy"], Dt), LS._pad(spot["river_strategy"], Dr)
        res.append(spot)
    out = {k: np.stack([np.asarray(r[k]) for r in res]) for k in ("strategy", "river_strategy", "value", "br", "status", "valid", "P", "t") + RZ.NODE_KEYS + TURN_STATE_KEYS}
    out["status"], out["t"] = out["status"].astype(np.uint8), out["t"].astype(np.uint32)
    return out
