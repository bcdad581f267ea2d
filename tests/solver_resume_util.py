"""What the resuming tests share (TEST INFRASTRUCTURE): pk_solve_river_resume / pk_solve_turn_resume called as they are on host arrays, state filled with a
sentinel, and the mask of the state entries the definition says are read.  Nothing here comes from a kernel."""
import numpy as np

import river_solver_spec as RS
import rvr_spec as VS
import solver_resolve_util as RU

H = 1326
SENTINEL = 0x5A5A5A5A5A5A5A5A                # a state entry that must not be read, or must survive: positive, beyond both clamps
RIVER_KEYS = RU.RIVER_KEYS + ("regret", "average")
TURN_KEYS = RU.TURN_KEYS + ("regret", "average", "river_regret", "river_average")
_c = RU._c


def river_call(S, board, dead, trees, tree_of, iters, ranges=None, reach=None, given=None, at=None, lock=None, locked=None, t0=None, regret=None,
               average=None):
    """pk_solve_river_resume on host arrays, nothing checked on the way -> dict of RIVER_KEYS; regret / average are copied first, the copies
    worked in place and returned (both None: the resolve call inside the library, no state in the dict)"""
    from pokerl_amd import _lib as L
    rows = S._TreeRows(trees, 64)
    m, D = len(board), max(len(t.decision_nodes) for t in rows.trees)
    board, dead, ranges, reach, given = _c(board, np.uint8), _c(dead, np.uint64), _c(ranges, np.uint16), _c(reach, np.uint32), _c(given, np.int64)
    tree_of, at, lock, locked, t0 = _c(tree_of, np.uint32), _c(at, np.uint8), _c(lock, np.uint8), _c(locked, np.uint16), _c(t0, np.uint32)
    out = dict(strategy=np.zeros((m, D, 4, H), np.uint16), value=np.zeros((m, 2, H), np.int64), br=np.zeros((m, 2, H), np.int64),
               node_reach=np.zeros((m, 2, H), np.uint32), node_value=np.zeros((m, 2, H), np.int64), node_br=np.zeros((m, 2, H), np.int64), status=np.zeros(m, np.uint8))
    if regret is not None:
        out["regret"], out["average"] = np.array(regret, np.int64, order="C"), np.array(average, np.int64, order="C")
        assert out["regret"].shape == (m, D, 4, H) == out["average"].shape
    no = [L.ptr(out[k]) if at is not None else None for k in ("node_reach", "node_value", "node_br")]
    L.check(L.lib().pk_solve_river_resume(0, m, L.ptr(board), L.ptr(dead), L.ptr(ranges), *rows.args(), L.ptr(tree_of), int(iters), L.ptr(lock), L.ptr(locked),
                                          L.ptr(reach), L.ptr(given), L.ptr(at), L.ptr(t0), L.ptr(out.get("regret")), L.ptr(out.get("average")),
                                          L.ptr(out["strategy"]), L.ptr(out["value"]), L.ptr(out["br"]), *no, L.ptr(out["status"])))
    return out


def sentinel_state(m, D):
    return np.full((m, D, 4, H), SENTINEL, np.int64), np.full((m, D, 4, H), SENTINEL, np.int64)


def river_read_mask(board, dead, trees, tree_of, lock=None):
    """bool [m, Dmax, 4, 1326]: the state entries of a SOLVED spot that the definition reads and writes -- a row of the spot's own tree that is
    not locked, an action of its node, a holding of the pool.  All False for a spot refused by its cards or its tree_of."""
    m = len(board)
    D = max(len(t.decision_nodes) for t in trees)
    mask = np.zeros((m, D, 4, H), bool)
    for i in range(m):
        k = 0 if tree_of is None else int(tree_of[i])
        status, _ = RS.check_spot([int(c) for c in board[i]], int(dead[i]))
        if status or k >= len(trees):
            continue
        valid = ~RU.invalid_holdings(board[i], 5, dead[i])
        for row, v in enumerate(trees[k].decision_nodes):
            if lock is not None and lock[i][row]:
                continue
            mask[i, row, :trees[k].num_actions(v)] = valid
    return mask


def turn_call(S, board, dead, trees, tree_of, iters, ranges=None, reach=None, at=None, at_card=None, lock=None, locked=None, river_lock=None, river_locked=None,
              t0=None, state=None, river_strategy=True):
    """pk_solve_turn_resume on host arrays -> dict of TURN_KEYS; state: (regret, average, river_regret, river_average), copied first, the copies
    worked in place and returned (None: the resolve call inside the library, no state in the dict)"""
    from pokerl_amd import _lib as L
    rows = S._TreeRows(trees, 128)
    m = len(board)
    Dt, Dr = max(len(t.decision_nodes) for t in rows.trees), max(len(t.river_decision_nodes) for t in rows.trees)
    board, dead, ranges, reach = _c(board, np.uint8), _c(dead, np.uint64), _c(ranges, np.uint16), _c(reach, np.uint32)
    tree_of, at, at_card, t0 = _c(tree_of, np.uint32), _c(at, np.uint8), _c(at_card, np.uint8), _c(t0, np.uint32)
    lock, locked, river_lock, river_locked = _c(lock, np.uint8), _c(locked, np.uint16), _c(river_lock, np.uint8), _c(river_locked, np.uint16)
    out = dict(strategy=np.zeros((m, Dt, 4, H), np.uint16), river_strategy=np.zeros((m, Dr, 52, 4, H), np.uint16) if river_strategy else None,
               value=np.zeros((m, 2, H), np.int64), br=np.zeros((m, 2, H), np.int64), node_reach=np.zeros((m, 2, H), np.uint32),
               node_value=np.zeros((m, 2, H), np.int64), node_br=np.zeros((m, 2, H), np.int64), status=np.zeros(m, np.uint8))
    keys = ("regret", "average", "river_regret", "river_average")
    if state is not None:
        for k, a, shape in zip(keys, state, [(m, Dt, 4, H)] * 2 + [(m, Dr, 52, 4, H)] * 2):
            out[k] = np.array(a, np.int64, order="C")
            assert out[k].shape == shape
    no = [L.ptr(out[k]) if at is not None else None for k in ("node_reach", "node_value", "node_br")]
    L.check(L.lib().pk_solve_turn_resume(0, m, L.ptr(board), L.ptr(dead), L.ptr(ranges), *rows.args(), L.ptr(tree_of), int(iters), L.ptr(lock), L.ptr(locked),
                                         L.ptr(river_lock), L.ptr(river_locked), L.ptr(reach), L.ptr(at), L.ptr(at_card), L.ptr(t0), *[L.ptr(out.get(k)) for k in keys],
                                         L.ptr(out["strategy"]), L.ptr(out["river_strategy"]), L.ptr(out["value"]), L.ptr(out["br"]), *no, L.ptr(out["status"])))
    return out


def turn_sentinel_state(m, Dt, Dr):
    return tuple(np.full(sh, SENTINEL, np.int64) for sh in [(m, Dt, 4, H)] * 2 + [(m, Dr, 52, 4, H)] * 2)


def turn_read_masks(board, dead, trees, tree_of, lock=None, river_lock=None):
    """(bool [m, Dtmax, 4, 1326], bool [m, Drmax, 52, 4, 1326]): the state entries of a SOLVED spot that are read and written: at the river
    level the cards of the pool and the pool's holdings without the card.  All False for a spot refused by its cards or its tree_of."""
    m = len(board)
    Dt, Dr = max(len(t.decision_nodes) for t in trees), max(len(t.river_decision_nodes) for t in trees)
    tm, rm = np.zeros((m, Dt, 4, H), bool), np.zeros((m, Dr, 52, 4, H), bool)
    for i in range(m):
        k = 0 if tree_of is None else int(tree_of[i])
        pool = RU.pool_of(board[i], 4, dead[i])
        if len(pool) < 5 or k >= len(trees):
            continue
        valid = ~RU.invalid_holdings(board[i], 4, dead[i])
        for row, v in enumerate(trees[k].decision_nodes):
            if lock is None or not lock[i][row]:
                tm[i, row, :trees[k].num_actions(v)] = valid
        for row, v in enumerate(trees[k].river_decision_nodes):
            if river_lock is None or not river_lock[i][row]:
                for c in pool:
                    rm[i, row, c, :trees[k].num_actions(v)] = valid & (VS.PAIR_A != c) & (VS.PAIR_B != c)
    return tm, rm
