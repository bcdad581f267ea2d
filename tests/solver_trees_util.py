"""What the tree-per-spot solver calls (pk_solve_river_trees / pk_solve_turn_trees) must return, assembled from the
numpy specs ONE SPOT AT A TIME: spot i is river_solver_spec.solve_spot / turn_solver_spec.solve_spot with tree trees[tree_of[i]], laid out
with the call's row strides (the most decision nodes of ANY tree passed), rows at or past the spot's own count 0; a spot whose tree_of
names no tree reports BAD_TREE beside whatever its cards report, and is all zeros.  Nothing here comes from a kernel.  Also the hand-made
trees the host, CPU-build and GPU tests share."""
import numpy as np

import river_solver_spec as RS
import turn_solver_spec as TS

H = RS.HOLDINGS
BAD_TREE = 32
FF = 0xFF


def river_expect(board, ranges, trees, tree_of, iters, dead=None):
    """-> dict(strategy uint16 [m, Dmax, 4, 1326], value, br int64 [m, 2, 1326], status uint8 [m], valid bool [m, 1326])"""
    m = len(board)
    Dmax = max(len(t.decision_nodes) for t in trees)
    out = dict(strategy=np.zeros((m, Dmax, 4, H), np.uint16), value=np.zeros((m, 2, H), np.int64), br=np.zeros((m, 2, H), np.int64),
               status=np.zeros(m, np.uint8), valid=np.zeros((m, H), bool))
    for i in range(m):
        d = 0 if dead is None else int(dead[i])
        k = int(tree_of[i])
        if k >= len(trees):                                                   # what the cards report (no tree is needed for that), and BAD_TREE
            out["status"][i] = RS.solve_spot([int(x) for x in board[i]], ranges[i], forced_river_tree(), 1, d)["status"] | BAD_TREE
            continue
        r = RS.solve_spot([int(x) for x in board[i]], ranges[i], trees[k], iters, d)
        D = r["strategy"].shape[0]
        out["strategy"][i, :D], out["value"][i], out["br"][i], out["status"][i], out["valid"][i] = r["strategy"], r["value"], r["br"], r["status"], r["valid"]
    return out


def turn_expect(board, ranges, trees, tree_of, iters, dead=None):
    """-> dict(strategy uint16 [m, Dtmax, 4, 1326], river_strategy uint16 [m, Drmax, 52, 4, 1326], value, br, status, valid, P [m])"""
    m = len(board)
    Dt, Dr = max(len(t.decision_nodes) for t in trees), max(len(t.river_decision_nodes) for t in trees)
    out = dict(strategy=np.zeros((m, Dt, 4, H), np.uint16), river_strategy=np.zeros((m, Dr, 52, 4, H), np.uint16), value=np.zeros((m, 2, H), np.int64),
               br=np.zeros((m, 2, H), np.int64), status=np.zeros(m, np.uint8), valid=np.zeros((m, H), bool), P=np.zeros(m, np.int64))
    for i in range(m):
        d = 0 if dead is None else int(dead[i])
        k = int(tree_of[i])
        if k >= len(trees):
            out["status"][i] = TS.check_spot([int(x) for x in board[i]], d)[0] | BAD_TREE
            continue
        r = TS.solve_spot([int(x) for x in board[i]], ranges[i], trees[k], iters, d)
        a, b = r["strategy"].shape[0], r["river_strategy"].shape[0]
        out["strategy"][i, :a], out["river_strategy"][i, :b] = r["strategy"], r["river_strategy"]
        out["value"][i], out["br"][i], out["status"][i], out["valid"][i], out["P"][i] = r["value"], r["br"], r["status"], r["valid"], r["P"]
    return out


def forced_river_tree():
    """three nodes: both players must check, then the showdown"""
    from pokerl_amd.solver import RiverTree
    return RiverTree([0, 1, 4], [[1, FF, FF, FF], [2, FF, FF, FF], [FF] * 4], [[0, 0]] * 3, 77)


def four_action_river_tree():
    """eleven nodes: a four-action root (check to showdown, three bet sizes), fold or call behind each bet"""
    from pokerl_amd.solver import RiverTree
    return RiverTree([0, 4, 1, 1, 1, 3, 4, 3, 4, 3, 4], [[1, 2, 3, 4], [FF] * 4, [5, 6, FF, FF], [7, 8, FF, FF], [9, 10, FF, FF]] + [[FF] * 4] * 6,
                     [[0, 0], [0, 0], [50, 0], [100, 0], [200, 0], [50, 0], [50, 50], [100, 0], [100, 100], [200, 0], [200, 200]], 100)


def chain_river_tree(pot=60):
    """sixty-four nodes, the most a tree may have: a forced first node, then 31 decisions in turn, each a fold or a raise of 10 on top of
    the call; the last one folds or calls"""
    from pokerl_amd.solver import RiverTree
    kind, child, put = [0, 1], [[1], []], [[0, 0], [0, 0]]
    node, p, puts = 1, 1, [0, 0]
    for d in range(31):
        fold, nxt = len(kind), len(kind) + 1
        child[node] = [fold, nxt]
        kind.append(2 + p); child.append([]); put.append(list(puts))
        puts = list(puts)
        puts[p] = max(puts) if d == 30 else max(puts) + 10
        kind.append(4 if d == 30 else 1 - p); child.append([]); put.append(list(puts))
        node, p = nxt, 1 - p
    assert len(kind) == 64
    return RiverTree(kind, [list(c) + [FF] * (4 - len(c)) for c in child], put, pot)


def allin_turn_tree():
    """A hand-made turn tree with an all-in chance -> showdown, ten nodes, three turn-level and two river-level decisions: player 0 checks
    or shoves 40; behind the check player 1 must check, the river card comes and both must check again; behind the shove player 1 folds or
    calls, and the call leads through a chance node straight to the showdown"""
    from pokerl_amd.solver import TurnTree
    nodes = [(0, [1, 2], (0, 0)),          # 0: player 0 checks / shoves 40
             (1, [3], (0, 0)),             # 1: player 1 must check
             (1, [4, 5], (40, 0)),         # 2: player 1 folds / calls
             (5, [6], (0, 0)),             # 3: chance after check-check
             (3, [], (40, 0)),             # 4: player 1 has folded
             (5, [7], (40, 40)),           # 5: chance, all in
             (0, [8], (0, 0)),             # 6: river, player 0 must check
             (4, [], (40, 40)),            # 7: showdown, all in
             (1, [9], (0, 0)),             # 8: river, player 1 must check
             (4, [], (0, 0))]              # 9: showdown
    return TurnTree([k for k, _, _ in nodes], [ch + [FF] * (4 - len(ch)) for _, ch, _ in nodes], [list(p) for _, _, p in nodes], 30)
