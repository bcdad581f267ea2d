"""GPU tests of the turn solver's re-solving call (pk_solve_turn_resolve: include/pokerl_hip.h "Re-solving").
IDENTITIES with the pinned entry points, byte for byte: reach = ranges << 1 is the locked call; `at` = the root gives value, br and the
root reach; a turn-level subtree of a solution, locked to the solution's rows and started from node_reach, has node_value and node_br as
its value and br; a river-level node under a river card is the RIVER solver's call on the five-card board with river_subtree, locked to that
card's rows; the river-level values of all pool cards sum to the chance node's; what is not read is not read.  And the RESTATEMENT
(tests/resolve_spec.py), byte for byte: live at pools 5, 9 and 12 with `at` at every node kind, a refused spot, a bad tree_of, a bad `at`
and two bad at_card between valid ones, reaches above the limit, two trees in one call, one spot, a batch and more spots than the grid, the
stream form; by fixture at P = 48."""
import ctypes as C
import os

import numpy as np
import pytest

import resolve_spec as RZ
import river_solver_spec as RS
import rvr_spec as VS
import solver_lock_util as LU
import solver_resolve_util as RU
import solver_trees_util as U

pytestmark = pytest.mark.gpu

H = RS.HOLDINGS
KEYS = ("strategy", "river_strategy", "value", "br", "status", "valid")
OUT = RU.TURN_KEYS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


@pytest.fixture(scope="module")
def S():
    from pokerl_amd import solver
    return solver


def kind_node(tree, kind, river):
    return next(v for v in range(tree.n) if tree.kind[v] == kind and bool(tree.river_level[v]) == river)


@pytest.fixture(scope="module")
def solved(PK, S):
    """One P = 10 spot on turn_tree(100, 400, (1.0,), 1) and its 16-iteration solution with the river-level strategies -- shared by the
    identities, never changed"""
    rng = np.random.default_rng(0x3181)
    board, _, dead = VS.random_boards(rng, 1, 4, 10)
    board = np.ascontiguousarray(board[:, :4])
    ranges = LU.random_ranges(rng, 1)
    tree = PK.turn_tree(100, 400, (1.0,), 1)
    sol = S.solve_turn_batch(board, ranges, tree, 16, dead, river_strategy=True)
    assert sol.status[0] == 0 and sol.pool[0] == 10
    for a in (board, dead, ranges, sol.strategy, sol.river_strategy, sol.value, sol.br):
        a.setflags(write=False)
    return dict(board=board, dead=dead, ranges=ranges, tree=tree, sol=sol, pool=RU.pool_of(board[0], 4, dead[0]))


def evaluate_at(S, x, at, at_card=None):
    """the solution again, every row locked and no iteration, with the node outputs at (at, at_card) [m] -- the same bytes as the solve"""
    m = len(at)
    rep = lambda a: np.repeat(a, m, axis=0)
    r = S.solve_turn_batch(rep(x["board"]), rep(x["ranges"]), x["tree"], 0, rep(x["dead"]), lock=np.ones(4, bool), locked=x["sol"].strategy[0],
                           river_lock=np.ones(12, bool), river_locked=x["sol"].river_strategy[0], at=np.asarray(at), at_card=at_card)
    assert not r.status.any() and all(r.value[i].tobytes() == x["sol"].value[0].tobytes() and r.br[i].tobytes() == x["sol"].br[0].tobytes() for i in range(m))
    return r


def test_identity_1_reach_from_ranges_is_the_locked_call(PK, S):
    rng = np.random.default_rng(0x3182)
    pools = [7, 9, 8, 6]
    board, _, dead = VS.random_boards(rng, 4, 4, lambda i: pools[i])
    board = np.ascontiguousarray(board[:, :4])
    board[2, 3] = board[2, 1]                                                 # a refused spot
    ranges = LU.random_ranges(rng, 4)
    trees = [PK.turn_tree(30, 20, (1.0,), 1), U.allin_turn_tree()]
    tree_of = np.array([0, 1, 0, 2], np.uint32)                               # ... and a tree_of that names no tree
    lock = LU.lock_of(trees, tree_of, ["p1", "none", "all", "all"])
    locked = LU.random_weights(rng, (4,) + lock.shape[1:] + (4, H))
    want = S.solve_turn_batch(board, ranges, trees, 2, dead, river_strategy=True, tree_of=tree_of, lock=lock, locked=locked)
    got = S.solve_turn_batch(board, None, trees, 2, dead, river_strategy=True, tree_of=tree_of, lock=lock, locked=locked, reach=ranges.astype(np.uint32) << 1)
    LU.same_bytes(got, want, KEYS, "reach = ranges << 1")
    assert want.status.tolist() == [0, 0, RS.DUP_CARD, 32] and got.node_value is None
    assert got[0].ev == want[0].ev and got[0].exploitability == want[0].exploitability


def test_identity_2_at_the_root(S, solved):
    x = solved
    r = evaluate_at(S, x, [0])
    assert r.node_value.tobytes() == r.value.tobytes() and r.node_br.tobytes() == r.br.tobytes() and r.node_value.any()
    assert (r.node_reach == (x["ranges"].astype(np.uint32) << 1) * r.valid[:, None]).all()


def test_identity_4_every_turn_level_subtree_of_a_solution(S, solved):
    x = solved
    tree, sol = x["tree"], x["sol"]
    nodes = tree.decision_nodes
    m = len(nodes)
    rep = lambda a: np.repeat(a, m, axis=0)
    whole = evaluate_at(S, x, nodes)
    subs = [tree.subtree(n) for n in nodes]
    Dt, Dr = max(len(r) for _, r, _ in subs), max(len(r) for _, _, r in subs)
    locked, rlocked = np.full((m, Dt, 4, H), 0xFFFF, np.uint16), np.full((m, Dr, 52, 4, H), 0xFFFF, np.uint16)
    for i, (_, rows, rrows) in enumerate(subs):
        locked[i, :len(rows)], rlocked[i, :len(rrows)] = sol.strategy[0][rows], sol.river_strategy[0][rrows]
    sub = S.solve_turn_batch(rep(x["board"]), None, [t for t, _, _ in subs], 0, rep(x["dead"]), lock=np.ones((m, Dt), np.uint8), locked=locked,
                             river_lock=np.ones((m, Dr), np.uint8), river_locked=rlocked, reach=whole.node_reach, at=np.zeros(m, np.uint8))
    assert not sub.status.any()
    for i, n in enumerate(nodes):
        assert sub.value[i].tobytes() == whole.node_value[i].tobytes(), ("value", n)
        assert sub.br[i].tobytes() == whole.node_br[i].tobytes(), ("br", n)
        assert sub.node_reach[i].tobytes() == whole.node_reach[i].tobytes(), ("reach", n)
    assert whole.node_value[1:].any() and (whole.node_br >= whole.node_value).all()


def test_identity_5_the_turn_solution_into_the_river_solver(S, solved):
    x = solved
    tree, sol, pool = x["tree"], x["sol"], x["pool"]
    for node in (tree.river_decision_nodes[0], tree.river_decision_nodes[5]):
        cards = [pool[0], pool[len(pool) // 2], pool[-1]]                     # the first pool card, one between, the last
        codes = np.array([VS.CANON[k] for k in cards], np.uint8)
        turn = evaluate_at(S, x, [node] * 3, codes)
        sub, rows = tree.river_subtree(node)
        board5 = np.concatenate([np.repeat(x["board"], 3, axis=0), codes[:, None]], axis=1)
        locked = np.stack([sol.river_strategy[0][rows][:, k] for k in cards])
        river = S.solve_river_batch(board5, None, sub, 0, np.repeat(x["dead"], 3), lock=np.ones(len(rows), bool), locked=locked, reach=turn.node_reach)
        assert not river.status.any() and river.valid.sum(axis=1).tolist() == [36] * 3
        for i, k in enumerate(cards):
            assert river.value[i].tobytes() == turn.node_value[i].tobytes() and river.br[i].tobytes() == turn.node_br[i].tobytes(), (node, k)
            with_card = (VS.PAIR_A == k) | (VS.PAIR_B == k)
            assert not turn.node_reach[i][:, with_card].any() and not turn.node_value[i][:, with_card].any() and turn.node_value[i].any()


def test_identity_6_the_cards_sum_to_the_chance_node(S, solved):
    x = solved
    tree, pool = x["tree"], x["pool"]
    chances = [v for v in range(tree.n) if tree.kind[v] == 5]
    for chance in (chances[0], chances[-1]):                                  # (the last one leads to a showdown or a decision: either kind of child)
        child = int(tree.child[chance][0])
        per_card = evaluate_at(S, x, [child] * len(pool), np.array([VS.CANON[k] for k in pool], np.uint8))
        at_chance = evaluate_at(S, x, [chance], np.array([0xFF], np.uint8))
        assert (per_card.node_value.sum(axis=0) == at_chance.node_value[0]).all() and (per_card.node_br.sum(axis=0) == at_chance.node_br[0]).all()
        assert at_chance.node_value.any() and (at_chance.node_reach[0] == per_card.node_reach.max(axis=0)).all()


def test_identity_9_not_read_means_not_read(PK, S):
    rng = np.random.default_rng(0x3183)
    pools = [7, 8, 6]
    board, _, dead = VS.random_boards(rng, 3, 4, lambda i: pools[i])
    board = np.ascontiguousarray(board[:, :4])
    board[1, 3] = board[1, 0]                                                 # refused
    tree = PK.turn_tree(30, 20, (1.0,), 1)
    reach = rng.integers(0, RZ.TURN_LIM + 1, (3, 2, H)).astype(np.uint32)
    at = np.array([1, 0, kind_node(tree, 5, False)], np.uint8)                # turn-level nodes: at_card is not read
    a = RU.turn_call(S, board, dead, [tree], None, 2, ranges=np.zeros((3, 2, H), np.uint16), reach=reach, at=at, at_card=np.zeros(3, np.uint8))
    reach2 = reach.copy()
    for i in range(3):
        reach2[i][:, RU.invalid_holdings(board[i], 4, dead[i])] = 0xFFFFFFFF
    b = RU.turn_call(S, board, dead, [tree], None, 2, ranges=np.full((3, 2, H), 0xFFFF, np.uint16), reach=reach2, at=at, at_card=np.full(3, 0xFF, np.uint8))
    RU.assert_equal(b, a, "ones in every slot that is not read", OUT)
    c = RU.turn_call(S, board, dead, [tree], None, 2, ranges=None, reach=reach2, at=at, at_card=None)
    RU.assert_equal(c, a, "ranges and at_card NULL", OUT)
    assert a["status"].tolist() == [0, RS.DUP_CARD, 0] and a["node_value"][2].any()


# ------------------------------------------------------------------------------------------------ against the restatement
def spec_batch(x, iters, pick=None):
    y = x if pick is None else {k: (v[pick] if isinstance(v, np.ndarray) else v) for k, v in x.items() if k != "want"}
    return RZ.solve_turn_batch(y["board"], None, y["trees"], y["tree_of"], iters, y["lock"], y["locked"], y["rlock"], y["rlocked"], y["dead"], y["reach"], y["at"],
                               y["at_card"])


def device_batch(S, x, iters, pick=None, river_strategy=True):
    y = x if pick is None else {k: (v[pick] if isinstance(v, np.ndarray) else v) for k, v in x.items() if k != "want"}
    return RU.turn_call(S, y["board"], y["dead"], y["trees"], y["tree_of"], iters, reach=y["reach"], at=y["at"], at_card=y["at_card"], lock=y["lock"],
                        locked=y["locked"], river_lock=y["rlock"], river_locked=y["rlocked"], river_strategy=river_strategy)


@pytest.fixture(scope="module")
def patterns(PK):
    """Pools 5, 9 and 12 on a small tree and the all-in tree, `at` at every node kind of both levels under the first, the last and a middle
    pool card, reaches above the limit, a refused spot, a bad tree_of, a bad `at` and two bad at_card between them -- the spots, and what the
    restatement gives at 2 iterations: computed once, never changed"""
    rng = np.random.default_rng(0x3184)
    pools = [5, 9, 12, 7, 8, 7, 6, 8, 7, 9, 8]
    m = len(pools)
    board, _, dead = VS.random_boards(rng, m, 4, lambda i: pools[i])
    board = np.ascontiguousarray(board[:, :4])
    board[4, 2] = board[4, 0]                                                 # refused, between valid ones
    small, allin = PK.turn_tree(30, 20, (1.0,), 1), U.allin_turn_tree()
    trees = [small, allin]
    tree_of = np.array([0, 0, 0, 1, 0, 2, 0, 0, 0, 1, 0], np.uint32)          # spot 5: a tree_of that names no tree
    rdec, rshow, rfold = small.river_decision_nodes[1], kind_node(small, 4, True), kind_node(small, 2, True)
    at = np.array([rdec, kind_node(small, 5, False), rshow, allin.n - 1, 0, 0, small.n, rdec, rdec, kind_node(allin, 3, False), rfold], np.uint8)
    pool = [RU.pool_of(board[i], 4, dead[i]) for i in range(m)]
    code = lambda i, j: int(VS.CANON[pool[i][j]])
    at_card = np.array([code(0, 0), 0xFF, code(2, -1), code(3, 3), 0, 0, 0, 0x1D, int(board[8, 1]), 0xFF, code(10, 4)], np.uint8)
    #                     first      (chance)  last      between    (refused) (no tree) (bad at) no card  a board card  (a turn-level fold)
    reach = RU.random_reach(rng, board, 4, dead, RZ.TURN_LIM, over=(1, 2))
    reach[[4, 5, 6, 7, 8]] = 0xFFFFFFFF                                       # refused spots: never read
    lock, rlock = LU.lock_of(trees, tree_of, ["none", "p1", "none", "all", "all", "all", "all", "all", "all", "none", [0]]), \
        LU.lock_of(trees, tree_of, ["none", "none", "p0", "all", "all", "all", "all", "all", "all", "none", [1, 2]], river=True)
    locked, rlocked = LU.random_weights(rng, (m, lock.shape[1], 4, H)), LU.random_weights(rng, (m, rlock.shape[1], 52, 4, H))
    x = dict(board=board, dead=dead, trees=trees, tree_of=tree_of, at=at, at_card=at_card, reach=reach, lock=lock, locked=locked, rlock=rlock, rlocked=rlocked)
    x["want"] = spec_batch(x, 2)
    for v in x["want"].values():
        v.setflags(write=False)
    return x


def test_the_patterns_at_every_pool_equal_the_restatement(S, patterns):
    x = patterns
    got = device_batch(S, x, 2)
    RU.assert_equal(got, x["want"], "eleven spots", OUT)
    assert got["status"].tolist() == [0, 0, 0, 0, RS.DUP_CARD, 32, 32, RS.BAD_CARD, RS.BAD_CARD, 0, 0]
    for i in (0, 1, 2, 3, 9, 10):
        assert got["node_reach"][i].any() and got["node_value"][i].any(), i
    for i in (4, 5, 6, 7, 8):
        assert not any(got[k][i].any() for k in OUT[:-1]), i
    assert x["want"]["valid"][2].sum() == 66 and (got["node_reach"][2] != 0).any(axis=0).sum() <= 55      # P = 12: the holdings with the card are 0


@pytest.mark.parametrize("iters", [0, 3])
def test_other_iteration_counts(S, patterns, iters):
    pick = np.array([1, 0, 7, 3, 10])
    RU.assert_equal(device_batch(S, patterns, iters, pick), spec_batch(patterns, iters, pick), "%d iterations" % iters, OUT)


def test_one_spot_alone_and_more_spots_than_the_grid(S, patterns):
    x = patterns
    for i in (0, 3, 10):
        RU.assert_equal(device_batch(S, x, 2, np.array([i])), {k: v[i:i + 1] for k, v in x["want"].items()}, "spot %d alone" % i, OUT)
    idx = np.tile(np.array([0, 3, 4, 6, 7, 9, 10]), 38)
    grid = S.turn_grid(x["trees"])
    assert len(idx) > grid and all(idx[i] != idx[i + grid] for i in range(len(idx) - grid))
    keys = [k for k in OUT if k != "river_strategy"]                         # (half a megabyte per spot and row: not at this size)
    got = device_batch(S, x, 2, idx, river_strategy=False)
    RU.assert_equal(got, {k: x["want"][k][idx] for k in keys}, "266 spots", keys)


def test_the_device_form_on_a_callers_stream(S, patterns):
    from pokerl_amd import hipmem
    x = patterns
    pick = np.array([0, 2, 4, 7, 9, 10])
    y = {k: (v[pick] if isinstance(v, np.ndarray) else v) for k, v in x.items() if k != "want"}
    want = {k: v[pick] for k, v in x["want"].items()}
    m, Dt = len(pick), y["lock"].shape[1]
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    names = ("board", "dead", "tree_of", "lock", "locked", "rlock", "rlocked", "reach", "at", "at_card")
    ins = {k: hipmem.DeviceBuffer(y[k].nbytes).upload(np.ascontiguousarray(y[k])) for k in names}
    sizes = dict(strategy=(np.uint16, (m, Dt, 4, H)), value=(np.int64, (m, 2, H)), br=(np.int64, (m, 2, H)), node_reach=(np.uint32, (m, 2, H)),
                 node_value=(np.int64, (m, 2, H)), node_br=(np.int64, (m, 2, H)), status=(np.uint8, (m,)))
    outs = {k: hipmem.DeviceBuffer(int(np.prod(shape)) * np.dtype(dt).itemsize) for k, (dt, shape) in sizes.items()}
    S.solve_turn_d(m, ins["board"].ptr, None, y["trees"], 2, dead_d=ins["dead"].ptr, strategy_d=outs["strategy"].ptr, value_d=outs["value"].ptr,
                   br_d=outs["br"].ptr, status_d=outs["status"].ptr, stream=stream, tree_of=ins["tree_of"].ptr, lock=ins["lock"].ptr, locked=ins["locked"].ptr,
                   river_lock=ins["rlock"].ptr, river_locked=ins["rlocked"].ptr, reach=ins["reach"].ptr, at=ins["at"].ptr, at_card=ins["at_card"].ptr,
                   node_reach_d=outs["node_reach"].ptr, node_value_d=outs["node_value"].ptr, node_br_d=outs["node_br"].ptr)
    assert hip.hipStreamSynchronize(stream) == 0
    got = {k: outs[k].download(sizes[k][0], int(np.prod(sizes[k][1]))).reshape(sizes[k][1]) for k in sizes}
    RU.assert_equal(got, want, "the stream form", list(sizes))
    assert hip.hipStreamDestroy(stream) == 0
    for b in list(ins.values()) + list(outs.values()):
        b.free()


def test_the_p48_fixture(S):
    """P = 48 by fixture (tests/golden/resolve/make.py writes it from the restatement alone; the CPU build of the kernel checks the same
    fixture): a river-level node under a card from the middle of the pool"""
    import importlib.util
    mk = importlib.util.spec_from_file_location("resolve_make", os.path.join(ROOT, "tests", "golden", "resolve", "make.py"))
    FX = importlib.util.module_from_spec(mk)
    mk.loader.exec_module(FX)
    x = FX.inputs("turn_p48")
    fx = np.load(os.path.join(ROOT, "tests", "golden", "resolve", "turn_p48.npz"))
    got = RU.turn_call(S, x["board"], x["dead"], [x["tree"]], None, x["iters"], reach=x["reach"], at=x["at"], at_card=x["at_card"], river_strategy=False)
    for k in FX.KEYS + ("status",):
        assert got[k][0].tobytes() == np.asarray(fx[k]).tobytes() and got[k][0].dtype == fx[k].dtype, k
    assert got["status"][0] == 0 and (got["node_reach"][0] != 0).any(axis=0).sum() > 900
