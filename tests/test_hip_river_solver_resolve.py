"""GPU tests of the river solver's re-solving call (pk_solve_river_resolve: include/pokerl_hip.h "Re-solving").
Two kinds.  IDENTITIES with the pinned entry points, byte for byte (no new reference): reach = ranges << 4 is the locked call; `at` = the
root gives value, br and the root reach; a solution's subtree, re-rooted, locked to the solution's rows and started from node_reach, has
node_value and node_br as its value and br, at every decision node; a gadget whose root is locked to "follow" is the subtree alone, one
locked to "terminate" gives the opponent what it was promised; what the definition says is not read is not read.  And the RESTATEMENT
(tests/resolve_spec.py), byte for byte: pools 4, 9, 33 and 46, a free gadget solve, `at` at every node kind, a refused spot, a bad tree_of
and a bad `at` between valid ones, reaches above the limit and given values beyond the clamp, two trees of different size in one call, one
spot, a batch and more spots than the grid, the host form and the stream form."""
import ctypes as C

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
KEYS = ("strategy", "value", "br", "status", "valid")
OUT = RU.RIVER_KEYS


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


@pytest.fixture(scope="module")
def S():
    from pokerl_amd import solver
    return solver


@pytest.fixture(scope="module")
def spot(PK):
    """One P = 12 spot and the default tree -- shared by the identities, never changed"""
    rng = np.random.default_rng(0x3171)
    board, _, dead = VS.random_boards(rng, 1, 5, 12)
    ranges = LU.random_ranges(rng, 1)
    for a in (board, dead, ranges):
        a.setflags(write=False)
    return dict(board=board, dead=dead, ranges=ranges, tree=PK.river_tree(100, 400))


def test_identity_1_reach_from_ranges_is_the_locked_call(PK, S):
    rng = np.random.default_rng(0x3172)
    pools = [9, 33, 12, 16, 10]
    board, _, dead = VS.random_boards(rng, 5, 5, lambda i: pools[i])
    board[2, 3] = board[2, 1]                                                 # a refused spot
    ranges = LU.random_ranges(rng, 5)
    trees = [PK.river_tree(100, 400), U.four_action_river_tree()]
    tree_of = np.array([0, 1, 0, 0, 2], np.uint32)                            # ... and a tree_of that names no tree
    lock = LU.lock_of(trees, tree_of, ["p1", "none", "all", [0, 2], "all"])
    locked = LU.random_weights(rng, (5, 14, 4, H))
    want = S.solve_river_batch(board, ranges, trees, 3, dead, tree_of=tree_of, lock=lock, locked=locked)
    got = S.solve_river_batch(board, None, trees, 3, dead, tree_of=tree_of, lock=lock, locked=locked, reach=ranges.astype(np.uint32) << 4)
    LU.same_bytes(got, want, KEYS, "reach = ranges << 4")
    assert want.status.tolist() == [0, 0, RS.DUP_CARD, 0, 32] and got.node_value is None and got.ranges is None
    assert got[0].ev == want[0].ev and got[0].exploitability == want[0].exploitability


def test_identity_2_at_the_root(S, spot):
    x = spot
    r = S.solve_river_batch(x["board"], x["ranges"], x["tree"], 16, x["dead"], at=0)
    plain = S.solve_river_batch(x["board"], x["ranges"], x["tree"], 16, x["dead"], lock=np.zeros(14, bool), locked=np.zeros((14, 4, H), np.uint16))
    LU.same_bytes(r, plain, KEYS, "at changes no other output")
    assert r.node_value.tobytes() == r.value.tobytes() and r.node_br.tobytes() == r.br.tobytes() and r.node_value.any()
    assert (r.node_reach == (x["ranges"].astype(np.uint32) << 4) * r.valid[:, None]).all() and r.node_reach.dtype == np.uint32


@pytest.mark.parametrize("iters", [3, 64])
def test_identity_3_every_subtree_of_a_solution(S, spot, iters):
    x = spot
    tree = x["tree"]
    nodes = tree.decision_nodes
    m = len(nodes)
    rep = lambda a: np.repeat(a, m, axis=0)
    whole = S.solve_river_batch(rep(x["board"]), rep(x["ranges"]), tree, iters, rep(x["dead"]), at=np.array(nodes))
    assert not whole.status.any() and all(whole.strategy[i].tobytes() == whole.strategy[0].tobytes() for i in range(m))
    subs = [tree.subtree(n) for n in nodes]
    D = max(len(rows) for _, rows in subs)
    locked = np.full((m, D, 4, H), 0xFFFF, np.uint16)                          # (rows past a subtree's own: not read)
    for i, (_, rows) in enumerate(subs):
        locked[i, :len(rows)] = whole.strategy[i][rows]
    sub = S.solve_river_batch(rep(x["board"]), None, [t for t, _ in subs], 0, rep(x["dead"]), lock=np.ones((m, D), np.uint8), locked=locked,
                              reach=whole.node_reach, at=np.zeros(m, np.uint8))
    assert not sub.status.any()
    for i, n in enumerate(nodes):
        assert sub.value[i].tobytes() == whole.node_value[i].tobytes(), ("value", iters, n)
        assert sub.br[i].tobytes() == whole.node_br[i].tobytes(), ("br", iters, n)
        assert sub.node_reach[i].tobytes() == whole.node_reach[i].tobytes(), ("reach", iters, n)
    assert whole.node_value[1:].any() and (whole.node_br >= whole.node_value).all()


def test_identities_7_and_8_a_gadget_locked_at_its_root(PK, S, spot):
    x = spot
    tree = x["tree"]
    node = int(tree.child[0][1])                                              # after player 0's first bet: player 1, the opponent, is to act
    first = S.solve_river_batch(x["board"], x["ranges"], tree, 16, x["dead"], at=node)
    sub, rows = tree.subtree(node)
    g = PK.gadget_tree(sub, 1)
    Dg = len(g.decision_nodes)
    rng = np.random.default_rng(0x3173)
    given = np.zeros((1, 2, H), np.int64)
    given[0, 1] = rng.integers(-(1 << 44), 1 << 44, H)
    lock, locked = np.zeros(Dg, bool), np.zeros((Dg, 4, H), np.uint16)
    lock[0], locked[0, 1] = True, 1                                           # weights 0 and 1: follow
    follow = S.solve_river_batch(x["board"], None, g, 16, x["dead"], lock=lock, locked=locked, reach=first.node_reach, given=given)
    alone = S.solve_river_batch(x["board"], None, sub, 16, x["dead"], reach=first.node_reach)
    assert follow.strategy[0, 1:].tobytes() == alone.strategy[0].tobytes() and follow.value.tobytes() == alone.value.tobytes()
    assert follow.br[0, 0].tobytes() == alone.br[0, 0].tobytes()              # the hero's; the opponent's best response ignores the lock:
    assert (follow.br[0, 1] == np.maximum(given[0, 1], alone.br[0, 1]) * alone.valid[0]).all()
    locked[0, 0], locked[0, 1] = 1, 0                                         # terminate
    stop = S.solve_river_batch(x["board"], None, g, 16, x["dead"], lock=lock, locked=locked, reach=first.node_reach, given=given, at=2)
    assert (stop.value[0, 1] == given[0, 1] * stop.valid[0]).all() and stop.value[0, 1].any()
    assert not stop.node_value[0, 0].any() and not stop.node_reach[0, 1].any() and stop.node_reach[0, 0].any()     # nothing of the opponent follows


def test_identity_9_not_read_means_not_read(PK, S):
    rng = np.random.default_rng(0x3174)
    pools = [9, 14, 11, 12]
    board, _, dead = VS.random_boards(rng, 4, 5, lambda i: pools[i])
    board[1, 4] = board[1, 0]                                                 # refused
    small = PK.river_tree(100, 50)
    trees = [small, PK.gadget_tree(small, 0)]
    tree_of = np.array([0, 1, 1, 0], np.uint32)
    reach = rng.integers(0, RZ.RIVER_LIM + 1, (4, 2, H)).astype(np.uint32)
    given = rng.integers(-(1 << 40), 1 << 40, (4, 2, H)).astype(np.int64)
    at = np.array([1, 0, 2, 0], np.uint8)
    a = RU.river_call(S, board, dead, trees, tree_of, 2, ranges=np.zeros((4, 2, H), np.uint16), reach=reach, given=given, at=at)
    reach2, given2 = reach.copy(), given.copy()
    for i in range(4):
        reach2[i][:, RU.invalid_holdings(board[i], 5, dead[i])] = 0xFFFFFFFF
        given2[i][:, RU.invalid_holdings(board[i], 5, dead[i])] = -1
    given2[[0, 3]] = -1                                                       # no given node in their tree
    assert (reach2 != reach).mean() > 0.5 and (given2 != given).mean() > 0.5
    b = RU.river_call(S, board, dead, trees, tree_of, 2, ranges=np.full((4, 2, H), 0xFFFF, np.uint16), reach=reach2, given=given2, at=at)
    RU.assert_equal(b, a, "ones in every slot that is not read", OUT)
    c = RU.river_call(S, board, dead, trees, tree_of, 2, ranges=None, reach=reach2, given=given2, at=at)
    RU.assert_equal(c, a, "ranges NULL", OUT)
    assert a["status"].tolist() == [0, RS.DUP_CARD, 0, 0] and a["node_value"][2].any()


# ------------------------------------------------------------------------------------------------ against the restatement
def spec_batch(x, iters, pick=None):
    y = x if pick is None else {k: (v[pick] if isinstance(v, np.ndarray) else v) for k, v in x.items() if k != "want"}
    return RZ.solve_river_batch(y["board"], None, y["trees"], y["tree_of"], iters, y["lock"], y["locked"], y["dead"], y["reach"], y["given"], y["at"])


def device_batch(S, x, iters, pick=None):
    y = x if pick is None else {k: (v[pick] if isinstance(v, np.ndarray) else v) for k, v in x.items() if k != "want"}
    return RU.river_call(S, y["board"], y["dead"], y["trees"], y["tree_of"], iters, reach=y["reach"], given=y["given"], at=y["at"], lock=y["lock"], locked=y["locked"])


@pytest.fixture(scope="module")
def patterns(PK):
    """Pools 4, 9, 33 and 46 on the default tree, a small tree and two gadgets, `at` at every node kind, reaches above the limit, given
    values beyond the clamp, a refused spot, a bad tree_of and two bad `at` between them -- the spots, and what the restatement gives at 2
    iterations: computed once, never changed"""
    rng = np.random.default_rng(0x3175)
    pools = [4, 9, 33, 46, 9, 12, 10, 9, 11, 10]
    board, _, dead = VS.random_boards(rng, 10, 5, lambda i: pools[i])
    board[5, 2] = board[5, 0]                                                 # refused, between valid ones
    default, small, four = PK.river_tree(100, 400), PK.river_tree(100, 50), U.four_action_river_tree()
    trees = [default, PK.gadget_tree(four, 0), PK.gadget_tree(small, 1), small]
    tree_of = np.array([2, 1, 0, 2, 0, 0, 4, 3, 1, 3], np.uint32)             # spot 6: a tree_of that names no tree
    leaf = lambda t, kind: next(v for v in range(t.n) if t.kind[v] == kind)
    at = np.array([0, 1, leaf(default, 4), 2, leaf(default, 3), 0, 0, small.n, 200, small.n - 1], np.uint8)      # spots 7, 8: no such node
    #               root (P1)  given  showdown  P0 below the gadget  fold  (refused)  (no tree)  bad  bad  the last node
    reach = RU.random_reach(rng, board, 5, dead, RZ.RIVER_LIM, over=(1, 3))
    reach[[5, 6, 7, 8]] = 0xFFFFFFFF                                          # refused spots: never read
    given = RU.random_given(rng, trees, tree_of, 10, beyond=(1, 3))
    lock = LU.lock_of(trees, tree_of, ["none", [0], "none", "none", "p1", "all", "all", "all", "all", "none"])       # spot 1: a gadget root locked to random weights
    locked = LU.random_weights(rng, (10, 14, 4, H))
    x = dict(board=board, dead=dead, trees=trees, tree_of=tree_of, at=at, reach=reach, given=given, lock=lock, locked=locked)
    x["want"] = spec_batch(x, 2)
    for v in x["want"].values():
        v.setflags(write=False)
    return x


def test_the_patterns_at_every_pool_equal_the_restatement(S, patterns):
    x = patterns
    got = device_batch(S, x, 2)
    RU.assert_equal(got, x["want"], "ten spots", OUT)
    assert got["status"].tolist() == [0, 0, 0, 0, 0, RS.DUP_CARD, 32, 32, 32, 0]
    assert x["want"]["valid"][3].sum() == 1035 and x["want"]["valid"][2].sum() == 528           # the third and the second owned position
    for i in (0, 1, 2, 3, 4, 9):
        assert got["node_reach"][i].any() and got["node_value"][i].any(), i
    for i in (5, 6, 7, 8):
        assert not any(got[k][i].any() for k in OUT[:-1]), i
    clamped = np.clip(x["given"][1], -RZ.GIVEN_LIM, RZ.GIVEN_LIM) * x["want"]["valid"][1]
    assert (got["node_value"][1] == clamped).all() and (got["node_br"][1] == clamped).all() and (np.abs(x["given"][1]) > RZ.GIVEN_LIM).any()


@pytest.mark.parametrize("iters", [0, 3])
def test_the_large_pools_at_other_iteration_counts(S, patterns, iters):
    pick = np.array([2, 3, 7, 1])
    RU.assert_equal(device_batch(S, patterns, iters, pick), spec_batch(patterns, iters, pick), "P = 33 and 46 at %d iterations" % iters, OUT)


def test_one_spot_alone_and_more_spots_than_the_grid(S, patterns):
    """a grid of 1 (one spot), and 300 spots -- seven of the spots repeated, so that a workgroup's second spot has another tree and node"""
    x = patterns
    for i in (0, 1, 4):
        RU.assert_equal(device_batch(S, x, 2, np.array([i])), {k: v[i:i + 1] for k, v in x["want"].items()}, "spot %d alone" % i, OUT)
    idx = np.tile(np.array([0, 1, 4, 5, 7, 8, 9]), 43)
    assert len(idx) > S.GRID_MAX and all(idx[i] != idx[i + S.GRID_MAX] for i in range(len(idx) - S.GRID_MAX))
    RU.assert_equal(device_batch(S, x, 2, idx), {k: v[idx] for k, v in x["want"].items()}, "301 spots", OUT)


def test_two_trees_of_different_size_and_a_free_gadget_solve(PK, S):
    rng = np.random.default_rng(0x3176)
    pools = [8, 7, 9, 6]
    board, _, dead = VS.random_boards(rng, 4, 5, lambda i: pools[i])
    forced, chain = U.forced_river_tree(), U.chain_river_tree()
    trees = [forced, chain, PK.gadget_tree(PK.river_tree(100, 400), 1)]
    tree_of = np.array([0, 1, 2, 1], np.uint32)
    at = np.array([forced.n - 1, chain.n - 1, 2, 40], np.uint8)
    x = dict(board=board, dead=dead, trees=trees, tree_of=tree_of, at=at, reach=RU.random_reach(rng, board, 5, dead, RZ.RIVER_LIM),
             given=RU.random_given(rng, trees, tree_of, 4), lock=None, locked=None)
    got = device_batch(S, x, 8)
    RU.assert_equal(got, spec_batch(x, 8), "a small tree, the largest, a gadget, the largest again", OUT)
    assert not got["status"].any() and got["strategy"][2, 0].any() and got["strategy"].shape[1] == 32


def test_the_device_form_on_a_callers_stream(S, patterns):
    """pk_solve_river_resolve_d on a non-default stream; then with only node_value asked for; then the Python host form where nothing is
    beyond its bounds"""
    from pokerl_amd import hipmem
    x = patterns
    pick = np.array([0, 4, 5, 7, 9, 2])
    y = {k: (v[pick] if isinstance(v, np.ndarray) else v) for k, v in x.items() if k != "want"}
    want = {k: v[pick] for k, v in x["want"].items()}
    m, D = len(pick), 14
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    ins = [hipmem.DeviceBuffer(a.nbytes).upload(a) for a in (y["board"], y["dead"], y["tree_of"], y["lock"], y["locked"], y["reach"], y["given"], y["at"])]
    sizes = dict(strategy=(np.uint16, (m, D, 4, H)), value=(np.int64, (m, 2, H)), br=(np.int64, (m, 2, H)), node_reach=(np.uint32, (m, 2, H)),
                 node_value=(np.int64, (m, 2, H)), node_br=(np.int64, (m, 2, H)), status=(np.uint8, (m,)))
    outs = {k: hipmem.DeviceBuffer(int(np.prod(shape)) * np.dtype(dt).itemsize) for k, (dt, shape) in sizes.items()}

    def download(keys):
        assert hip.hipStreamSynchronize(stream) == 0
        return {k: outs[k].download(sizes[k][0], int(np.prod(sizes[k][1]))).reshape(sizes[k][1]) for k in keys}
    S.solve_river_d(m, ins[0].ptr, None, y["trees"], 2, dead_d=ins[1].ptr, strategy_d=outs["strategy"].ptr, value_d=outs["value"].ptr, br_d=outs["br"].ptr,
                    status_d=outs["status"].ptr, stream=stream, tree_of=ins[2].ptr, lock=ins[3].ptr, locked=ins[4].ptr, reach=ins[5].ptr, given=ins[6].ptr,
                    at=ins[7].ptr, node_reach_d=outs["node_reach"].ptr, node_value_d=outs["node_value"].ptr, node_br_d=outs["node_br"].ptr)
    RU.assert_equal(download(OUT), want, "the stream form", OUT)
    poison = np.full((m, 2, H), 0x5A5A5A5A, np.uint32)
    outs["node_reach"].upload(poison)
    S.solve_river_d(m, ins[0].ptr, None, y["trees"], 2, dead_d=ins[1].ptr, status_d=outs["status"].ptr, stream=stream, tree_of=ins[2].ptr, reach=ins[5].ptr,
                    given=ins[6].ptr, at=ins[7].ptr, node_value_d=outs["node_value"].ptr)
    got = download(("node_value", "node_reach", "status"))
    free = RZ.solve_river_batch(y["board"], None, y["trees"], y["tree_of"], 2, None, None, y["dead"], y["reach"], y["given"], y["at"])
    RU.assert_equal(got, free, "node_value alone, nothing locked", ("node_value", "status"))
    assert got["node_reach"].tobytes() == poison.tobytes()                    # an output that was not passed is not written
    assert hip.hipStreamDestroy(stream) == 0
    for b in ins + list(outs.values()):
        b.free()
    ok = np.array([0, 4, 9])                                                  # (spots whose reach and given pass the wrapper's bounds)
    z = {k: (v[ok] if isinstance(v, np.ndarray) else v) for k, v in x.items() if k != "want"}
    reach = np.where(z["reach"] == 0xFFFFFFFF, 0, z["reach"])
    host = S.solve_river_batch(z["board"], None, z["trees"], 2, z["dead"], tree_of=z["tree_of"], lock=z["lock"], locked=z["locked"], reach=reach,
                               given=np.where(z["given"] == -1, 0, z["given"]), at=z["at"])
    RU.assert_equal({k: getattr(host, k) for k in OUT}, {k: v[ok] for k, v in x["want"].items()}, "solve_river_batch", OUT)


def test_resolve_river_unsafe_and_safe(PK, S, spot):
    x = spot
    tree, cards, dead = x["tree"], [int(c) for c in x["board"][0]], int(x["dead"][0])
    node = int(tree.child[0][1])
    first = S.solve_river(cards, x["ranges"][0], tree, 64, dead=dead, at=node)
    sub, rows = tree.subtree(node)
    unsafe = S.resolve_river(cards, sub, first.node_reach, 16, 0, dead=dead)
    want = RZ.solve_river_spot(cards, None, sub, 16, dead=dead, reach=first.node_reach)
    assert unsafe.strategy.tobytes() == want["strategy"].tobytes() and unsafe.value.tobytes() == want["value"].tobytes() and unsafe.tree is sub
    safe = S.resolve_river(cards, sub, first.node_reach, 16, 0, opponent_values=first.node_br[1], dead=dead)
    flat = first.node_reach.astype(np.int64)
    flat[1] = int(flat[1].max())
    given = np.zeros((2, H), np.int64)
    given[1] = first.node_br[1]
    want = RZ.solve_river_spot(cards, None, PK.gadget_tree(sub, 1), 16, dead=dead, reach=flat, given=given)
    assert safe.strategy.shape == unsafe.strategy.shape and safe.strategy.tobytes() == want["strategy"][1:].tobytes() and safe.br.tobytes() == want["br"].tobytes()
    assert safe.tree is sub and safe.exploitability >= 0
