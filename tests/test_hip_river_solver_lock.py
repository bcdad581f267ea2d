"""GPU tests of the river solver with locked nodes (pk_solve_river_locked: include/pokerl_hip.h "Locked nodes").
Two kinds.  IDENTITIES with the existing, pinned entry points (no new reference): nothing locked is pk_solve_river_trees byte for byte; a
solution fed back with every row locked and no iteration is reproduced with its value and br; with player 1 locked to a solution player
0's best response is that solution's and its gap falls with the iterations; what the definition says is not read is not read; X and 2X
give the same outputs.  And the RESTATEMENT (tests/solver_lock_spec.py), byte for byte: pools 4, 9, 33 and 46, the default tree and a
four-action root, the lock patterns, a refused spot and a bad tree_of between valid ones, two trees with locks past the smaller one's
rows, one spot, a batch, and more spots than the grid; the stream form; the host form; evaluate_river."""
import ctypes as C

import numpy as np
import pytest

import river_solver_spec as RS
import rvr_spec as VS
import solver_lock_spec as LS
import solver_lock_util as LU
import solver_trees_util as U

pytestmark = pytest.mark.gpu

H = RS.HOLDINGS
KEYS = ("strategy", "value", "br", "status", "valid")
OUT = ("strategy", "value", "br", "status")


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


@pytest.fixture(scope="module")
def S():
    from pokerl_amd import solver
    return solver


def as_dict(r):
    return {k: np.asarray(getattr(r, k)) for k in KEYS}


@pytest.fixture(scope="module")
def plain(PK, S):
    """One P = 16 spot on the default tree and its plain 64-iteration solution -- shared by the identities, never changed"""
    rng = np.random.default_rng(0x10c3)
    board, _, dead = VS.random_boards(rng, 1, 5, 16)
    ranges = LU.random_ranges(rng, 1)
    tree = PK.river_tree(100, 400)
    sol = S.solve_river_batch(board, ranges, [tree], 64, dead, tree_of=np.zeros(1, np.uint32))
    assert sol.status[0] == 0 and sol.valid[0].sum() == 120
    for a in (sol.strategy, sol.value, sol.br):
        a.setflags(write=False)
    return dict(board=board, dead=dead, ranges=ranges, tree=tree, sol=sol)


def test_identity_1_nothing_locked_is_the_tree_per_spot_call(PK, S):
    rng = np.random.default_rng(0x10c1)
    pools = [9, 33, 12, 47, 10]
    board, _, dead = VS.random_boards(rng, 5, 5, lambda i: pools[i])
    board[2, 3] = board[2, 1]                                                 # a refused spot
    ranges = LU.random_ranges(rng, 5)
    trees = [PK.river_tree(100, 400), U.four_action_river_tree()]
    tree_of = np.array([0, 1, 0, 0, 2], np.uint32)                            # ... and a tree_of that names no tree
    want = S.solve_river_batch(board, ranges, trees, 3, dead, tree_of=tree_of)
    flags0 = S.solve_river_batch(board, ranges, trees, 3, dead, tree_of=tree_of, lock=np.zeros((5, 14), np.uint8),
                                 locked=np.full((5, 14, 4, H), 0xFFFF, np.uint16))
    LU.same_bytes(flags0, want, KEYS, "flags all 0")
    assert want.status.tolist() == [0, 0, RS.DUP_CARD, 0, 32]
    one = S.solve_river_batch(board[:2], ranges[:2], trees[0], 3, dead[:2], lock=np.zeros(14, bool), locked=np.zeros((14, 4, H), np.uint16))
    ref = S.solve_river_batch(board[:2], ranges[:2], trees[0], 3, dead[:2])  # one tree, tree_of NULL: the one-tree call
    LU.same_bytes(one, ref, KEYS, "one tree, no tree_of")


def test_identity_2_a_solution_fed_back_is_reproduced(S, plain):
    x = plain
    back = S.solve_river_batch(x["board"], x["ranges"], x["tree"], 0, x["dead"], lock=np.ones(14, bool), locked=x["sol"])
    LU.same_bytes(back, x["sol"], KEYS, "fed back")
    ev = S.evaluate_river_batch(x["board"], x["ranges"], x["tree"], x["sol"].strategy, x["dead"])
    LU.same_bytes(ev, back, KEYS, "evaluate_river_batch")
    assert ev[0].exploitability == x["sol"][0].exploitability and ev[0].ev == x["sol"][0].ev


def test_identity_3_one_side_locked(S, plain):
    x = plain
    lock = x["tree"].rows_of(1)
    assert lock.any() and not lock.all()
    gaps = []
    for iters in (0, 16, 64, 256):
        r = S.solve_river_batch(x["board"], x["ranges"], x["tree"], iters, x["dead"], lock=lock, locked=x["sol"])
        assert r.br[0, 0].tobytes() == x["sol"].br[0, 0].tobytes(), iters     # player 0's best response reads only player 1's reaches
        assert r.strategy[0, lock].tobytes() == x["sol"].strategy[0, lock].tobytes(), iters
        gaps.append(LS.gap(x["ranges"][0], r.value[0], r.br[0], 0))
    print("player 0's gap at 0 / 16 / 64 / 256 iterations:", gaps)
    assert all(a > b for a, b in zip(gaps, gaps[1:])), gaps


def test_identity_4_not_read_means_not_read(PK, S):
    rng = np.random.default_rng(0x10c4)
    pools = [9, 14, 11, 12, 10]
    board, _, dead = VS.random_boards(rng, 5, 5, lambda i: pools[i])
    board[1, 4] = board[1, 0]                                                 # refused
    ranges = LU.random_ranges(rng, 5)
    trees = [PK.river_tree(100, 400), U.forced_river_tree(), U.four_action_river_tree()]
    tree_of = np.array([0, 0, 1, 2, 7], np.uint32)
    lock = LU.lock_of(trees, tree_of, ["p1", "all", "all", [0, 2], "all"])
    locked = LU.random_weights(rng, (5, 14, 4, H))
    a = S.solve_river_batch(board, ranges, trees, 2, dead, tree_of=tree_of, lock=lock, locked=locked)
    lock2, locked2 = LU.poison_unread(lock, locked, trees, tree_of, a.valid)
    assert (lock2 != lock).any() and (locked2 != locked).mean() > 0.5
    b = S.solve_river_batch(board, ranges, trees, 2, dead, tree_of=tree_of, lock=lock2, locked=locked2)
    LU.same_bytes(a, b, KEYS, "0xFFFF in every slot that is not read")
    assert a.status.tolist() == [0, RS.DUP_CARD, 0, 0, 32]


def test_identity_5_scale(S, plain):
    x = plain
    rng = np.random.default_rng(0x10c5)
    locked = LU.random_weights(rng, (1, 14, 4, H))
    lock = x["tree"].rows_of(0)
    a = S.solve_river_batch(x["board"], x["ranges"], x["tree"], 3, x["dead"], lock=lock, locked=locked >> 1)
    b = S.solve_river_batch(x["board"], x["ranges"], x["tree"], 3, x["dead"], lock=lock, locked=(locked >> 1) * 2)
    LU.same_bytes(a, b, KEYS, "X and 2X")


# ------------------------------------------------------------------------------------------------ against the restatement
def spec_batch(x, iters):
    return LS.solve_river_batch(x["board"], x["ranges"], x["trees"], x["tree_of"], iters, x["lock"], x["locked"], x["dead"])


@pytest.fixture(scope="module")
def patterns(PK):
    """Pools 4, 9, 33 and 46 on the default tree and the four-action root under every lock pattern, a refused spot and a bad tree_of
    between them -- the spots, and what the restatement gives at 2 iterations: computed once, never changed"""
    rng = np.random.default_rng(0x10c6)
    pools = [4, 9, 33, 46, 9, 12, 33, 9, 10, 46]
    board, _, dead = VS.random_boards(rng, 10, 5, lambda i: pools[i])
    board[5, 2] = board[5, 0]                                                 # refused, between valid ones
    ranges = LU.random_ranges(rng, 10)
    trees = [PK.river_tree(100, 400), U.four_action_river_tree()]
    tree_of = np.array([0, 1, 0, 1, 0, 0, 1, 3, 1, 0], np.uint32)             # spot 7: a tree_of that names no tree
    pats = ["p1", "all", "none", "p0", [5], "all", [0], "all", "all", "p1"]    # [5]: a single inner node; spot 8: an all-zero locked row
    lock = LU.lock_of(trees, tree_of, pats)
    locked = LU.random_weights(rng, (10, 14, 4, H))
    locked[8] = 0
    x = dict(board=board, dead=dead, ranges=ranges, trees=trees, tree_of=tree_of, lock=lock, locked=locked, pools=pools)
    x["want"] = spec_batch(x, 2)
    for v in x["want"].values():
        v.setflags(write=False)
    return x


def test_the_lock_patterns_at_every_pool_equal_the_restatement(S, patterns):
    x = patterns
    got = as_dict(S.solve_river_batch(x["board"], x["ranges"], x["trees"], 2, x["dead"], tree_of=x["tree_of"], lock=x["lock"], locked=x["locked"]))
    LU.assert_equal(got, x["want"], "ten spots", KEYS)
    assert got["status"].tolist() == [0, 0, 0, 0, 0, RS.DUP_CARD, 0, 32, 0, 0]
    assert got["valid"][3].sum() == 1035 and got["valid"][2].sum() == 528     # the third and the second owned position
    uniform = got["strategy"][8][:, :, got["valid"][8]]                       # the all-zero locked rows: the uniform row
    assert set(np.unique(uniform[0]).tolist()) == {8192} and set(np.unique(uniform[1, :2]).tolist()) == {16384}


@pytest.mark.parametrize("iters", [1, 3])
def test_the_large_pools_at_other_iteration_counts(S, patterns, iters):
    x = patterns
    pick = [2, 3, 6, 9]
    y = {k: (x[k][pick] if k not in ("trees", "pools", "want") else x[k]) for k in x}
    got = as_dict(S.solve_river_batch(y["board"], y["ranges"], y["trees"], iters, y["dead"], tree_of=y["tree_of"], lock=y["lock"], locked=y["locked"]))
    LU.assert_equal(got, spec_batch(y, iters), "P = 33 and 46 at %d iterations" % iters, KEYS)


def test_one_spot_alone_and_more_spots_than_the_grid(S, patterns):
    """a grid of 1 (one spot), and 300 spots -- six of the spots repeated, so that a workgroup's second spot has another lock pattern"""
    x = patterns
    for i in (0, 4, 8):
        one = as_dict(S.solve_river_batch(x["board"][i:i + 1], x["ranges"][i:i + 1], x["trees"], 2, x["dead"][i:i + 1], tree_of=x["tree_of"][i:i + 1],
                                          lock=x["lock"][i:i + 1], locked=x["locked"][i:i + 1]))
        LU.assert_equal(one, {k: v[i:i + 1] for k, v in x["want"].items()}, "spot %d alone" % i, KEYS)
    pick = np.array([0, 1, 4, 5, 7, 8])
    idx = np.tile(pick, 50)
    assert len(idx) > S.GRID_MAX and all(idx[i] != idx[i + S.GRID_MAX] for i in range(len(idx) - S.GRID_MAX))
    got = as_dict(S.solve_river_batch(x["board"][idx], x["ranges"][idx], x["trees"], 2, x["dead"][idx], tree_of=x["tree_of"][idx], lock=x["lock"][idx],
                                      locked=x["locked"][idx]))
    LU.assert_equal(got, {k: v[idx] for k, v in x["want"].items()}, "300 spots", KEYS)


def test_two_trees_with_locks_past_the_smaller_ones_rows(PK, S):
    rng = np.random.default_rng(0x10c7)
    pools = [8, 7, 9, 6]
    board, _, dead = VS.random_boards(rng, 4, 5, lambda i: pools[i])
    ranges = LU.random_ranges(rng, 4)
    trees = [U.forced_river_tree(), U.chain_river_tree()]
    tree_of = np.array([0, 1, 0, 1], np.uint32)
    lock = np.zeros((4, 32), np.uint8)
    lock[0, [1, 5, 31]] = 1
    lock[1, [3, 20, 31]] = 1
    lock[2] = 1
    locked = LU.random_weights(rng, (4, 32, 4, H))
    x = dict(board=board, dead=dead, ranges=ranges, trees=trees, tree_of=tree_of, lock=lock, locked=locked)
    got = as_dict(S.solve_river_batch(board, ranges, trees, 2, dead, tree_of=tree_of, lock=lock, locked=locked))
    LU.assert_equal(got, spec_batch(x, 2), "locks past the smaller tree's rows", KEYS)
    assert not got["strategy"][0, 2:].any() and got["strategy"][1, 31].any()


def test_the_device_forms_on_a_callers_stream(S, patterns):
    """pk_solve_river_locked_d on a non-default stream, then with lock NULL (nothing locked: the tree-per-spot call), then one tree with
    tree_of NULL through solve_river_d"""
    from pokerl_amd import _lib as L
    from pokerl_amd import hipmem
    x = patterns
    m, D = 10, 14
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    ins = [hipmem.DeviceBuffer(a.nbytes).upload(a) for a in (x["board"], x["dead"], x["ranges"], x["tree_of"], x["lock"], x["locked"])]
    outs = [hipmem.DeviceBuffer(n) for n in (m * D * 4 * H * 2, m * 2 * H * 8, m * 2 * H * 8, m)]

    def download():
        assert hip.hipStreamSynchronize(stream) == 0
        return dict(strategy=outs[0].download(np.uint16, m * D * 4 * H).reshape(m, D, 4, H), value=outs[1].download(np.int64, m * 2 * H).reshape(m, 2, H),
                    br=outs[2].download(np.int64, m * 2 * H).reshape(m, 2, H), status=outs[3].download(np.uint8, m))
    S.solve_river_d(m, ins[0].ptr, ins[2].ptr, x["trees"], 2, dead_d=ins[1].ptr, strategy_d=outs[0].ptr, value_d=outs[1].ptr, br_d=outs[2].ptr,
                    status_d=outs[3].ptr, stream=stream, tree_of=ins[3].ptr, lock=ins[4].ptr, locked=ins[5].ptr)
    LU.assert_equal(download(), x["want"], "the stream form", OUT)
    rows = S._TreeRows(x["trees"], 64)
    L.check(L.lib().pk_solve_river_locked_d(0, m, ins[0].ptr, ins[1].ptr, ins[2].ptr, *rows.args(), ins[3].ptr, 2, None, ins[5].ptr, outs[0].ptr,
                                            outs[1].ptr, outs[2].ptr, outs[3].ptr, stream))
    free = S.solve_river_batch(x["board"], x["ranges"], x["trees"], 2, x["dead"], tree_of=x["tree_of"])
    LU.assert_equal(download(), {k: getattr(free, k) for k in OUT}, "lock NULL", OUT)
    S.solve_river_d(m, ins[0].ptr, ins[2].ptr, x["trees"][0], 0, dead_d=ins[1].ptr, strategy_d=outs[0].ptr, value_d=outs[1].ptr, br_d=outs[2].ptr,
                    status_d=outs[3].ptr, stream=stream, lock=ins[4].ptr, locked=ins[5].ptr)
    host = S.solve_river_batch(x["board"], x["ranges"], x["trees"][0], 0, x["dead"], lock=x["lock"], locked=x["locked"])
    LU.assert_equal(download(), {k: getattr(host, k) for k in OUT}, "one tree, tree_of NULL, no iteration: the host form", OUT)
    assert hip.hipStreamDestroy(stream) == 0
    for b in ins + outs:
        b.free()


def test_evaluate_river_is_the_all_locked_call(PK, S, plain):
    x = plain
    rng = np.random.default_rng(0x10c8)
    strategy = LU.random_weights(rng, (14, 4, H))
    cards = [int(c) for c in x["board"][0]]
    a = S.evaluate_river(cards, x["ranges"][0], x["tree"], strategy, dead=int(x["dead"][0]))
    b = S.solve_river(cards, x["ranges"][0], x["tree"], 0, dead=int(x["dead"][0]), lock=np.ones(14, bool), locked=strategy)
    LU.same_bytes(a, b, KEYS, "evaluate_river")
    want = LS.solve_river_spot([int(c) for c in x["board"][0]], x["ranges"][0], x["tree"], 0, np.ones(14), strategy, int(x["dead"][0]))
    LU.assert_equal({k: getattr(a, k) for k in KEYS}, {k: np.asarray(want[k], np.uint8 if k == "status" else None) for k in KEYS}, "the restatement", KEYS)
    assert a.exploitability == RS.exploitability(x["ranges"][0], want["value"], want["br"], want["valid"]) and a.exploitability > 0
    assert (S.evaluate_river(cards, x["ranges"][0], x["tree"], a, dead=int(x["dead"][0])).strategy == a.strategy).all()      # a solution as the strategy
