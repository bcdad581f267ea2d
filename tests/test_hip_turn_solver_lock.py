"""GPU tests of the turn solver with locked nodes (pk_solve_turn_locked: include/pokerl_hip.h "Locked nodes").
The IDENTITIES with the existing, pinned entry points (nothing locked; a solution fed back; one side locked; not read means not read;
scale), the RESTATEMENT live at P = 5, 9 and 12 (tests/solver_lock_spec.py) and through its fixtures at P = 33 and 48
(tests/golden/solver_lock: the inputs are regenerated from the fixture's seed by make.py there, which the CPU build of the kernel checks
too), the stream form, the host form and evaluate_turn."""
import ctypes as C
import hashlib
import importlib.util
import os

import numpy as np
import pytest

import rvr_spec as VS
import solver_lock_spec as LS
import solver_lock_util as LU
import solver_trees_util as U
import turn_solver_spec as TS

pytestmark = pytest.mark.gpu

H = TS.HOLDINGS
KEYS = ("strategy", "river_strategy", "value", "br", "status", "valid")
OUT = ("strategy", "river_strategy", "value", "br", "status")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solver_lock")


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


@pytest.fixture(scope="module")
def S():
    from pokerl_amd import solver
    return solver


def spots(rng, pools):
    board, _, dead = VS.random_boards(rng, len(pools), 4, lambda i: pools[i])
    return np.ascontiguousarray(board[:, :4]), dead, LU.random_ranges(rng, len(pools))


def as_dict(r):
    return {k: np.asarray(getattr(r, k)) for k in KEYS}


def pool_cards(valid):
    """per spot: the canonical indices of the pool's cards, from the valid holdings"""
    A = np.array([a for b in range(52) for a in range(b)])
    B = np.array([b for b in range(52) for a in range(b)])
    return [set(A[v].tolist()) | set(B[v].tolist()) for v in valid]


@pytest.fixture(scope="module")
def plain(PK, S):
    """One P = 9 spot on turn_tree(100, 400, (1.0,), 1) and its plain 16-iteration solution with river_strategy -- shared, never changed"""
    rng = np.random.default_rng(0x10c4)
    board, dead, ranges = spots(rng, [9])
    tree = PK.turn_tree(100, 400, (1.0,), 1)
    sol = S.solve_turn_batch(board, ranges, [tree], 16, dead, river_strategy=True, tree_of=np.zeros(1, np.uint32))
    assert sol.status[0] == 0 and sol.pool[0] == 9
    for a in (sol.strategy, sol.river_strategy, sol.value, sol.br):
        a.setflags(write=False)
    return dict(board=board, dead=dead, ranges=ranges, tree=tree, sol=sol)


def test_identity_1_nothing_locked_is_the_tree_per_spot_call(PK, S):
    rng = np.random.default_rng(0x10d1)
    board, dead, ranges = spots(rng, [9, 20, 10, 48, 8])
    board[2, 3] = board[2, 1]                                                 # a refused spot
    trees = [PK.turn_tree(30, 20, (1.0,), 1), U.allin_turn_tree()]
    tree_of = np.array([0, 1, 0, 0, 2], np.uint32)                            # ... and a tree_of that names no tree
    want = S.solve_turn_batch(board, ranges, trees, 2, dead, river_strategy=True, tree_of=tree_of)
    flags0 = S.solve_turn_batch(board, ranges, trees, 2, dead, river_strategy=True, tree_of=tree_of, lock=np.zeros((5, 4), np.uint8),
                                locked=np.full((5, 4, 4, H), 0xFFFF, np.uint16), river_lock=np.zeros(4, bool), river_locked=np.full((4, 52, 4, H), 0xFFFF, np.uint16))
    LU.same_bytes(flags0, want, KEYS, "flags all 0")
    assert want.status.tolist() == [0, 0, TS.DUP_CARD, 0, 32]
    one = S.solve_turn_batch(board[:2], ranges[:2], trees[0], 2, dead[:2], river_strategy=True, lock=np.zeros(4, bool), locked=np.zeros((4, 4, H), np.uint16))
    ref = S.solve_turn_batch(board[:2], ranges[:2], trees[0], 2, dead[:2], river_strategy=True)      # one tree, tree_of NULL, no river_ pair
    LU.same_bytes(one, ref, KEYS, "one tree, no tree_of")


def test_identity_2_a_solution_fed_back_is_reproduced(S, plain):
    x = plain
    back = S.solve_turn_batch(x["board"], x["ranges"], x["tree"], 0, x["dead"], river_strategy=True, lock=np.ones(4, bool), locked=x["sol"],
                              river_lock=np.ones(12, bool))
    LU.same_bytes(back, x["sol"], KEYS, "fed back")
    ev = S.evaluate_turn_batch(x["board"], x["ranges"], x["tree"], x["sol"].strategy, x["sol"].river_strategy, x["dead"], return_river_strategy=True)
    LU.same_bytes(ev, back, KEYS, "evaluate_turn_batch")
    assert ev[0].exploitability == x["sol"][0].exploitability and ev[0].ev == x["sol"][0].ev


def test_identity_3_one_side_locked(S, plain):
    x = plain
    lock, rlock = x["tree"].rows_of(1)
    assert lock.any() and not lock.all() and rlock.any() and not rlock.all()
    gaps = []
    for iters in (0, 16, 64):
        r = S.solve_turn_batch(x["board"], x["ranges"], x["tree"], iters, x["dead"], river_strategy=True, lock=lock, locked=x["sol"], river_lock=rlock)
        assert r.br[0, 0].tobytes() == x["sol"].br[0, 0].tobytes(), iters     # player 0's best response reads only player 1's reaches
        assert r.strategy[0, lock].tobytes() == x["sol"].strategy[0, lock].tobytes(), iters
        assert r.river_strategy[0, rlock].tobytes() == x["sol"].river_strategy[0, rlock].tobytes(), iters
        gaps.append(LS.gap(x["ranges"][0], r.value[0], r.br[0], 0))
    print("player 0's gap at 0 / 16 / 64 iterations:", gaps)
    assert all(a > b for a, b in zip(gaps, gaps[1:])), gaps


def test_identity_4_not_read_means_not_read(PK, S):
    rng = np.random.default_rng(0x10d4)
    board, dead, ranges = spots(rng, [9, 12, 8, 10, 9])
    board[1, 3] = board[1, 0]                                                 # refused
    trees = [PK.turn_tree(30, 20, (1.0,), 1), U.allin_turn_tree()]
    tree_of = np.array([0, 0, 1, 0, 7], np.uint32)
    lock = LU.lock_of(trees, tree_of, ["p1", "all", "all", [0, 2], "all"])
    rlock = LU.lock_of(trees, tree_of, ["p0", "all", [1], "all", "all"], river=True)
    locked, rlocked = LU.random_weights(rng, (5, 4, 4, H)), LU.random_weights(rng, (5, 4, 52, 4, H))
    kw = dict(river_strategy=True, tree_of=tree_of)
    a = S.solve_turn_batch(board, ranges, trees, 2, dead, lock=lock, locked=locked, river_lock=rlock, river_locked=rlocked, **kw)
    lock2, locked2 = LU.poison_unread(lock, locked, trees, tree_of, a.valid)
    rlock2, rlocked2 = LU.poison_unread(rlock, rlocked, trees, tree_of, a.valid, river=True, pool=pool_cards(a.valid))
    assert (rlock2 != rlock).any() and (locked2 != locked).mean() > 0.5 and (rlocked2 != rlocked).mean() > 0.5
    b = S.solve_turn_batch(board, ranges, trees, 2, dead, lock=lock2, locked=locked2, river_lock=rlock2, river_locked=rlocked2, **kw)
    LU.same_bytes(a, b, KEYS, "0xFFFF in every slot that is not read")
    assert a.status.tolist() == [0, TS.DUP_CARD, 0, 0, 32]


def test_identity_5_scale(S, plain):
    x = plain
    rng = np.random.default_rng(0x10d5)
    locked, rlocked = LU.random_weights(rng, (1, 4, 4, H)), LU.random_weights(rng, (1, 12, 52, 4, H))
    lock, rlock = x["tree"].rows_of(0)
    kw = dict(river_strategy=True, lock=lock, river_lock=rlock)
    a = S.solve_turn_batch(x["board"], x["ranges"], x["tree"], 2, x["dead"], locked=locked >> 1, river_locked=rlocked >> 1, **kw)
    b = S.solve_turn_batch(x["board"], x["ranges"], x["tree"], 2, x["dead"], locked=(locked >> 1) * 2, river_locked=(rlocked >> 1) * 2, **kw)
    LU.same_bytes(a, b, KEYS, "X and 2X")


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.fixture(scope="module")
def patterns(PK):
    """Pools 5, 9 and 12 on two trees under the lock patterns of both levels, a refused spot and a bad tree_of between them, locks past the
    smaller tree's rows -- and what the restatement gives at 2 iterations: computed once, never changed"""
    rng = np.random.default_rng(0x10d6)
    board, dead, ranges = spots(rng, [5, 9, 12, 9, 8, 9, 12, 7])
    board[3, 2] = board[3, 0]                                                 # refused, between valid ones
    trees = [PK.turn_tree(30, 20, (1.0,), 1), U.allin_turn_tree()]
    tree_of = np.array([0, 0, 0, 0, 1, 5, 1, 0], np.uint32)                   # spot 5: a tree_of that names no tree
    lock = LU.lock_of(trees, tree_of, ["p1", "all", "none", "all", [0, 3], "all", "p0", "all"])
    rlock = LU.lock_of(trees, tree_of, ["p1", "none", "all", "all", [1, 3], "all", "none", "all"], river=True)
    lock[4, 3] = rlock[4, 3] = rlock[6, 2] = 1                                # flags on rows the ten-node tree does not have
    locked, rlocked = LU.random_weights(rng, (8, 4, 4, H)), LU.random_weights(rng, (8, 4, 52, 4, H))
    locked[7], rlocked[7] = 0, 0                                              # all-zero locked rows: the uniform row
    x = dict(board=board, dead=dead, ranges=ranges, trees=trees, tree_of=tree_of, lock=lock, locked=locked, river_lock=rlock, river_locked=rlocked)
    x["want"] = LS.solve_turn_batch(board, ranges, trees, tree_of, 2, lock, locked, rlock, rlocked, dead)
    for v in x["want"].values():
        v.setflags(write=False)
    return x


def test_the_lock_patterns_equal_the_restatement(S, patterns):
    x = patterns
    r = S.solve_turn_batch(x["board"], x["ranges"], x["trees"], 2, x["dead"], river_strategy=True, tree_of=x["tree_of"], lock=x["lock"], locked=x["locked"],
                           river_lock=x["river_lock"], river_locked=x["river_locked"])
    got = as_dict(r)
    LU.assert_equal(got, x["want"], "eight spots", KEYS)
    assert got["status"].tolist() == [0, 0, 0, TS.DUP_CARD, 0, 32, 0, 0] and r.pool.tolist() == x["want"]["P"].tolist()
    for i in (0, 4, 7):                                                       # a grid of 1: the spot alone
        one = as_dict(S.solve_turn_batch(x["board"][i:i + 1], x["ranges"][i:i + 1], x["trees"], 2, x["dead"][i:i + 1], river_strategy=True,
                                         tree_of=x["tree_of"][i:i + 1], lock=x["lock"][i:i + 1], locked=x["locked"][i:i + 1],
                                         river_lock=x["river_lock"][i:i + 1], river_locked=x["river_locked"][i:i + 1]))
        LU.assert_equal(one, {k: x["want"][k][i:i + 1] for k in KEYS}, "spot %d alone" % i, KEYS)


def test_twice_the_spots_by_repeating_them(S, patterns):
    x = patterns
    idx = np.concatenate([np.arange(8), np.arange(8)[::-1]])
    got = as_dict(S.solve_turn_batch(x["board"][idx], x["ranges"][idx], x["trees"], 2, x["dead"][idx], river_strategy=True, tree_of=x["tree_of"][idx],
                                     lock=x["lock"][idx], locked=x["locked"][idx], river_lock=x["river_lock"][idx], river_locked=x["river_locked"][idx]))
    LU.assert_equal(got, {k: x["want"][k][idx] for k in KEYS}, "sixteen spots", KEYS)


@pytest.mark.parametrize("name", ["turn_p33", "turn_p48"])
def test_the_large_pools_through_the_restatements_fixtures(S, name):
    """528 and 1128 turn holdings, 496 and 1081 under a card: the second and the third owned position"""
    mk = importlib.util.spec_from_file_location("solver_lock_make", os.path.join(GOLDEN, "make.py"))
    make = importlib.util.module_from_spec(mk)
    mk.loader.exec_module(make)
    x = make.inputs(name)
    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    r = S.solve_turn_batch(x["board"], x["ranges"], x["tree"], x["iters"], x["dead"], river_strategy=True, lock=x["lock"], locked=x["locked"],
                           river_lock=x["river_lock"], river_locked=x["river_locked"])
    assert r.pool[0] == make.FIXTURES[name][0]
    want = dict(strategy=fx["strategy"][None], value=fx["value"][None], br=fx["br"][None], status=fx["status"][None])
    LU.assert_equal({k: getattr(r, k) for k in want}, want, name, ("strategy", "value", "br", "status"))
    assert hashlib.sha256(np.ascontiguousarray(r.river_strategy[0]).tobytes()).hexdigest() == str(fx["river_sha256"])


def test_the_device_forms_on_a_callers_stream(S, patterns):
    """pk_solve_turn_locked_d on a non-default stream, then with both lock pointers NULL (nothing locked: the tree-per-spot call)"""
    from pokerl_amd import _lib as L
    from pokerl_amd import hipmem
    x = patterns
    m, Dt, Dr = 8, 4, 4
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    ins = [hipmem.DeviceBuffer(a.nbytes).upload(a) for a in (x["board"], x["dead"], x["ranges"], x["tree_of"], x["lock"], x["locked"], x["river_lock"],
                                                             x["river_locked"])]
    outs = [hipmem.DeviceBuffer(n) for n in (m * Dt * 4 * H * 2, m * Dr * 52 * 4 * H * 2, m * 2 * H * 8, m * 2 * H * 8, m)]

    def download():
        assert hip.hipStreamSynchronize(stream) == 0
        return dict(strategy=outs[0].download(np.uint16, m * Dt * 4 * H).reshape(m, Dt, 4, H),
                    river_strategy=outs[1].download(np.uint16, m * Dr * 52 * 4 * H).reshape(m, Dr, 52, 4, H),
                    value=outs[2].download(np.int64, m * 2 * H).reshape(m, 2, H), br=outs[3].download(np.int64, m * 2 * H).reshape(m, 2, H),
                    status=outs[4].download(np.uint8, m))
    S.solve_turn_d(m, ins[0].ptr, ins[2].ptr, x["trees"], 2, dead_d=ins[1].ptr, strategy_d=outs[0].ptr, river_strategy_d=outs[1].ptr, value_d=outs[2].ptr,
                   br_d=outs[3].ptr, status_d=outs[4].ptr, stream=stream, tree_of=ins[3].ptr, lock=ins[4].ptr, locked=ins[5].ptr, river_lock=ins[6].ptr,
                   river_locked=ins[7].ptr)
    LU.assert_equal(download(), x["want"], "the stream form", OUT)
    rows = S._TreeRows(x["trees"], 128)
    L.check(L.lib().pk_solve_turn_locked_d(0, m, ins[0].ptr, ins[1].ptr, ins[2].ptr, *rows.args(), ins[3].ptr, 2, None, ins[5].ptr, None, None, outs[0].ptr,
                                           outs[1].ptr, outs[2].ptr, outs[3].ptr, outs[4].ptr, stream))
    free = S.solve_turn_batch(x["board"], x["ranges"], x["trees"], 2, x["dead"], river_strategy=True, tree_of=x["tree_of"])
    LU.assert_equal(download(), {k: getattr(free, k) for k in OUT}, "lock NULL", OUT)
    assert hip.hipStreamDestroy(stream) == 0
    for b in ins + outs:
        b.free()


def test_evaluate_turn_is_the_all_locked_call(S, plain):
    x = plain
    rng = np.random.default_rng(0x10d8)
    strategy, rstrat = LU.random_weights(rng, (4, 4, H)), LU.random_weights(rng, (12, 52, 4, H))
    cards, dead = [int(c) for c in x["board"][0]], int(x["dead"][0])
    a = S.evaluate_turn(cards, x["ranges"][0], x["tree"], strategy, rstrat, dead=dead)
    b = S.solve_turn(cards, x["ranges"][0], x["tree"], 0, dead=dead, lock=np.ones(4, bool), locked=strategy, river_lock=np.ones(12, bool), river_locked=rstrat)
    LU.same_bytes(a, b, KEYS, "evaluate_turn")
    want = LS.solve_turn_spot(cards, x["ranges"][0], x["tree"], 0, np.ones(4), strategy, np.ones(12), rstrat, dead)
    for k in ("strategy", "value", "br", "valid"):
        assert (np.asarray(getattr(a, k)) == want[k]).all(), k
    assert a.exploitability == TS.exploitability(x["ranges"][0], want["value"], want["br"], want["valid"], 9) and a.exploitability > 0
