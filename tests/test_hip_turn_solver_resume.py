"""GPU tests of the turn solver's resuming call (pk_solve_turn_resume: include/pokerl_hip.h "Resuming a solve").
Byte for byte throughout.  IDENTITY (i): state given with t0 = 0 changes no other output of the pinned pk_solve_turn_resolve -- at pools
5, 9 and 12, and at P = 48 with 2 iterations, where the pinned entry point is the reference.  IDENTITY (ii): a solve stopped and continued,
2 + 3 and five times 1 (at P = 48: 1 + 1), with locks at both levels, reaches and `at`, two trees in one call, spots at different t0 in one
call.  The RESTATEMENT (tests/resume_spec.py) at pools 5, 9 and 12: the state of both levels after 1, 2 and 3 iterations, and a start
from a state beyond both clamps.  What is not read is not read, survives a t0 > 0 call and is 0 after a t0 = 0 call -- cards outside the
pool and holdings with the card among it; a refused spot's state is untouched; a locked river-level row's state survives, so the word the
kernel packs that node's probabilities into never leaves.  The stream form, the Python forms and solve_turn_until.
A river-level row costs 4.4 MB per spot and array, so the batch larger than the grid runs on a tree without river-level decisions (its
river-level state is empty); spots at different t0 WITH river-level state run in a batch of six."""
import ctypes as C

import numpy as np
import pytest

import resume_spec as RM
import river_solver_spec as RS
import rvr_spec as VS
import solver_lock_util as LU
import solver_resolve_util as RU
import solver_resume_util as MU
import solver_trees_util as U

pytestmark = pytest.mark.gpu

H = RS.HOLDINGS
OUT = RU.TURN_KEYS
ALL = MU.TURN_KEYS
STATE = ALL[len(OUT):]
FF = 0xFF
LIM = (1 << 17) - 1


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


@pytest.fixture(scope="module")
def S():
    from pokerl_amd import solver
    return solver


def shove_tree(S):
    """player 0 checks or shoves 40, player 1 folds or calls; either way the river card comes and the hand is shown down: no river-level decision"""
    nodes = [(0, [1, 2], (0, 0)), (5, [3], (0, 0)), (1, [4, 5], (40, 0)), (4, [], (0, 0)), (3, [], (40, 0)), (5, [6], (40, 40)), (4, [], (40, 40))]
    return S.TurnTree([k for k, _, _ in nodes], [ch + [FF] * (4 - len(ch)) for _, ch, _ in nodes], [list(p) for _, _, p in nodes], 30)


def take(x, pick):
    return x if pick is None else {k: (v[pick] if isinstance(v, np.ndarray) else v) for k, v in x.items()}


def call(S, x, iters, t0=None, state=None, pick=None, river_strategy=True):
    y = take(x, pick)
    return MU.turn_call(S, y["board"], y["dead"], y["trees"], y["tree_of"], iters, reach=y["reach"], at=y["at"], at_card=y["at_card"], lock=y["lock"],
                        locked=y["locked"], river_lock=y["rlock"], river_locked=y["rlocked"], t0=t0, state=state, river_strategy=river_strategy)


def spec(x, iters, t0=None, state=None, pick=None):
    y = take(x, pick)
    return RM.solve_turn_batch(y["board"], None, y["trees"], y["tree_of"], iters, y["lock"], y["locked"], y["rlock"], y["rlocked"], y["dead"], y["reach"], y["at"],
                               y["at_card"], t0, *(state if state is not None else ()))


def rows_of(x):
    return max(len(t.decision_nodes) for t in x["trees"]), max(len(t.river_decision_nodes) for t in x["trees"])


def chain(S, x, splits, pick=None, river_strategy=True):
    """a solve in len(splits) calls, from a sentinel state that t0 = 0 must not read -> the last call's dict"""
    m = len(x["board"] if pick is None else pick)
    state, done, r = MU.turn_sentinel_state(m, *rows_of(x)), 0, None
    for it in splits:
        r = call(S, x, it, np.full(m, done, np.uint32), state, pick, river_strategy)
        state, done = tuple(r[k] for k in STATE), done + it
    return r


def masks(x, pick=None):
    y = take(x, pick)
    return MU.turn_read_masks(y["board"], y["dead"], y["trees"], y["tree_of"], y["lock"], y["rlock"])


@pytest.fixture(scope="module")
def patterns(PK, S):
    """Pools 5, 9 and 12 on turn_tree(100, 400, (1.0,), 1) and the all-in tree; locks at both levels, reaches above the limit, `at` at a
    river-level node; a refused spot and a tree_of that names no tree between valid ones -- never changed"""
    rng = np.random.default_rng(0x3781)
    pools = [5, 9, 12, 7, 8, 7]
    board, _, dead = VS.random_boards(rng, 6, 4, lambda i: pools[i])
    board = np.ascontiguousarray(board[:, :4])
    board[3, 2] = board[3, 0]                                                 # refused, between valid ones
    big, allin = PK.turn_tree(100, 400, (1.0,), 1), U.allin_turn_tree()
    trees = [big, allin]
    tree_of = np.array([1, 0, 1, 0, 2, 0], np.uint32)                         # spot 4: no such tree
    pool0 = RU.pool_of(board[0], 4, dead[0])
    at = np.array([6, 0, 0, 0, 0, big.river_decision_nodes[0]], np.uint8)
    at_card = np.array([int(VS.CANON[pool0[0]]), FF, FF, FF, FF, int(VS.CANON[RU.pool_of(board[5], 4, dead[5])[-1]])], np.uint8)
    reach = RU.random_reach(rng, board, 4, dead, LIM, over=(1,))
    reach[[3, 4]] = 0xFFFFFFFF
    lock = LU.lock_of(trees, tree_of, ["none", "none", "p1", "all", "all", [0]])
    rlock = LU.lock_of(trees, tree_of, ["none", "none", [1], "all", "all", "p1"], river=True)
    locked, rlocked = LU.random_weights(rng, (6, lock.shape[1], 4, H)), LU.random_weights(rng, (6, rlock.shape[1], 52, 4, H))
    x = dict(board=board, dead=dead, trees=trees, tree_of=tree_of, at=at, at_card=at_card, reach=reach, lock=lock, locked=locked, rlock=rlock, rlocked=rlocked)
    assert rows_of(x) == (4, 12)
    for v in x.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return x


STATUS = [0, 0, 0, RS.DUP_CARD, 32, 0]
SOLVED = np.array([0, 1, 2, 5])


def test_identity_i_and_what_a_fresh_solve_leaves(S, patterns):
    x = patterns
    want = RU.turn_call(S, x["board"], x["dead"], x["trees"], x["tree_of"], 3, reach=x["reach"], at=x["at"], at_card=x["at_card"], lock=x["lock"],
                        locked=x["locked"], river_lock=x["rlock"], river_locked=x["rlocked"])
    RU.assert_equal(call(S, x, 3), want, "no state: the resolve call", OUT)
    got = call(S, x, 3, None, MU.turn_sentinel_state(6, 4, 12))               # t0 NULL
    RU.assert_equal(got, want, "state, t0 NULL", OUT)
    assert got["status"].tolist() == STATUS and got["value"][2].any() and got["node_value"][5].any()
    tm, rm = masks(x)
    for k, read in zip(STATE, (tm, tm, rm, rm)):
        assert (got[k][[3, 4]] == MU.SENTINEL).all() and not got[k][SOLVED][~read[SOLVED]].any() and got[k][read].any(), k
    assert not rm[2, 1].any() and rm[2, 0].any() and rm[5].any() and tm[0].sum() < tm[2].sum()
    same = call(S, x, 3, np.zeros(6, np.uint32), tuple(got[k] for k in STATE))
    RU.assert_equal(same, got, "t0 = 0 reads nothing of a state that is there", ALL)


@pytest.mark.parametrize("iters", [1, 2, 3])
def test_the_state_equals_the_restatement(S, patterns, iters):
    x = patterns
    state = MU.turn_sentinel_state(6, 4, 12)
    got, want = call(S, x, iters, None, state), spec(x, iters, None, state)
    RU.assert_equal(got, want, "the state after %d iterations" % iters, ALL)
    assert want["P"].tolist() == [5, 9, 12, 0, 0, 7] and want["t"].tolist() == [iters, iters, iters, 0, 0, iters]


@pytest.mark.parametrize("splits", [(2, 3), (1, 1, 1, 1, 1)])
def test_identity_ii_a_solve_stopped_and_continued(S, patterns, splits):
    """... two trees of different size in the call, locks at both levels, reaches and a river-level at"""
    x = patterns
    pick = None if len(splits) == 2 else np.array([0, 5, 2])
    want = chain(S, x, (5,), pick)
    RU.assert_equal(chain(S, x, splits, pick), want, "%r against 5" % (splits,), ALL)
    assert want["river_regret"][1].any() and want["river_strategy"].any()


def test_spots_at_different_t0_with_river_level_state(S, patterns):
    """six spots in one call at t0 = 0, 1, 2, 3, 0, 2 -- zeros among them -- each equal to its own single-spot chain"""
    x = patterns
    base, t_of = np.array([0, 1, 2, 5, 1, 0]), [0, 1, 2, 3, 0, 2]
    alone = {(b, t): chain(S, x, (t,), np.array([b]), False) for b, t in set(zip(base.tolist(), t_of)) | {(int(b), t + 1) for b, t in zip(base, t_of)} if t}
    state = [a.copy() for a in MU.turn_sentinel_state(6, 4, 12)]
    for i, (b, t) in enumerate(zip(base.tolist(), t_of)):
        if t:
            for a, k in zip(state, STATE):
                a[i] = alone[(b, t)][k][0]
    got = call(S, x, 1, np.array(t_of, np.uint32), state, base, False)
    for i, (b, t) in enumerate(zip(base.tolist(), t_of)):
        for k in ("strategy", "value", "br", "node_value", "status") + STATE:
            assert got[k][i].tobytes() == alone[(b, t + 1)][k][0].tobytes(), (i, k)


def test_every_spot_at_its_own_t0_in_a_batch_larger_than_the_grid(S):
    """five small spots on the tree without river-level decisions, each at t0 = 0 .. 3, 260 spots in one call of 2 iterations"""
    rng = np.random.default_rng(0x3782)
    board, _, dead = VS.random_boards(rng, 5, 4, lambda i: 5 + i)
    board = np.ascontiguousarray(board[:, :4])
    base = dict(board=board, dead=dead, trees=[shove_tree(S)], tree_of=None, at=None, at_card=None, reach=RU.random_reach(rng, board, 4, dead, LIM), lock=None,
                locked=None, rlock=None, rlocked=None)
    assert rows_of(base) == (2, 0)
    alone = {(b, t): chain(S, base, (t,), np.array([b])) for b in range(5) for t in range(1, 6)}
    b_of, t_of = np.tile(np.arange(5), 52), np.tile(np.repeat(np.arange(4), 5), 13)
    m, grid = len(b_of), S.turn_grid(base["trees"])
    assert m > grid and all(t_of[i] != t_of[i + grid] for i in range(m - grid))
    state = [a.copy() for a in MU.turn_sentinel_state(m, 2, 0)]
    for i in range(m):
        if t_of[i]:
            state[0][i], state[1][i] = alone[(int(b_of[i]), int(t_of[i]))]["regret"][0], alone[(int(b_of[i]), int(t_of[i]))]["average"][0]
    got = call(S, base, 2, t_of.astype(np.uint32), state, b_of)
    for i in range(m):
        w = alone[(int(b_of[i]), int(t_of[i]) + 2)]
        for k in ("strategy", "value", "br", "status", "regret", "average"):
            assert got[k][i].tobytes() == w[k][0].tobytes(), (i, k)
    assert got["regret"].any() and not got["status"].any()


def test_what_is_not_read_survives_and_refusals_leave_the_state_alone(S, patterns):
    """a sentinel in every entry that is not read -- locked rows of both levels, rows past the small tree's, cards outside the pool, holdings
    with the card, the refused spots -- changes no byte and is still there after a t0 > 0 call; PK_EQ_BAD_ITER and a bad at_card beside them"""
    x = dict(patterns)
    first = chain(S, x, (2,))
    tm, rm = masks(x)
    marked = [np.where(read, first[k], MU.SENTINEL) for k, read in zip(STATE, (tm, tm, rm, rm))]
    t0 = np.full(6, 2, np.uint32)
    want = call(S, x, 2, t0, tuple(first[k] for k in STATE))
    got = call(S, x, 2, t0, marked)
    RU.assert_equal(got, want, "a sentinel in every state entry that is not read", OUT)
    for k, read in zip(STATE, (tm, tm, rm, rm)):
        assert (got[k][~read] == MU.SENTINEL).all() and (got[k][read] == want[k][read]).all(), k
    assert (got["river_regret"][5][~rm[5]] == MU.SENTINEL).all() and rm[5].sum() < rm[5].size // 4          # the locked river-level rows of spot 5 among them
    zero = call(S, x, 2, np.zeros(6, np.uint32), marked)
    for k, read in zip(STATE, (tm, tm, rm, rm)):
        assert not zero[k][SOLVED][~read[SOLVED]].any() and (zero[k][[3, 4]] == MU.SENTINEL).all(), k
    at_card = x["at_card"].copy()
    at_card[0] = int(x["board"][0, 1])                                        # a board card: no card of the pool
    x["at_card"] = at_card
    t0 = np.array([2, 4095, 2, 0, 9, 0xFFFFFFFF], np.uint32)
    bad = call(S, x, 2, t0, marked)
    assert bad["status"].tolist() == [RS.BAD_CARD, RM.BAD_ITER, 0, RS.DUP_CARD, 32, RM.BAD_ITER]
    for i in (0, 1, 3, 4, 5):
        assert not any(bad[k][i].any() for k in OUT[:-1]) and all(bad[k][i].tobytes() == marked[j][i].tobytes() for j, k in enumerate(STATE)), i
    for k in ALL:
        assert bad[k][2].tobytes() == got[k][2].tobytes(), k                  # the neighbour


def test_a_state_beyond_both_clamps_equals_the_restatement(S, patterns):
    x = patterns
    rng = np.random.default_rng(0x3783)
    pick = np.array([0, 2, 5])
    big = np.iinfo(np.int64)
    rv = np.array([big.min, -1, 0, 12345, RM.TURN_RMAX, RM.TURN_RMAX + 1, big.max, 1 << 59], np.int64)
    av = np.array([big.min, -7, 0, 999, RM.TURN_AMAX, RM.TURN_AMAX + 1, big.max, 1 << 40], np.int64)
    state = (rng.choice(rv, (3, 4, 4, H)), rng.choice(av, (3, 4, 4, H)), rng.choice(rv, (3, 12, 52, 4, H)), rng.choice(av, (3, 12, 52, 4, H)))
    t0 = np.array([4093, 1, 4000], np.uint32)
    got, want = call(S, x, 3, t0, state, pick), spec(x, 3, t0, state, pick)
    RU.assert_equal(got, want, "clamped on the way in", ALL)
    tm, rm = masks(x, pick)
    assert not got["status"].any() and (got["regret"][tm] >= 0).all() and (got["river_regret"][rm] < 1 << 61).all() and (got["river_average"][rm] < 1 << 42).all()


def test_no_iterations_returns_the_state_as_it_came(S, patterns):
    x = patterns
    pick = np.array([0, 5])
    first = chain(S, x, (3,), pick)
    again = call(S, x, 0, np.full(2, 3, np.uint32), tuple(first[k] for k in STATE), pick)
    RU.assert_equal(again, first, "iters = 0 from a state", ALL)


def test_p48_through_the_pinned_entry_point(PK, S):
    """the largest pool: identity (i) against pk_solve_turn_resolve at 2 iterations, identity (ii) as 1 + 1, on the all-in tree"""
    rng = np.random.default_rng(0x3784)
    board, _, dead = VS.random_boards(rng, 1, 4, 48)
    board = np.ascontiguousarray(board[:, :4])
    x = dict(board=board, dead=dead, trees=[U.allin_turn_tree()], tree_of=None, at=np.array([6], np.uint8), at_card=np.array([int(VS.CANON[RU.pool_of(board[0], 4, dead[0])[20]])], np.uint8),
             reach=RU.random_reach(rng, board, 4, dead, LIM), lock=None, locked=None, rlock=None, rlocked=None)
    want = RU.turn_call(S, board, dead, x["trees"], None, 2, reach=x["reach"], at=x["at"], at_card=x["at_card"])
    whole, split = chain(S, x, (2,)), chain(S, x, (1, 1))
    RU.assert_equal(whole, want, "state with t0 = 0 at P = 48", OUT)
    RU.assert_equal(split, whole, "1 + 1 at P = 48", ALL)
    tm, rm = masks(x)
    assert want["status"][0] == 0 and tm[0, 0, 0].sum() == 1128 and rm[0, 0, RU.pool_of(board[0], 4, dead[0])[20], 0].sum() == 1081 and whole["river_average"][rm].any()
    assert not whole["river_average"][~rm].any() and not whole["regret"][~tm].any() and whole["regret"][tm].any()    # (a forced check has no regret)


def test_the_device_form_on_a_callers_stream_and_the_python_forms(PK, S, patterns):
    from pokerl_amd import hipmem
    x = patterns
    pick = np.array([0, 3, 5])
    y = take(x, pick)
    m, Dt, Dr = 3, 4, 12
    first, want = chain(S, x, (2,), pick), chain(S, x, (5,), pick)
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    y["t0"] = np.full(m, 2, np.uint32)
    names = ("board", "dead", "tree_of", "lock", "locked", "rlock", "rlocked", "reach", "at", "at_card", "t0")
    ins = {k: hipmem.DeviceBuffer(y[k].nbytes).upload(np.ascontiguousarray(y[k])) for k in names}
    sizes = dict(strategy=(np.uint16, (m, Dt, 4, H)), river_strategy=(np.uint16, (m, Dr, 52, 4, H)), value=(np.int64, (m, 2, H)), br=(np.int64, (m, 2, H)),
                 node_reach=(np.uint32, (m, 2, H)), node_value=(np.int64, (m, 2, H)), node_br=(np.int64, (m, 2, H)), status=(np.uint8, (m,)),
                 regret=(np.int64, (m, Dt, 4, H)), average=(np.int64, (m, Dt, 4, H)), river_regret=(np.int64, (m, Dr, 52, 4, H)),
                 river_average=(np.int64, (m, Dr, 52, 4, H)))
    outs = {k: hipmem.DeviceBuffer(int(np.prod(shape)) * np.dtype(dt).itemsize) for k, (dt, shape) in sizes.items()}
    for k in STATE:
        outs[k].upload(first[k])
    S.solve_turn_d(m, ins["board"].ptr, None, y["trees"], 3, dead_d=ins["dead"].ptr, strategy_d=outs["strategy"].ptr, river_strategy_d=outs["river_strategy"].ptr,
                   value_d=outs["value"].ptr, br_d=outs["br"].ptr, status_d=outs["status"].ptr, stream=stream, tree_of=ins["tree_of"].ptr, lock=ins["lock"].ptr,
                   locked=ins["locked"].ptr, river_lock=ins["rlock"].ptr, river_locked=ins["rlocked"].ptr, reach=ins["reach"].ptr, at=ins["at"].ptr,
                   at_card=ins["at_card"].ptr, node_reach_d=outs["node_reach"].ptr, node_value_d=outs["node_value"].ptr, node_br_d=outs["node_br"].ptr,
                   t0_d=ins["t0"].ptr, regret_d=outs["regret"].ptr, average_d=outs["average"].ptr, river_regret_d=outs["river_regret"].ptr,
                   river_average_d=outs["river_average"].ptr)
    assert hip.hipStreamSynchronize(stream) == 0
    got = {k: outs[k].download(sizes[k][0], int(np.prod(sizes[k][1]))).reshape(sizes[k][1]) for k in sizes}
    RU.assert_equal(got, want, "the stream form, continued in place", ALL)
    assert hip.hipStreamDestroy(stream) == 0
    for b in list(ins.values()) + list(outs.values()):
        b.free()
    ok = np.array([0, 5])
    z = take(x, ok)
    kw = dict(tree_of=z["tree_of"], lock=z["lock"], locked=z["locked"], river_lock=z["rlock"], river_locked=z["rlocked"], reach=np.minimum(z["reach"], LIM),
              at=z["at"], at_card=z["at_card"], river_strategy=True)
    a = S.solve_turn_batch(z["board"], None, z["trees"], 2, z["dead"], keep_state=True, **kw)
    b = S.solve_turn_batch(z["board"], None, z["trees"], 3, z["dead"], state=a.state, **kw)
    whole = chain(S, x, (5,), ok)
    RU.assert_equal({k: getattr(b, k) for k in OUT} | {k: getattr(b.state, k) for k in STATE}, whole, "solve_turn_batch twice", ALL)
    assert a.state.t.tolist() == [2, 2] and b.state.t.tolist() == [5, 5] and b[0].state.river_regret.shape == (2, 52, 4, H) and b[1].state.regret.shape == (4, 4, H)
    assert b.state.nbytes == S.solver_state_bytes(z["trees"], 2) == 2 * 2 * (4 + 52 * 12) * 4 * H * 8


def test_solve_until_follows_the_explicit_chain(PK, S):
    rng = np.random.default_rng(0x3785)
    board, _, dead = VS.random_boards(rng, 2, 4, lambda i: [10, 8][i])
    board = np.ascontiguousarray(board[:, :4])
    ranges, tree = LU.random_ranges(rng, 2), U.allin_turn_tree()
    explicit, state = [], None
    for _ in range(3):
        r = S.solve_turn_batch(board, ranges, tree, 8, dead, state=state, keep_state=True)
        state = r.state
        explicit.append([r[0].exploitability, r[1].exploitability])
    explicit = np.array(explicit)
    full = S.solve_turn_until_batch(board, ranges, tree, -1.0, step=8, max_iters=24, dead=dead)
    assert full.iters == 24 and full.trace.tobytes() == explicit.tobytes() and full.strategy.tobytes() == r.strategy.tobytes()      # never met: max_iters
    assert full.state.river_regret.tobytes() == state.river_regret.tobytes() and full.state.t.tolist() == [24, 24]
    step = int(np.argmax((explicit <= explicit[1].max()).all(axis=1)))        # the first step at which both spots are at or under the target
    early = S.solve_turn_until_batch(board, ranges, tree, float(explicit[1].max()), step=8, max_iters=24, dead=dead)
    assert early.iters == 8 * (step + 1) and early.trace.tobytes() == explicit[:step + 1].tobytes()
    short = S.solve_turn_until_batch(board, ranges, tree, -1.0, step=8, max_iters=12, dead=dead)
    assert short.iters == 12 and short.trace.shape == (2, 2) and short.trace[0].tobytes() == explicit[0].tobytes()
    one = S.solve_turn_until([int(c) for c in board[1]], ranges[1], tree, float(explicit[0, 1]), step=8, max_iters=24, dead=int(dead[1]))
    assert one.iters == 8 and one.trace.tolist() == [explicit[0, 1]] and int(one.state.t) == 8
