"""GPU tests of the river solver's resuming call (pk_solve_river_resume: include/pokerl_hip.h "Resuming a solve").
Byte for byte throughout.  IDENTITY (i): state given with t0 = 0 changes no other output of the pinned pk_solve_river_resolve.  IDENTITY
(ii): a solve stopped and continued -- 2 + 3, five times 1, 16 + 48 -- leaves the state and every output of the solve that ran through,
with locks, reaches, a gadget's given values and `at`, with two trees in one call, and with every spot of a batch larger than the grid at
its own t0.  The RESTATEMENT (tests/resume_spec.py): the state after 1, 2 and 3 iterations at pools 4, 9, 33 and 46, and a start from a
state beyond both clamps.  What is not read is not read: a sentinel there changes no byte, survives a t0 > 0 call and is 0 after a t0 = 0
call; a refused spot's state is untouched.  The stream form, the Python forms and solve_river_until."""
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
OUT = RU.RIVER_KEYS
ALL = MU.RIVER_KEYS
FF = 0xFF


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


@pytest.fixture(scope="module")
def S():
    from pokerl_amd import solver
    return solver


def five_node_tree(S):
    """player 0 checks to a showdown or bets 50; player 1 folds or calls"""
    return S.RiverTree([0, 4, 1, 3, 4], [[1, 2, FF, FF], [FF] * 4, [3, 4, FF, FF], [FF] * 4, [FF] * 4], [[0, 0], [0, 0], [50, 0], [50, 0], [50, 50]], 100)


def take(x, pick):
    return x if pick is None else {k: (v[pick] if isinstance(v, np.ndarray) else v) for k, v in x.items()}


def call(S, x, iters, t0=None, state=None, pick=None):
    """the device on the spots of x (a dict of arrays with a leading [m], the trees apart); state: (regret, average) or None"""
    y = take(x, pick)
    regret, average = state if state is not None else (None, None)
    return MU.river_call(S, y["board"], y["dead"], y["trees"], y["tree_of"], iters, reach=y["reach"], given=y["given"], at=y["at"], lock=y["lock"],
                         locked=y["locked"], t0=t0, regret=regret, average=average)


def spec(x, iters, t0=None, state=None, pick=None):
    y = take(x, pick)
    regret, average = state if state is not None else (None, None)
    return RM.solve_river_batch(y["board"], None, y["trees"], y["tree_of"], iters, y["lock"], y["locked"], y["dead"], y["reach"], y["given"], y["at"], t0, regret,
                                average)


def chain(S, x, splits, pick=None):
    """a solve in len(splits) calls, from a sentinel state that t0 = 0 must not read -> the last call's dict"""
    m = len(x["board"] if pick is None else pick)
    D = max(len(t.decision_nodes) for t in x["trees"])
    state, done, r = MU.sentinel_state(m, D), 0, None
    for it in splits:
        r = call(S, x, it, np.full(m, done, np.uint32), state, pick)
        state, done = (r["regret"], r["average"]), done + it
    return r


@pytest.fixture(scope="module")
def patterns(PK, S):
    """Pools 4, 9, 33 and 46 on the default tree, the five-node tree and a gadget; locks, reaches above the limit, given values, `at`; a
    refused spot and a tree_of that names no tree between valid ones -- never changed"""
    rng = np.random.default_rng(0x3771)
    pools = [4, 9, 33, 46, 9, 12, 10, 11]
    board, _, dead = VS.random_boards(rng, 8, 5, lambda i: pools[i])
    board[5, 2] = board[5, 0]                                                 # refused, between valid ones
    default, five = PK.river_tree(100, 400), five_node_tree(S)
    trees = [default, five, PK.gadget_tree(five, 1)]
    tree_of = np.array([1, 2, 0, 0, 0, 0, 3, 1], np.uint32)                   # spot 6: no such tree
    at = np.array([0, 1, 3, 2, 0, 0, 0, 4], np.uint8)
    reach = RU.random_reach(rng, board, 5, dead, RS_LIM, over=(3,))
    reach[[5, 6]] = 0xFFFFFFFF
    given = RU.random_given(rng, trees, tree_of, 8)
    lock = LU.lock_of(trees, tree_of, ["none", "none", "none", "none", "p1", "all", "all", [1]])
    locked = LU.random_weights(rng, (8, 14, 4, H))
    x = dict(board=board, dead=dead, trees=trees, tree_of=tree_of, at=at, reach=reach, given=given, lock=lock, locked=locked)
    for v in x.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return x


RS_LIM = (1 << 20) - 1
STATUS = [0, 0, 0, 0, 0, RS.DUP_CARD, 32, 0]


def test_identity_i_state_with_t0_zero_changes_no_other_output(S, patterns):
    x = patterns
    want = RU.river_call(S, x["board"], x["dead"], x["trees"], x["tree_of"], 3, reach=x["reach"], given=x["given"], at=x["at"], lock=x["lock"], locked=x["locked"])
    RU.assert_equal(call(S, x, 3), want, "no state: the resolve call", OUT)
    state = MU.sentinel_state(8, 14)
    got = call(S, x, 3, None, state)                                          # t0 NULL
    RU.assert_equal(got, want, "state, t0 NULL", OUT)
    RU.assert_equal(call(S, x, 3, np.zeros(8, np.uint32), state), got, "state, t0 = 0", ALL)
    assert got["status"].tolist() == STATUS and got["value"][3].any()
    # what a fresh solve leaves: the sentinel at the refused spots, 0 at every other entry that is not read
    read = MU.river_read_mask(x["board"], x["dead"], x["trees"], x["tree_of"], x["lock"])
    for k in ("regret", "average"):
        assert (got[k][[5, 6]] == MU.SENTINEL).all() and not got[k][[0, 1, 2, 3, 4, 7]][~read[[0, 1, 2, 3, 4, 7]]].any(), k
    assert (got["average"][read] >= 0).all() and got["regret"][read].any() and got["average"][7, 0][read[7, 0]].any() and not read[7, 1].any()


@pytest.mark.parametrize("iters", [1, 2, 3])
def test_the_state_equals_the_restatement(S, patterns, iters):
    x = patterns
    state = MU.sentinel_state(8, 14)
    got, want = call(S, x, iters, None, state), spec(x, iters, None, state)
    RU.assert_equal(got, want, "the state after %d iterations" % iters, ALL)
    assert want["valid"][3].sum() == 1035 and want["valid"][2].sum() == 528 and want["t"].tolist() == [iters] * 5 + [0, 0, iters]


@pytest.mark.parametrize("splits", [(2, 3), (1, 1, 1, 1, 1), (16, 48)])
def test_identity_ii_a_solve_stopped_and_continued(S, patterns, splits):
    """... with two trees of different size and a gadget in the call, player 1's rows locked at spot 4, one row at spot 7, reaches, given and at"""
    x = patterns
    pick = None if sum(splits) < 10 else np.array([1, 3, 4, 7])
    want = chain(S, x, (sum(splits),), pick)
    RU.assert_equal(chain(S, x, splits, pick), want, "%r against %d" % (splits, sum(splits)), ALL)
    assert want["regret"].any() and want["strategy"].any()


def test_every_spot_at_its_own_t0_in_a_batch_larger_than_the_grid(S, patterns):
    """six small spots, each present at t0 = 0, 1, 2 and 3 with the state its own one-spot chain left, 312 spots in one call of 2 iterations:
    spot by spot the result of that spot solved alone for t0 + 2 iterations"""
    x = patterns
    rng = np.random.default_rng(0x3772)
    board, _, dead = VS.random_boards(rng, 6, 5, lambda i: 5 + i)
    five = x["trees"][1]
    base = dict(board=board, dead=dead, trees=[five], tree_of=None, at=None, reach=RU.random_reach(rng, board, 5, dead, RS_LIM), given=None, lock=None, locked=None)
    alone = {(b, t): chain(S, base, (t,), np.array([b])) for b in range(6) for t in range(1, 6)}
    b_of, t_of = np.tile(np.arange(6), 52), np.tile(np.repeat(np.arange(4), 6), 13)
    m = len(b_of)
    assert m > S.GRID_MAX and all(t_of[i] != t_of[i + S.GRID_MAX] for i in range(m - S.GRID_MAX))       # a workgroup's second spot: another t0
    regret, average = MU.sentinel_state(m, 2)
    for i in range(m):
        if t_of[i]:
            regret[i], average[i] = alone[(int(b_of[i]), int(t_of[i]))]["regret"][0], alone[(int(b_of[i]), int(t_of[i]))]["average"][0]
    got = call(S, base, 2, t_of.astype(np.uint32), (regret, average), b_of)
    for i in range(m):
        w = alone[(int(b_of[i]), int(t_of[i]) + 2)]
        for k in ("strategy", "value", "br", "status", "regret", "average"):
            assert got[k][i].tobytes() == w[k][0].tobytes(), (i, k)


def test_what_is_not_read_is_not_read_and_survives(S, patterns):
    x = patterns
    first = chain(S, x, (2,))
    read = MU.river_read_mask(x["board"], x["dead"], x["trees"], x["tree_of"], x["lock"])
    t0 = np.full(8, 2, np.uint32)
    want = call(S, x, 3, t0, (first["regret"], first["average"]))
    marked = [np.where(read, first[k], MU.SENTINEL) for k in ("regret", "average")]
    assert (marked[0] != first["regret"]).mean() > 0.3
    got = call(S, x, 3, t0, marked)
    RU.assert_equal(got, want, "a sentinel in every state entry that is not read", OUT)
    for k, mk in zip(("regret", "average"), marked):
        assert (got[k][~read] == MU.SENTINEL).all() and (got[k][read] == want[k][read]).all(), k      # locked rows, rows past D, refused spots ...
    zero = call(S, x, 3, np.zeros(8, np.uint32), marked)
    solved = np.array([0, 1, 2, 3, 4, 7])
    for k in ("regret", "average"):
        assert not zero[k][solved][~read[solved]].any() and (zero[k][[5, 6]] == MU.SENTINEL).all(), k


def test_refusals_leave_the_state_alone_and_disturb_no_neighbour(S, patterns):
    """PK_EQ_BAD_ITER at two spots (t0 + iters = 4097; t0 = 2^32 - 1), a duplicate card, no tree, and a bad `at`, between valid spots"""
    x = dict(patterns)
    at = x["at"].copy()
    at[4] = 200
    x["at"] = at
    first = chain(S, patterns, (2,))
    regret, average = first["regret"].copy(), first["average"].copy()
    regret[[1, 4, 5, 6, 7]], average[[1, 4, 5, 6, 7]] = MU.SENTINEL, -MU.SENTINEL
    t0 = np.array([2, 4095, 0, 2, 2, 0, 5000, 0xFFFFFFFF], np.uint32)
    got = call(S, x, 2, t0, (regret, average))
    assert got["status"].tolist() == [0, RM.BAD_ITER, 0, 0, 32, RS.DUP_CARD, 32, RM.BAD_ITER]
    for i in (1, 4, 5, 6, 7):
        assert not any(got[k][i].any() for k in OUT[:-1]), i
        assert (got["regret"][i] == MU.SENTINEL).all() and (got["average"][i] == -MU.SENTINEL).all(), i
    ok = np.array([0, 2, 3])
    want = call(S, patterns, 2, t0[ok], (regret[ok], average[ok]), ok)
    RU.assert_equal({k: v[ok] for k, v in got.items()}, want, "the neighbours", ALL)
    assert want["status"].tolist() == [0, 0, 0]
    edge = call(S, patterns, 1, np.full(3, 4095, np.uint32), (regret[ok], average[ok]), ok)       # t0 + iters = 4096 is allowed
    assert edge["status"].tolist() == [0, 0, 0]


def test_a_state_beyond_both_clamps_equals_the_restatement(S, patterns):
    x = patterns
    rng = np.random.default_rng(0x3773)
    pick = np.array([0, 1, 7, 2])
    shape = (4, 14, 4, H)
    big = np.iinfo(np.int64)
    regret = rng.choice(np.array([big.min, -1, 0, 12345, RM.RIVER_RMAX, RM.RIVER_RMAX + 1, big.max, 1 << 57], np.int64), shape)
    average = rng.choice(np.array([big.min, -7, 0, 999, RM.RIVER_AMAX, RM.RIVER_AMAX + 1, big.max, 1 << 43], np.int64), shape)
    t0 = np.array([4093, 1, 7, 4000], np.uint32)
    got, want = call(S, x, 3, t0, (regret, average), pick), spec(x, 3, t0, (regret, average), pick)
    RU.assert_equal(got, want, "clamped on the way in", ALL)
    y = take(x, pick)
    read = MU.river_read_mask(y["board"], y["dead"], y["trees"], y["tree_of"], y["lock"])
    assert not got["status"].any() and (got["regret"][read] >= 0).all() and (got["regret"][read] < 1 << 59).all() and (got["average"][read] < 1 << 45).all()
    assert (got["regret"][read] > RM.RIVER_RMAX).any() or (got["regret"][read] == RM.RIVER_RMAX).any()


def test_no_iterations_returns_the_state_as_it_came(S, patterns):
    x = patterns
    first = chain(S, x, (3,))
    again = call(S, x, 0, np.full(8, 3, np.uint32), (first["regret"], first["average"]))
    RU.assert_equal(again, first, "iters = 0 from a state", ALL)
    fresh = call(S, x, 0, None, MU.sentinel_state(8, 14))
    assert not fresh["regret"][[0, 1, 2, 3, 4, 7]].any() and not fresh["average"][[0, 1, 2, 3, 4, 7]].any() and fresh["strategy"][0].any()


def test_the_device_form_on_a_callers_stream_and_the_python_forms(PK, S, patterns):
    from pokerl_amd import hipmem
    x = patterns
    pick = np.array([0, 4, 5, 7, 2])
    y = take(x, pick)
    m, D = len(pick), 14
    first, want = chain(S, x, (2,), pick), chain(S, x, (5,), pick)
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    t0 = np.full(m, 2, np.uint32)
    ins = [hipmem.DeviceBuffer(a.nbytes).upload(a) for a in (y["board"], y["dead"], y["tree_of"], y["lock"], y["locked"], y["reach"], y["given"], y["at"], t0)]
    sizes = dict(strategy=(np.uint16, (m, D, 4, H)), value=(np.int64, (m, 2, H)), br=(np.int64, (m, 2, H)), node_reach=(np.uint32, (m, 2, H)),
                 node_value=(np.int64, (m, 2, H)), node_br=(np.int64, (m, 2, H)), status=(np.uint8, (m,)), regret=(np.int64, (m, D, 4, H)),
                 average=(np.int64, (m, D, 4, H)))
    outs = {k: hipmem.DeviceBuffer(int(np.prod(shape)) * np.dtype(dt).itemsize) for k, (dt, shape) in sizes.items()}
    outs["regret"].upload(first["regret"]); outs["average"].upload(first["average"])
    S.solve_river_d(m, ins[0].ptr, None, y["trees"], 3, dead_d=ins[1].ptr, strategy_d=outs["strategy"].ptr, value_d=outs["value"].ptr, br_d=outs["br"].ptr,
                    status_d=outs["status"].ptr, stream=stream, tree_of=ins[2].ptr, lock=ins[3].ptr, locked=ins[4].ptr, reach=ins[5].ptr, given=ins[6].ptr,
                    at=ins[7].ptr, node_reach_d=outs["node_reach"].ptr, node_value_d=outs["node_value"].ptr, node_br_d=outs["node_br"].ptr,
                    t0_d=ins[8].ptr, regret_d=outs["regret"].ptr, average_d=outs["average"].ptr)
    assert hip.hipStreamSynchronize(stream) == 0
    got = {k: outs[k].download(sizes[k][0], int(np.prod(sizes[k][1]))).reshape(sizes[k][1]) for k in ALL}
    RU.assert_equal(got, want, "the stream form, continued in place", ALL)
    assert hip.hipStreamDestroy(stream) == 0
    for b in ins + list(outs.values()):
        b.free()
    # solve_river_batch: keep_state, then state; solution[i].state is the spot's, cut to its tree's rows
    ok = np.array([0, 4, 7])
    z = take(x, ok)
    kw = dict(tree_of=z["tree_of"], lock=z["lock"], locked=z["locked"], reach=np.minimum(z["reach"], RS_LIM), given=np.where(z["given"] == -1, 0, z["given"]), at=z["at"])
    a = S.solve_river_batch(z["board"], None, z["trees"], 2, z["dead"], keep_state=True, **kw)
    b = S.solve_river_batch(z["board"], None, z["trees"], 3, z["dead"], state=a.state, **kw)
    whole = chain(S, x, (5,), ok)
    RU.assert_equal({k: getattr(b, k) for k in OUT} | dict(regret=b.state.regret, average=b.state.average), whole, "solve_river_batch twice", ALL)
    assert a.state.t.tolist() == [2, 2, 2] and b.state.t.tolist() == [5, 5, 5] and a.state.regret.tobytes() == chain(S, x, (2,), ok)["regret"].tobytes()
    assert b[0].state.regret.shape == (2, 4, H) and b[1].state.regret.shape == (14, 4, H) and int(b[2].state.t) == 5
    assert b.state.nbytes == S.solver_state_bytes(z["trees"], 3) == 2 * 3 * 14 * 4 * H * 8
    plain = S.solve_river_batch(z["board"], None, z["trees"], 5, z["dead"], **kw)
    assert plain.state is None and plain.strategy.tobytes() == b.strategy.tobytes()


@pytest.fixture(scope="module")
def seeded(PK):
    rng = np.random.default_rng(0x3774)
    board, _, dead = VS.random_boards(rng, 2, 5, lambda i: [24, 9][i])
    return dict(board=board, dead=dead, ranges=LU.random_ranges(rng, 2), tree=PK.river_tree(100, 400))


def test_solve_until_follows_the_explicit_chain(S, seeded):
    x = seeded
    explicit, state = [], None
    for _ in range(4):
        r = S.solve_river_batch(x["board"], x["ranges"], x["tree"], 16, x["dead"], state=state, keep_state=True)
        state = r.state
        explicit.append([r[0].exploitability, r[1].exploitability])
    explicit = np.array(explicit)
    assert (np.diff(explicit[:, 0]) < 0).all()                                # the P = 24 spot falls strictly along its steps
    full = S.solve_river_until_batch(x["board"], x["ranges"], x["tree"], 0.0, step=16, max_iters=64, dead=x["dead"])
    assert full.iters == 64 and full.trace.shape == (4, 2) and full.trace.tobytes() == explicit.tobytes()        # never met: stops at max_iters
    assert full.strategy.tobytes() == r.strategy.tobytes() and full.state.regret.tobytes() == state.regret.tobytes() and full.state.t.tolist() == [64, 64]
    target = float(explicit[1].max())                                         # met by both spots at the second step, and not before
    assert explicit[0].max() > target
    early = S.solve_river_until_batch(x["board"], x["ranges"], x["tree"], target, step=16, max_iters=64, dead=x["dead"])
    assert early.iters == 32 and early.trace.tobytes() == explicit[:2].tobytes() and early[1].exploitability == explicit[1, 1]
    short = S.solve_river_until_batch(x["board"], x["ranges"], x["tree"], 0.0, step=16, max_iters=40, dead=x["dead"])
    assert short.iters == 40 and short.trace.shape == (3, 2) and short.trace[:2].tobytes() == explicit[:2].tobytes()   # the last call: 8 iterations
    cards, dead = [int(c) for c in x["board"][0]], int(x["dead"][0])
    one = S.solve_river_until(cards, x["ranges"][0], x["tree"], target, step=16, max_iters=64, dead=dead)
    assert one.trace.ndim == 1 and one.trace[-1] <= target and one.iters == 16 * len(one.trace) and one.trace.tolist() == explicit[:len(one.trace), 0].tolist()
    again = S.solve_river(cards, x["ranges"][0], x["tree"], 8, dead=dead, state=one.state)
    assert int(again.state.t) == one.iters + 8
    with pytest.raises(ValueError, match="exceed 4096"):
        S.solve_river(cards, x["ranges"][0], x["tree"], 4090, dead=dead, state=one.state)
