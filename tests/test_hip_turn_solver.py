"""GPU tests of the turn solver (pk_solve_turn: DESIGN.md section 3.13): EVERY output of every case equals the numpy spec
(turn_solver_spec.py) bit for bit, river_strategy included where P <= 20 -- the smallest pools, the edges of the sort pad and of the slots
a lane owns (live spec up to P = 34; P = 45 .. 48 and the magnitude edge through the spec's fixtures, tests/golden/turn_solver), a 128-node
tree, an empty range -- plus the identity with range vs range on check, check, deal, check, check, batches larger than the grid (also where
the work-space ceiling makes the grid small), bad spots inside good batches, the stream form, and convergence."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

import rvr_spec as VS
import turn_solver_spec as TS

pytestmark = pytest.mark.gpu

H = TS.HOLDINGS
KEYS = ("strategy", "value", "br", "status", "valid")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "turn_solver")
FF = 0xFF


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


def custom_tree(kind, child, put, pot):
    from pokerl_amd.solver import TurnTree
    return TurnTree(kind, [list(c) + [FF] * (4 - len(c)) for c in child], put, pot)


def small_tree(PK):
    """20 nodes: one bet size, one bet a street; the river bet is all-in"""
    t = PK.turn_tree(100, 50, (0.5,), 1)
    assert t.n == 20
    return t


def EC():
    """tools/host_sim/equity_cases.py: the hand-made tree with a four-action root (turn_feature_tree) lives beside the CPU cases"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = os.path.join(root, "tools", "host_sim")
    if p not in sys.path:
        sys.path.insert(0, p)
    import equity_cases
    return equity_cases


def checked_down_tree(pot):
    """check, check, deal, check, check, showdown: one action at every node"""
    return custom_tree([0, 1, 5, 0, 1, 4], [[1], [2], [3], [4], [5], []], [[0, 0]] * 6, pot)


def chain_tree(pot=60):
    """128 nodes: 31 turn-level decisions in turn (fold, or raise 10 on top of the call; the last one folds or calls), the river card,
    then 32 river-level decisions of the same kind and a showdown"""
    kind, child, put = [0], [[]], [[0, 0]]
    node, p, puts = 0, 0, [0, 0]
    for street, count in ((0, 31), (1, 32)):
        for d in range(count):
            fold, nxt = len(kind), len(kind) + 1
            child[node] = [fold, nxt]
            kind.append(2 + p); child.append([]); put.append(list(puts))
            puts = list(puts)
            last = d == count - 1
            puts[p] = max(puts) if last else max(puts) + 10
            kind.append((5 if street == 0 else 4) if last else 1 - p); child.append([]); put.append(list(puts))
            node, p = nxt, 1 - p
        if street == 0:                                                       # the chance node's child: player 0 opens the river
            child[node] = [len(kind)]
            kind.append(0); child.append([]); put.append(list(puts))
            node, p = len(kind) - 1, 0
    assert len(kind) == 128, len(kind)
    return custom_tree(kind, child, put, pot)


def random_ranges(rng, m):
    w = rng.integers(0, 65536, (m, 2, H)).astype(np.uint16)
    for row in w.reshape(-1, H):
        row[rng.integers(0, H, 200)] = 0
        row[rng.integers(0, H, 100)] = 65535
    return w


def invariants(out):
    v = out["valid"]
    assert out["strategy"].dtype == np.uint16 and out["value"].dtype == np.int64 and out["br"].dtype == np.int64
    assert (out["strategy"].astype(np.int64).sum(axis=2).transpose(0, 2, 1)[v] == TS.ONE).all()          # every valid row sums to ONE
    assert not out["strategy"].transpose(0, 3, 1, 2)[~v].any()
    for k in ("value", "br"):
        assert not out[k].transpose(0, 2, 1)[~v].any()
    assert (out["br"] >= out["value"]).all()
    assert not v[out["status"] != 0].any()


def device_solve(board, ranges, tree, iters, dead=None, river=False):
    from pokerl_amd import solver as S
    r = S.solve_turn_batch(np.ascontiguousarray(board[:, :4]), ranges, tree, iters, dead, river_strategy=river)
    out = {k: np.asarray(getattr(r, k)) for k in KEYS}
    if river:
        out["river_strategy"] = r.river_strategy
    out["P"] = np.asarray(r.pool)
    invariants(out)
    return out


def assert_equal(got, want, where, keys=KEYS):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype and (a == b).all(), (where, k, np.argwhere(a != b)[:4].tolist())


def check_against_spec(rng, pools, tree, iters, ranges=None, where=""):
    board, _, dead = VS.random_boards(rng, len(pools), 4, lambda i: pools[i])
    ranges = random_ranges(rng, len(pools)) if ranges is None else ranges
    river = max(pools) <= 20
    got = device_solve(board, ranges, tree, iters, dead, river)
    assert not got["status"].any() and (got["valid"].sum(axis=1) == [p * (p - 1) // 2 for p in pools]).all() and (got["P"] == pools).all()
    assert_equal(got, TS.solve_batch(board[:, :4], ranges, tree, iters, dead), where, KEYS + (("river_strategy",) if river else ()))
    return got


@pytest.mark.parametrize("iters", [1, 2, 33])
def test_the_smallest_pools(PK, iters):
    """P = 5: ten holdings, three disjoint partners each, one river card for a pair of them"""
    rng = np.random.default_rng(500 + iters)
    check_against_spec(rng, [5, 6, 7], PK.turn_tree(100, 400, (1.0,), 1), iters, where="P = 5 .. 7, %d iterations" % iters)


@pytest.mark.parametrize("pool", [32, 33, 34])
def test_pools_around_the_sort_pad_and_the_slots_a_lane_owns(PK, pool):
    """496 / 528 / 561 turn holdings and 465 / 496 / 528 under a card: the 512-edge of the sort pad and of a lane owning one or two"""
    rng = np.random.default_rng(510 + pool)
    check_against_spec(rng, [pool], small_tree(PK), 2, where="small tree")
    check_against_spec(rng, [pool], EC().turn_feature_tree(), 2, where="four actions")


def fixture(name):
    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    return fx, fx["board"][None].copy(), np.array([fx["dead"]], np.uint64), fx["ranges"][None].copy()


@pytest.mark.parametrize("name", ["p45", "p46", "p47", "p48", "magnitude"])
def test_the_largest_pools_and_the_magnitude_edge_through_the_specs_fixtures(PK, name):
    """990 .. 1128 turn holdings, 946 .. 1081 under a card: the 1024- and 1088-edges; `magnitude`: every weight 65 535, pot + put = 8191"""
    fx, board, dead, ranges = fixture(name)
    tree = PK.turn_tree(int(fx["pot"]), int(fx["stack"]), (1.0,), 1)
    assert tree.n == 36 and tree.n - int(tree.river_level.sum()) == 9
    if name == "magnitude":
        assert tree.pot + int(tree.put.max()) == 8191 and (ranges == 65535).all() and int(fx["regret_bits"]) <= 60
    got = device_solve(board, ranges, tree, int(fx["iters"]), dead, river=True)
    want = dict(strategy=fx["strategy"][None], value=fx["value"][None], br=fx["br"][None], status=fx["status"][None])
    assert_equal(got, want, name, ("strategy", "value", "br", "status"))
    assert hashlib.sha256(np.ascontiguousarray(got["river_strategy"][0]).tobytes()).hexdigest() == str(fx["river_sha256"])


def test_checked_down_is_range_vs_range_on_the_turn_board(PK):
    """No spec involved: on check, check, deal, check, check, showdown value[p][h] = br[p][h] = 2 (2 pot win[h] + pot tie[h]) with win / tie
    of range vs range on the four-card board against w_{1-p} (its counts run over the P - 4 river cards; the reach is weight << 1)."""
    from pokerl_amd import judger as J
    rng = np.random.default_rng(520)
    pot = 120
    board, nboard, dead = VS.random_boards(rng, 3, 4, lambda i: (48, 33, 10)[i])
    ranges = random_ranges(rng, 3)
    got = device_solve(board, ranges, checked_down_tree(pot), 2, dead)
    for p in (0, 1):
        r = J.range_vs_range_batch(board, nboard, dead, ranges[:, 1 - p])
        want = 2 * (2 * pot * r.win.astype(np.int64) + pot * r.tie.astype(np.int64))
        assert (got["value"][:, p] == want).all() and (got["br"][:, p] == want).all(), p


def test_a_128_node_tree(PK):
    rng = np.random.default_rng(530)
    check_against_spec(rng, [6, 9], chain_tree(), 2, where="128 nodes")


def test_one_range_all_zero(PK):
    rng = np.random.default_rng(540)
    ranges = random_ranges(rng, 2)
    ranges[0, 1] = 0
    ranges[1, 0] = 0
    got = check_against_spec(rng, [20, 12], small_tree(PK), 2, ranges=ranges, where="an empty range")
    assert not got["value"][0, 0].any() and not got["value"][1, 1].any()      # nobody to meet


def more_spots_than(PK, tree, grid, pool, seed):
    rng = np.random.default_rng(seed)
    m = 2 * grid + 1
    board, _, dead = VS.random_boards(rng, m, 4, pool)
    ranges = random_ranges(rng, m)
    for i in (grid, 2 * grid):
        board[i], dead[i], ranges[i] = board[0], dead[0], ranges[0]
    got = device_solve(board, ranges, tree, 2, dead)
    for k in KEYS:
        assert got[k][0].tobytes() == got[k][grid].tobytes() == got[k][2 * grid].tobytes(), k
    return board, dead, ranges, got


def test_more_spots_than_the_grid(PK):
    """m = 513 at P = 5 on the small tree, where the grid is 256: every spot equals the spec"""
    from pokerl_amd import solver as S
    tree = small_tree(PK)
    assert S.turn_grid(tree) == 256
    board, dead, ranges, got = more_spots_than(PK, tree, 256, 5, 550)
    assert_equal(got, TS.solve_batch(board[:, :4], ranges, tree, 2, dead), "513 spots")


def test_more_spots_than_the_grid_the_work_space_allows(PK):
    """a 128-node tree: the 4 GiB ceiling makes the grid smaller than 256; m = 2 grid + 1 at P = 5, a sample of spots against the spec"""
    from pokerl_amd import solver as S
    tree = chain_tree()
    grid = S.turn_grid(tree)
    assert 16 <= grid < 256, grid
    board, dead, ranges, got = more_spots_than(PK, tree, grid, 5, 560)
    pick = [0, 1, grid - 1, grid, grid + 1, 2 * grid - 1, 2 * grid]
    want = TS.solve_batch(board[pick, :4], ranges[pick], tree, 2, dead[pick])
    assert_equal({k: got[k][pick] for k in KEYS}, want, "2 grid + 1 spots")


def test_status_inside_a_good_batch_alone_and_no_spots(PK):
    from pokerl_amd import _lib as L
    from pokerl_amd import solver as S
    rng = np.random.default_rng(570)
    m = 7
    board, _, dead = VS.random_boards(rng, m, 4, lambda i: 9)
    board = np.ascontiguousarray(board[:, :4])
    ranges = random_ranges(rng, m)
    board[1, 2] = 0x3D                                                        # no card
    board[3, 3] = board[3, 0]                                                 # the same card twice
    dead[5] = np.uint64(((1 << 52) - 1) & ~0b1111)                            # four cards are not dead: no river card
    dead[6] |= np.uint64(1 << 60)                                             # a dead bit that is no card
    tree = small_tree(PK)
    got = device_solve(board, ranges, tree, 3, dead, river=True)
    want = TS.solve_batch(board, ranges, tree, 3, dead)
    assert (want["status"][[1, 3, 6]] == [TS.BAD_CARD, TS.DUP_CARD, TS.BAD_CARD]).all() and want["status"][5] & TS.SMALL_POOL
    assert_equal(got, want, "bad spots inside a good batch", KEYS + ("river_strategy",))
    status = np.full(m, 7, np.uint8)
    L.check(L.lib().pk_solve_turn(0, m, L.ptr(board), L.ptr(dead), L.ptr(ranges), *S._tree_args(tree), 3, None, None, None, None, L.ptr(status)))
    assert (status == got["status"]).all()
    value, status = np.full((m, 2, H), 7, np.int64), np.full(m, 7, np.uint8)
    L.check(L.lib().pk_solve_turn(0, 0, L.ptr(board), L.ptr(dead), L.ptr(ranges), *S._tree_args(tree), 3, None, None, L.ptr(value), None, L.ptr(status)))
    assert (value == 7).all() and (status == 7).all()


def test_the_device_form_on_a_callers_stream(PK):
    from pokerl_amd import hipmem
    from pokerl_amd import solver as S
    rng = np.random.default_rng(580)
    m = 4
    board, _, dead = VS.random_boards(rng, m, 4, lambda i: (48, 30, 5, 9)[i])
    board = np.ascontiguousarray(board[:, :4])
    ranges = random_ranges(rng, m)
    tree = small_tree(PK)
    Dt, Dr = len(tree.decision_nodes), len(tree.river_decision_nodes)
    want = device_solve(board, ranges, tree, 3, dead, river=True)
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0              # hipStreamNonBlocking: a caller's own stream
    ins = [hipmem.DeviceBuffer(x.nbytes).upload(x) for x in (board, dead, ranges)]
    outs = [hipmem.DeviceBuffer(n) for n in (m * Dt * 4 * H * 2, m * Dr * 52 * 4 * H * 2, m * 2 * H * 8, m * 2 * H * 8, m)]
    for rep in range(2):                                                      # (the second call reuses the stream's work space)
        S.solve_turn_d(m, ins[0].ptr, ins[2].ptr, tree, 3, dead_d=ins[1].ptr, strategy_d=outs[0].ptr, river_strategy_d=outs[1].ptr,
                       value_d=outs[2].ptr, br_d=outs[3].ptr, status_d=outs[4].ptr, stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        assert (outs[0].download(np.uint16, m * Dt * 4 * H).reshape(m, Dt, 4, H) == want["strategy"]).all()
        assert (outs[1].download(np.uint16, m * Dr * 52 * 4 * H).reshape(m, Dr, 52, 4, H) == want["river_strategy"]).all()
        assert (outs[2].download(np.int64, m * 2 * H).reshape(m, 2, H) == want["value"]).all()
        assert (outs[3].download(np.int64, m * 2 * H).reshape(m, 2, H) == want["br"]).all()
        assert (outs[4].download(np.uint8, m) == want["status"]).all()
    assert hip.hipStreamDestroy(stream) == 0
    for x in ins + outs:
        x.free()


def test_convergence(PK):
    """One seeded P = 16 spot: the device exploitability at 16, 64 and 256 iterations is strictly decreasing, and at 256 iterations every
    output equals the spec's."""
    from pokerl_amd import solver as S
    rng = np.random.default_rng(590)
    board, _, dead = VS.random_boards(rng, 1, 4, 16)
    board = np.ascontiguousarray(board[:, :4])
    ranges = random_ranges(rng, 1)
    tree = small_tree(PK)
    sols = {it: S.solve_turn_batch(board, ranges, tree, it, dead) for it in (16, 64, 256)}
    expl = [sols[it][0].exploitability for it in (16, 64, 256)]
    print("exploitability at 16, 64, 256 iterations:", expl)
    assert expl[0] > expl[1] > expl[2] > 0
    want = TS.solve_batch(board, ranges, tree, 256, dead)
    assert_equal({k: np.asarray(getattr(sols[256], k)) for k in KEYS}, want, "256 iterations")
    assert expl[2] == TS.exploitability(ranges[0], want["value"][0], want["br"][0], want["valid"][0], 16)
