"""GPU tests of the river solver (pk_solve_river: DESIGN.md section 3.12): EVERY output of every case equals the numpy spec
(river_solver_spec.py) bit for bit -- pools around the edges of the sort pad and of the positions a lane owns, the forced tree, a
four-action node, a 64-node tree, the default tree, the magnitude edge, an empty range -- plus the identity with range vs range on the
forced tree, batches larger than the persistent grid, bad spots inside good batches, the stream form, and convergence."""
import ctypes as C

import numpy as np
import pytest

import river_solver_spec as RS
import rvr_spec as VS

pytestmark = pytest.mark.gpu

H = RS.HOLDINGS
KEYS = ("strategy", "value", "br", "status", "valid")


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


def custom_tree(kind, child, put, pot):
    from pokerl_amd.solver import RiverTree
    rows = [list(c) + [0xFF] * (4 - len(c)) for c in child]
    return RiverTree(kind, rows, put, pot)


def forced_tree(pot):
    """check, check, showdown: one action at every node"""
    return custom_tree([0, 1, 4], [[1], [2], []], [[0, 0]] * 3, pot)


def four_action_tree(pot=100):
    """player 0 checks to a showdown or bets 50, 100 or 200; player 1 folds or calls: 11 nodes"""
    kind, child, put = [0, 4], [[1, 2, 3, 4], []], [[0, 0], [0, 0]]
    for bet in (50, 100, 200):
        kind.append(1); child.append([]); put.append([bet, 0])
    for i, bet in enumerate((50, 100, 200)):
        child[2 + i] = [len(kind), len(kind) + 1]
        kind += [3, 4]; child += [[], []]; put += [[bet, 0], [bet, bet]]
    return custom_tree(kind, child, put, pot)


def chain_tree(pot=60):
    """64 nodes: a forced first node, then 31 decisions in turn, each a fold or a raise of 10 on top of the call; the last one folds or calls"""
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
    return custom_tree(kind, child, put, pot)


def random_ranges(rng, m):
    w = rng.integers(0, 65536, (m, 2, H)).astype(np.uint16)
    for row in w.reshape(-1, H):
        row[rng.integers(0, H, 200)] = 0
        row[rng.integers(0, H, 100)] = 65535
    return w


def as_dict(r):
    return {k: np.asarray(getattr(r, k)) for k in KEYS}


def invariants(out):
    v = out["valid"]
    assert out["strategy"].dtype == np.uint16 and out["value"].dtype == np.int64 and out["br"].dtype == np.int64
    assert (out["strategy"].astype(np.int64).sum(axis=2).transpose(0, 2, 1)[v] == RS.ONE).all()          # every valid row sums to ONE
    assert not out["strategy"].transpose(0, 3, 1, 2)[~v].any()
    for k in ("value", "br"):
        assert not out[k].transpose(0, 2, 1)[~v].any()
    assert (out["br"] >= out["value"]).all()
    assert not v[out["status"] != 0].any()


def device_solve(board, ranges, tree, iters, dead=None):
    from pokerl_amd import solver as S
    out = as_dict(S.solve_river_batch(board, ranges, tree, iters, dead))
    invariants(out)
    return out


def assert_equal(got, want, where):
    for k in KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype and (a == b).all(), (where, k, np.argwhere(a != b)[:4].tolist())


def check_against_spec(rng, pools, tree, iters, ranges=None, where=""):
    board, _, dead = VS.random_boards(rng, len(pools), 5, lambda i: pools[i])
    ranges = random_ranges(rng, len(pools)) if ranges is None else ranges
    got = device_solve(board, ranges, tree, iters, dead)
    assert not got["status"].any() and (got["valid"].sum(axis=1) == [p * (p - 1) // 2 for p in pools]).all()
    assert_equal(got, RS.solve_batch(board, ranges, tree, iters, dead), where)
    return got


def test_the_smallest_pool_on_the_default_tree(PK):
    """P = 4: six holdings, one disjoint partner each; 33 iterations, and 1 and 2"""
    rng = np.random.default_rng(401)
    tree = PK.river_tree(100, 400)
    assert tree.n == 39
    for iters in (1, 2, 33):
        check_against_spec(rng, [4, 5, 6], tree, iters, where="P = 4 .. 6, %d iterations" % iters)


@pytest.mark.parametrize("pools", [(32, 33), (45, 46)])
def test_pools_around_the_sort_pad_and_the_positions_a_lane_owns(PK, pools):
    """496 / 528 and 990 / 1035 holdings: the 512- and 1024-edges of the sort pad and of a lane owning one, two or three positions"""
    rng = np.random.default_rng(402 + pools[0])
    check_against_spec(rng, list(pools), PK.river_tree(100, 400), 2, where="default tree")
    check_against_spec(rng, list(pools), four_action_tree(), 3, where="four actions")


def test_the_full_pool(PK):
    rng = np.random.default_rng(403)
    check_against_spec(rng, [47], forced_tree(77), 1, where="forced tree")
    check_against_spec(rng, [47], four_action_tree(), 2, where="four actions")
    check_against_spec(rng, [47], PK.river_tree(100, 50), 8, where="9 nodes, 8 iterations")


def test_the_magnitude_edge(PK):
    """every weight 65 535 and pot + put = 8191, full pool"""
    rng = np.random.default_rng(404)
    tree = PK.river_tree(1001, 7190, bet_fractions=(8.0,), max_raises=1)
    assert tree.n == 9 and tree.pot + int(tree.put.max()) == 8191
    check_against_spec(rng, [47], tree, 8, ranges=np.full((1, 2, H), 65535, np.uint16), where="magnitude edge")


def test_a_64_node_tree_and_a_forced_node(PK):
    rng = np.random.default_rng(405)
    check_against_spec(rng, [9, 12], chain_tree(), 2, where="64 nodes")
    check_against_spec(rng, [9, 33], forced_tree(100), 33, where="forced tree")


def test_one_range_all_zero(PK):
    rng = np.random.default_rng(406)
    ranges = random_ranges(rng, 2)
    ranges[0, 1] = 0
    ranges[1, 0] = 0
    got = check_against_spec(rng, [33, 20], PK.river_tree(100, 400), 2, ranges=ranges, where="an empty range")
    assert not got["value"][0, 0].any() and not got["value"][1, 1].any()      # nobody to meet


def test_the_forced_tree_is_range_vs_range(PK):
    """No spec involved: on check-check-showdown value[0][h] = 16 (2 pot win[h] + pot tie[h]) with win / tie of range vs range against w_1."""
    from pokerl_amd import judger as J
    rng = np.random.default_rng(407)
    pot = 120
    board, nboard, dead = VS.random_boards(rng, 3, 5, lambda i: (47, 33, 10)[i])
    ranges = random_ranges(rng, 3)
    got = device_solve(board, ranges, forced_tree(pot), 2, dead)
    for p in (0, 1):
        r = J.range_vs_range_batch(board, nboard, dead, ranges[:, 1 - p])
        want = 16 * (2 * pot * r.win.astype(np.int64) + pot * r.tie.astype(np.int64))
        assert (got["value"][:, p] == want).all() and (got["br"][:, p] == want).all(), p


def test_more_spots_than_the_grid(PK):
    """m = 2 x the grid limit + 1 spots at P = 6: every spot equals the spec; a spot repeated at 0, grid and 2 grid is byte-identical"""
    from pokerl_amd import solver as S
    rng = np.random.default_rng(408)
    grid = S.GRID_MAX
    m = 2 * grid + 1
    board, _, dead = VS.random_boards(rng, m, 5, 6)
    ranges = random_ranges(rng, m)
    for i in (grid, 2 * grid):
        board[i], dead[i], ranges[i] = board[0], dead[0], ranges[0]
    tree = PK.river_tree(100, 50)
    got = device_solve(board, ranges, tree, 2, dead)
    assert_equal(got, RS.solve_batch(board, ranges, tree, 2, dead), "%d spots" % m)
    for k in KEYS:
        assert got[k][0].tobytes() == got[k][grid].tobytes() == got[k][2 * grid].tobytes(), k


def test_status_inside_a_good_batch_alone_and_no_spots(PK):
    from pokerl_amd import _lib as L
    from pokerl_amd import solver as S
    rng = np.random.default_rng(409)
    m = 7
    board, _, dead = VS.random_boards(rng, m, 5, lambda i: 12)
    ranges = random_ranges(rng, m)
    board[1, 2] = 0x3D                                                        # no card
    board[3, 4] = board[3, 0]                                                 # the same card twice
    dead[5] = np.uint64(((1 << 52) - 1) & ~0b111)                             # three cards are not dead: too few
    dead[6] |= np.uint64(1 << 60)                                             # a dead bit that is no card
    tree = PK.river_tree(100, 50)
    got = device_solve(board, ranges, tree, 3, dead)
    want = RS.solve_batch(board, ranges, tree, 3, dead)
    assert (want["status"][[1, 3, 6]] == [RS.BAD_CARD, RS.DUP_CARD, RS.BAD_CARD]).all() and want["status"][5] & RS.SMALL_POOL
    assert_equal(got, want, "bad spots inside a good batch")
    status = np.full(m, 7, np.uint8)
    L.check(L.lib().pk_solve_river(0, m, L.ptr(board), L.ptr(dead), L.ptr(ranges), *S._tree_args(tree), 3, None, None, None, L.ptr(status)))
    assert (status == got["status"]).all()
    value, status = np.full((m, 2, H), 7, np.int64), np.full(m, 7, np.uint8)
    L.check(L.lib().pk_solve_river(0, 0, L.ptr(board), L.ptr(dead), L.ptr(ranges), *S._tree_args(tree), 3, None, L.ptr(value), None, L.ptr(status)))
    assert (value == 7).all() and (status == 7).all()


def test_the_device_form_on_a_callers_stream(PK):
    from pokerl_amd import hipmem
    from pokerl_amd import solver as S
    rng = np.random.default_rng(410)
    m = 5
    board, _, dead = VS.random_boards(rng, m, 5, lambda i: (47, 30, 4, 46, 9)[i])
    ranges = random_ranges(rng, m)
    tree = PK.river_tree(100, 400)
    D = len(tree.decision_nodes)
    want = device_solve(board, ranges, tree, 4, dead)
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0              # hipStreamNonBlocking: a caller's own stream
    ins = [hipmem.DeviceBuffer(x.nbytes).upload(x) for x in (board, dead, ranges)]
    outs = [hipmem.DeviceBuffer(n) for n in (m * D * 4 * H * 2, m * 2 * H * 8, m * 2 * H * 8, m)]
    for rep in range(2):                                                      # (the second call reuses the stream's work space)
        S.solve_river_d(m, ins[0].ptr, ins[2].ptr, tree, 4, dead_d=ins[1].ptr, strategy_d=outs[0].ptr, value_d=outs[1].ptr, br_d=outs[2].ptr,
                        status_d=outs[3].ptr, stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        assert (outs[0].download(np.uint16, m * D * 4 * H).reshape(m, D, 4, H) == want["strategy"]).all()
        assert (outs[1].download(np.int64, m * 2 * H).reshape(m, 2, H) == want["value"]).all()
        assert (outs[2].download(np.int64, m * 2 * H).reshape(m, 2, H) == want["br"]).all()
        assert (outs[3].download(np.uint8, m) == want["status"]).all()
    assert hip.hipStreamDestroy(stream) == 0
    for x in ins + outs:
        x.free()


def test_convergence_on_the_default_tree(PK):
    """One seeded spot, the pool shrunk to P = 24 with `dead` so that 256 spec iterations stay a few seconds: the device exploitability
    at 16, 64 and 256 iterations is strictly decreasing, and at 256 iterations every output equals the spec's."""
    from pokerl_amd import solver as S
    rng = np.random.default_rng(411)
    board, _, dead = VS.random_boards(rng, 1, 5, 24)
    ranges = random_ranges(rng, 1)
    tree = PK.river_tree(100, 400)
    sols = {it: S.solve_river_batch(board, ranges, tree, it, dead) for it in (16, 64, 256)}
    expl = [sols[it][0].exploitability for it in (16, 64, 256)]
    print("exploitability at 16, 64, 256 iterations:", expl)
    assert expl[0] > expl[1] > expl[2] > 0
    want = RS.solve_batch(board, ranges, tree, 256, dead)
    assert_equal(as_dict(sols[256]), want, "256 iterations")
    assert expl[2] == RS.exploitability(ranges[0], want["value"][0], want["br"][0], want["valid"][0])
