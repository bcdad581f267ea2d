"""GPU tests of the turn solver with a tree per spot (pk_solve_turn_trees: DESIGN.md section 3.14), the river tests' pattern one street
earlier: spot i's outputs -- river_strategy included -- are byte for byte the numpy spec's for that spot alone with tree tree_of[i]
(solver_trees_util.turn_expect; pools shrunk with `dead`), laid out with the call's two row strides, the rows past the spot's own zero.
Trees: turn_tree(100, 400, (1.0,), 1) (36 nodes, 4 + 12 decisions), a hand-made ten-node tree with an all-in chance -> showdown (3 + 2) and
turn_tree(30, 20, (1.0,), 1) (20 nodes, 4 + 4)."""
import ctypes as C

import numpy as np
import pytest

import rvr_spec as VS
import solver_trees_util as U
import turn_solver_spec as TS

pytestmark = pytest.mark.gpu

H = TS.HOLDINGS
KEYS = ("strategy", "river_strategy", "value", "br", "status", "valid")
BAD_TREE = 32


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


def random_ranges(rng, m):
    w = rng.integers(0, 65536, (m, 2, H)).astype(np.uint16)
    for row in w.reshape(-1, H):
        row[rng.integers(0, H, 200)] = 0
        row[rng.integers(0, H, 100)] = 65535
    return w


def spots(rng, pools):
    board, _, dead = VS.random_boards(rng, len(pools), 4, lambda i: pools[i])
    return np.ascontiguousarray(board[:, :4]), dead, random_ranges(rng, len(pools))


def as_dict(r, keys=KEYS):
    return {k: np.asarray(getattr(r, k)) for k in keys}


def assert_equal(got, want, where, keys=KEYS):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype and (a == b).all(), (where, k, np.argwhere(a != b)[:4].tolist())


def solve(board, ranges, trees, tree_of, iters, dead, river=True):
    from pokerl_amd import solver as S
    return S.solve_turn_batch(board, ranges, trees, iters, dead, river_strategy=river, tree_of=tree_of)


def the_trees(PK):
    trees = [PK.turn_tree(100, 400, (1.0,), 1), U.allin_turn_tree(), PK.turn_tree(30, 20, (1.0,), 1)]
    assert [(t.n, len(t.decision_nodes), len(t.river_decision_nodes)) for t in trees] == [(36, 4, 12), (10, 3, 2), (20, 4, 4)]
    return trees


@pytest.fixture(scope="module")
def mixed(PK):
    """(b)'s spots, trees and what the spec gives for them -- computed once, shared with the stream form's test, never changed"""
    rng = np.random.default_rng(0x7431)
    pools = [9, 14, 10, 12, 9, 13, 11, 14]
    tree_of = np.array([1, 0, 1, 2, 0, 2, 1, 0], np.uint32)                   # big after small (1 -> 0, 2 -> 0) and small after big (0 -> 1, 0 -> 2)
    board, dead, ranges = spots(rng, pools)
    trees = the_trees(PK)
    want = U.turn_expect(board, ranges, trees, tree_of, 3, dead)
    for v in want.values():
        v.setflags(write=False)
    return dict(board=board, dead=dead, ranges=ranges, trees=trees, tree_of=tree_of, want=want)


def test_one_tree_is_the_single_tree_call(PK):
    """(a) ntrees = 1: P = 9, 12, 14 and a refused spot against the spec and against pk_solve_turn, and one P = 48 spot against the
    single-tree device call; 4 iterations"""
    from pokerl_amd import solver as S
    rng = np.random.default_rng(0x7430)
    board, dead, ranges = spots(rng, [9, 12, 14, 48, 10])
    board[4, 3] = board[4, 1]                                                 # a card twice
    tree = PK.turn_tree(100, 400, (1.0,), 1)
    keys = tuple(k for k in KEYS if k != "river_strategy")                    # (river_strategy at P = 48: 6.6 MB a spot; the small pools below have it)
    got = as_dict(solve(board, ranges, [tree], np.zeros(5, np.uint32), 4, dead, river=False), keys)
    one = as_dict(S.solve_turn_batch(board, ranges, tree, 4, dead), keys)
    for k in keys:
        assert got[k].tobytes() == one[k].tobytes(), k
    assert got["status"].tolist() == [0, 0, 0, 0, TS.DUP_CARD] and got["valid"][3].sum() == 1128
    small = [0, 1, 2, 4]
    with_river = as_dict(solve(board[small], ranges[small], [tree], np.zeros(4, np.uint32), 4, dead[small]))
    assert_equal(with_river, TS.solve_batch(board[small], ranges[small], tree, 4, dead[small]), "one tree, against the spec")
    for k in keys:
        assert (with_river[k] == got[k][small]).all(), k


def test_mixed_trees_every_spot_equals_the_spec_with_its_own_tree(PK, mixed):
    """(b) three trees, eight spots at P = 9 .. 14, 3 iterations; both strategies' rows past the spot's own are zero"""
    x = mixed
    r = solve(x["board"], x["ranges"], x["trees"], x["tree_of"], 3, x["dead"])
    got = as_dict(r)
    assert got["strategy"].shape == (8, 4, 4, H) and got["river_strategy"].shape == (8, 12, 52, 4, H) and not got["status"].any()
    assert_equal(got, x["want"], "mixed trees")
    for i in range(8):
        tree = x["trees"][x["tree_of"][i]]
        Dt, Dr = len(tree.decision_nodes), len(tree.river_decision_nodes)
        assert not got["strategy"][i, Dt:].any() and got["strategy"][i, Dt - 1].any(), i
        assert not got["river_strategy"][i, Dr:].any() and got["river_strategy"][i, Dr - 1].any(), i
        one = r[i]
        assert one.tree is tree and one.strategy.shape == (Dt, 4, H) and one.river_strategy.shape == (Dr, 52, 4, H)
        w = x["want"]
        assert one.exploitability == TS.exploitability(x["ranges"][i], w["value"][i], w["br"][i], w["valid"][i], int(w["P"][i])), i
        assert list(one.ev) == TS.ev(x["ranges"][i], w["value"][i], w["valid"][i], int(w["P"][i])), i


def test_more_spots_than_the_grid_with_a_different_tree_on_the_second_spot(PK):
    """(c) m = 260 at P = 6 .. 8, 1 iteration: the call's grid is sized for the largest tree and is below m; tree_of steps by one from a
    workgroup's first spot i to its second spot i + grid, whatever the grid"""
    from pokerl_amd import solver as S
    rng = np.random.default_rng(0x7432)
    m = 260
    trees = the_trees(PK)
    grid = S.turn_grid(trees, m)
    tree_of = ((np.arange(m) % grid + np.arange(m) // grid) % 3).astype(np.uint32)
    assert 16 <= grid < m and grid == S.turn_grid(trees) and all(tree_of[i + grid] != tree_of[i] for i in range(m - grid)), grid
    board, dead, ranges = spots(rng, [6 + i % 3 for i in range(m)])
    got = as_dict(solve(board, ranges, trees, tree_of, 1, dead, river=False), tuple(k for k in KEYS if k != "river_strategy"))
    want = U.turn_expect(board, ranges, trees, tree_of, 1, dead)
    assert_equal(got, want, "%d spots on a grid of %d" % (m, grid), tuple(k for k in KEYS if k != "river_strategy"))


def test_a_tree_of_that_names_no_tree(PK):
    """(d) tree_of = ntrees and 0xFFFFFFFF inside a good batch: PK_EQ_BAD_TREE and zeros there, the neighbours equal the spec"""
    rng = np.random.default_rng(0x7433)
    board, dead, ranges = spots(rng, [9, 10, 11, 12, 9, 10])
    trees = the_trees(PK)[1:]
    tree_of = np.array([1, 2, 0, 0xFFFFFFFF, 1, 0], np.uint32)
    got = as_dict(solve(board, ranges, trees, tree_of, 2, dead))
    assert got["status"].tolist() == [0, BAD_TREE, 0, BAD_TREE, 0, 0]
    for i in (1, 3):
        assert not any(got[k][i].any() for k in ("strategy", "river_strategy", "value", "br", "valid")), i
    assert_equal(got, U.turn_expect(board, ranges, trees, tree_of, 2, dead), "bad tree_of inside a good batch")


def test_an_unreferenced_tree_still_sets_the_strides(PK):
    """(e) the 36-node tree is passed and named by no spot: 4 and 12 rows a spot; everything else as without it"""
    rng = np.random.default_rng(0x7434)
    board, dead, ranges = spots(rng, [12, 9])
    trees = the_trees(PK)
    tree_of = np.array([1, 1], np.uint32)
    got = as_dict(solve(board, ranges, trees, tree_of, 2, dead))
    assert got["strategy"].shape == (2, 4, 4, H) and got["river_strategy"].shape == (2, 12, 52, 4, H)
    assert_equal(got, U.turn_expect(board, ranges, trees, tree_of, 2, dead), "an unreferenced tree")
    without = as_dict(solve(board, ranges, trees[1:2], np.zeros(2, np.uint32), 2, dead))
    assert without["strategy"].shape == (2, 3, 4, H) and without["river_strategy"].shape == (2, 2, 52, 4, H)
    assert (without["strategy"] == got["strategy"][:, :3]).all() and not got["strategy"][:, 3:].any()
    assert (without["river_strategy"] == got["river_strategy"][:, :2]).all() and not got["river_strategy"][:, 2:].any()
    for k in ("value", "br", "status"):
        assert (without[k] == got[k]).all(), k


def test_the_device_form_with_the_host_trees_overwritten_behind_the_call(PK, mixed):
    """(f) pk_solve_turn_trees_d on a caller's stream: the host tree arrays are overwritten as soon as the call returns, before the stream
    is synchronised; the results equal (b)'s"""
    from pokerl_amd import _lib as L
    from pokerl_amd import hipmem
    from pokerl_amd import solver as S
    x = mixed
    m, Dt, Dr = 8, 4, 12
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0              # hipStreamNonBlocking: a caller's own stream
    ins = [hipmem.DeviceBuffer(a.nbytes).upload(a) for a in (x["board"], x["dead"], x["ranges"], x["tree_of"])]
    outs = [hipmem.DeviceBuffer(n) for n in (m * Dt * 4 * H * 2, m * Dr * 52 * 4 * H * 2, m * 2 * H * 8, m * 2 * H * 8, m)]
    for rep in range(2):                                                      # (the second call reuses the stream's work space)
        rows = S._TreeRows(x["trees"], 128)
        L.check(L.lib().pk_solve_turn_trees_d(0, m, ins[0].ptr, ins[1].ptr, ins[2].ptr, *rows.args(), ins[3].ptr, 3, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                              outs[3].ptr, outs[4].ptr, stream))
        for a in (rows.n, rows.kind, rows.child, rows.put, rows.pot):
            a[...] = 0xFF if a.dtype == np.uint8 else 0xFFFFFFFF
        assert hip.hipStreamSynchronize(stream) == 0
        assert (outs[0].download(np.uint16, m * Dt * 4 * H).reshape(m, Dt, 4, H) == x["want"]["strategy"]).all()
        assert (outs[1].download(np.uint16, m * Dr * 52 * 4 * H).reshape(m, Dr, 52, 4, H) == x["want"]["river_strategy"]).all()
        assert (outs[2].download(np.int64, m * 2 * H).reshape(m, 2, H) == x["want"]["value"]).all()
        assert (outs[3].download(np.int64, m * 2 * H).reshape(m, 2, H) == x["want"]["br"]).all()
        assert (outs[4].download(np.uint8, m) == x["want"]["status"]).all()
    S.solve_turn_d(m, ins[0].ptr, ins[2].ptr, x["trees"], 3, dead_d=ins[1].ptr, status_d=outs[4].ptr, stream=stream, tree_of=ins[3].ptr)   # the Python form
    assert hip.hipStreamSynchronize(stream) == 0 and not outs[4].download(np.uint8, m).any()
    assert hip.hipStreamDestroy(stream) == 0
    for b in ins + outs:
        b.free()


def test_the_full_pool_among_small_tree_spots(PK):
    """(g) one P = 48 spot on the 36-node tree between spots of the ten-node tree: it equals the single-tree device call, the others the spec"""
    from pokerl_amd import solver as S
    rng = np.random.default_rng(0x7436)
    board, dead, ranges = spots(rng, [9, 48, 10])
    trees = the_trees(PK)
    tree_of = np.array([1, 0, 1], np.uint32)
    keys = tuple(k for k in KEYS if k != "river_strategy")
    got = as_dict(solve(board, ranges, trees, tree_of, 2, dead, river=False), keys)
    one = as_dict(S.solve_turn_batch(board[1:2], ranges[1:2], trees[0], 2, dead[1:2]), keys)
    for k in keys:
        assert got[k][1].tobytes() == one[k][0].tobytes(), k
    assert got["valid"][1].sum() == 1128
    small = [0, 2]
    want = U.turn_expect(board[small], ranges[small], trees, tree_of[small], 2, dead[small])
    assert_equal({k: got[k][small] for k in keys}, want, "the small-tree spots around the full pool", keys)
