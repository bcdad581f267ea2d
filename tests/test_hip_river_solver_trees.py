"""GPU tests of the river solver with a tree per spot (pk_solve_river_trees: DESIGN.md section 3.14).  The definition is the test: spot i's
outputs are byte for byte what pk_solve_river gives for that spot alone with tree tree_of[i] -- here the numpy spec run one spot at a time
with that spot's tree (solver_trees_util.river_expect; pools shrunk with `dead` so that the live spec is the reference), laid out with the
call's row stride, the rows past the spot's own zero.  One tree (the identity with pk_solve_river), five mixed trees with big after small
and small after big, more spots than the grid with a different tree on a workgroup's second spot, tree_of that names no tree, a tree no
spot names, the stream form with the host tree arrays overwritten behind the call, and the full pool on the largest tree."""
import ctypes as C

import numpy as np
import pytest

import river_solver_spec as RS
import rvr_spec as VS
import solver_trees_util as U

pytestmark = pytest.mark.gpu

H = RS.HOLDINGS
KEYS = ("strategy", "value", "br", "status", "valid")
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


def as_dict(r):
    return {k: np.asarray(getattr(r, k)) for k in KEYS}


def assert_equal(got, want, where, keys=KEYS):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype and (a == b).all(), (where, k, np.argwhere(a != b)[:4].tolist())


def solve(board, ranges, trees, tree_of, iters, dead):
    from pokerl_amd import solver as S
    return S.solve_river_batch(board, ranges, trees, iters, dead, tree_of=tree_of)


def mixed_trees(PK):
    """39 nodes (D = 14), the forced 3, the four-action 11, the 64-node chain, and 9 nodes"""
    trees = [PK.river_tree(100, 400), U.forced_river_tree(), U.four_action_river_tree(), U.chain_river_tree(), PK.river_tree(40, 30, (1.0,), 1)]
    assert [t.n for t in trees] == [39, 3, 11, 64, 9] and len(trees[0].decision_nodes) == 14
    return trees


@pytest.fixture(scope="module")
def mixed(PK):
    """(b)'s spots, trees and what the spec gives for them -- computed once, shared with the stream form's test, never changed"""
    rng = np.random.default_rng(0x7231)
    pools = [9, 24, 12, 16, 7, 20, 11, 24, 6, 13, 10, 17]
    tree_of = np.array([1, 3, 1, 0, 4, 3, 2, 0, 3, 1, 4, 2], np.uint32)       # big after small (1 -> 3, 4 -> 3) and small after big (3 -> 1, 0 -> 4)
    board, _, dead = VS.random_boards(rng, 12, 5, lambda i: pools[i])
    ranges = random_ranges(rng, 12)
    trees = mixed_trees(PK)
    want = U.river_expect(board, ranges, trees, tree_of, 3, dead)
    for v in want.values():
        v.setflags(write=False)
    return dict(board=board, dead=dead, ranges=ranges, trees=trees, tree_of=tree_of, pools=pools, want=want)


def test_one_tree_is_the_single_tree_call(PK):
    """(a) ntrees = 1: P = 9, 16, 24, 47 and a refused spot on the default tree, 8 iterations"""
    from pokerl_amd import solver as S
    rng = np.random.default_rng(0x7230)
    pools = [9, 16, 24, 47, 12]
    board, _, dead = VS.random_boards(rng, 5, 5, lambda i: pools[i])
    board[4, 3] = board[4, 1]                                                 # a card twice
    ranges = random_ranges(rng, 5)
    tree = PK.river_tree(100, 400)
    got = as_dict(solve(board, ranges, [tree], np.zeros(5, np.uint32), 8, dead))
    one = as_dict(S.solve_river_batch(board, ranges, tree, 8, dead))
    for k in KEYS:
        assert got[k].tobytes() == one[k].tobytes(), k
    assert got["status"].tolist() == [0, 0, 0, 0, RS.DUP_CARD]
    small = [0, 1, 2, 4]                                                      # P <= 24 and the refused spot: the spec itself
    want = RS.solve_batch(board[small], ranges[small], tree, 8, dead[small])
    assert_equal({k: got[k][small] for k in KEYS}, want, "one tree, against the spec")


def test_mixed_trees_every_spot_equals_the_spec_with_its_own_tree(PK, mixed):
    """(b) five trees, twelve spots, 3 iterations"""
    x = mixed
    r = solve(x["board"], x["ranges"], x["trees"], x["tree_of"], 3, x["dead"])
    got = as_dict(r)
    assert got["strategy"].shape == (12, 32, 4, H) and not got["status"].any()
    assert_equal(got, x["want"], "mixed trees")
    for i in range(12):
        tree = x["trees"][x["tree_of"][i]]
        D = len(tree.decision_nodes)
        assert not got["strategy"][i, D:].any() and got["strategy"][i, D - 1].any(), i      # rows >= D are zero, the last own row is not
        one = r[i]
        assert one.tree is tree and one.strategy.shape == (D, 4, H)
        spec = RS.solve_spot([int(c) for c in x["board"][i]], x["ranges"][i], tree, 3, int(x["dead"][i]))
        assert one.exploitability == RS.exploitability(x["ranges"][i], spec["value"], spec["br"], spec["valid"]), i
        assert list(one.ev) == RS.ev(x["ranges"][i], spec["value"], spec["valid"]), i


def test_more_spots_than_the_grid_with_a_different_tree_on_the_second_spot(PK):
    """(c) m = 300 at P = 6 .. 9, 2 iterations, tree_of[i] = i % 3: workgroup i's second spot i + 256 has another tree"""
    from pokerl_amd import solver as S
    rng = np.random.default_rng(0x7232)
    m = 300
    tree_of = (np.arange(m) % 3).astype(np.uint32)
    assert m > S.GRID_MAX and all(tree_of[i + S.GRID_MAX] != tree_of[i] for i in range(m - S.GRID_MAX))
    board, _, dead = VS.random_boards(rng, m, 5, lambda i: 6 + i % 4)
    ranges = random_ranges(rng, m)
    trees = [U.four_action_river_tree(), PK.river_tree(100, 50), U.forced_river_tree()]
    got = as_dict(solve(board, ranges, trees, tree_of, 2, dead))
    assert_equal(got, U.river_expect(board, ranges, trees, tree_of, 2, dead), "%d spots" % m)


def test_a_tree_of_that_names_no_tree(PK):
    """(d) tree_of = ntrees and 0xFFFFFFFF inside a good batch: PK_EQ_BAD_TREE and zeros there, the neighbours equal the spec"""
    from pokerl_amd import _lib as L
    rng = np.random.default_rng(0x7233)
    m = 6
    board, _, dead = VS.random_boards(rng, m, 5, lambda i: 10 + i)
    ranges = random_ranges(rng, m)
    trees = [PK.river_tree(100, 50), U.four_action_river_tree()]
    tree_of = np.array([1, 2, 0, 0xFFFFFFFF, 1, 0], np.uint32)
    got = as_dict(solve(board, ranges, trees, tree_of, 2, dead))
    assert got["status"].tolist() == [0, BAD_TREE, 0, BAD_TREE, 0, 0] and L.EQ_BAD_TREE == BAD_TREE
    for i in (1, 3):
        assert not got["strategy"][i].any() and not got["value"][i].any() and not got["br"][i].any() and not got["valid"][i].any()
    assert_equal(got, U.river_expect(board, ranges, trees, tree_of, 2, dead), "bad tree_of inside a good batch")
    board[1, 0] = 0x3D                                                        # ... and beside what the cards report
    status = np.full(m, 7, np.uint8)
    rows = __import__("pokerl_amd").solver._TreeRows(trees, 64)
    L.check(L.lib().pk_solve_river_trees(0, m, L.ptr(board), L.ptr(dead), L.ptr(ranges), *rows.args(), L.ptr(tree_of), 2, None, None, None, L.ptr(status)))
    assert status.tolist() == [0, BAD_TREE | RS.BAD_CARD, 0, BAD_TREE, 0, 0]  # status alone: the preparation kernels write it


def test_an_unreferenced_tree_still_sets_the_stride(PK):
    """(e) the 64-node tree is passed and named by no spot: 32 rows a spot, the rows past the spot's own zero; the rest as without it"""
    rng = np.random.default_rng(0x7234)
    board, _, dead = VS.random_boards(rng, 3, 5, lambda i: (14, 9, 21)[i])
    ranges = random_ranges(rng, 3)
    trees = [PK.river_tree(100, 50), U.chain_river_tree(), U.forced_river_tree()]
    tree_of = np.array([0, 2, 0], np.uint32)
    got = as_dict(solve(board, ranges, trees, tree_of, 2, dead))
    assert got["strategy"].shape == (3, 32, 4, H)
    assert_equal(got, U.river_expect(board, ranges, trees, tree_of, 2, dead), "an unreferenced tree")
    without = as_dict(solve(board, ranges, [trees[0], trees[2]], np.array([0, 1, 0], np.uint32), 2, dead))
    assert without["strategy"].shape == (3, 4, 4, H) and (without["strategy"] == got["strategy"][:, :4]).all() and not got["strategy"][:, 4:].any()
    for k in ("value", "br", "status"):
        assert (without[k] == got[k]).all(), k


def test_the_device_form_with_the_host_trees_overwritten_behind_the_call(PK, mixed):
    """(f) pk_solve_river_trees_d on a caller's stream: the host tree arrays are overwritten as soon as the call returns, before the
    stream is synchronised; the results equal (b)'s"""
    from pokerl_amd import _lib as L
    from pokerl_amd import hipmem
    from pokerl_amd import solver as S
    x = mixed
    m, D = 12, 32
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0              # hipStreamNonBlocking: a caller's own stream
    ins = [hipmem.DeviceBuffer(a.nbytes).upload(a) for a in (x["board"], x["dead"], x["ranges"], x["tree_of"])]
    outs = [hipmem.DeviceBuffer(n) for n in (m * D * 4 * H * 2, m * 2 * H * 8, m * 2 * H * 8, m)]
    for rep in range(2):                                                      # (the second call reuses the stream's work space)
        rows = S._TreeRows(x["trees"], 64)
        L.check(L.lib().pk_solve_river_trees_d(0, m, ins[0].ptr, ins[1].ptr, ins[2].ptr, *rows.args(), ins[3].ptr, 3, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                               outs[3].ptr, stream))
        for a in (rows.n, rows.kind, rows.child, rows.put, rows.pot):
            a[...] = 0xFF if a.dtype == np.uint8 else 0xFFFFFFFF
        assert hip.hipStreamSynchronize(stream) == 0
        assert (outs[0].download(np.uint16, m * D * 4 * H).reshape(m, D, 4, H) == x["want"]["strategy"]).all()
        assert (outs[1].download(np.int64, m * 2 * H).reshape(m, 2, H) == x["want"]["value"]).all()
        assert (outs[2].download(np.int64, m * 2 * H).reshape(m, 2, H) == x["want"]["br"]).all()
        assert (outs[3].download(np.uint8, m) == x["want"]["status"]).all()
    S.solve_river_d(m, ins[0].ptr, ins[2].ptr, x["trees"], 3, dead_d=ins[1].ptr, status_d=outs[3].ptr, stream=stream, tree_of=ins[3].ptr)   # the Python form
    assert hip.hipStreamSynchronize(stream) == 0 and not outs[3].download(np.uint8, m).any()
    assert hip.hipStreamDestroy(stream) == 0
    for b in ins + outs:
        b.free()


def test_the_full_pool_on_the_largest_tree_among_small_ones(PK):
    """(g) one P = 47 spot with the 64-node tree between small-tree spots: it equals the single-tree device call, the others the spec"""
    from pokerl_amd import solver as S
    rng = np.random.default_rng(0x7236)
    pools = [8, 47, 11, 9]
    board, _, dead = VS.random_boards(rng, 4, 5, lambda i: pools[i])
    ranges = random_ranges(rng, 4)
    trees = [U.forced_river_tree(), U.chain_river_tree(), PK.river_tree(40, 30, (1.0,), 1)]
    tree_of = np.array([0, 1, 2, 0], np.uint32)
    got = as_dict(solve(board, ranges, trees, tree_of, 2, dead))
    one = as_dict(S.solve_river_batch(board[1:2], ranges[1:2], trees[1], 2, dead[1:2]))
    for k in KEYS:
        assert got[k][1].tobytes() == one[k][0].tobytes(), k
    assert got["valid"][1].sum() == 1081 and got["strategy"][1, 31].any()
    small = [0, 2, 3]
    want = U.river_expect(board[small], ranges[small], trees, tree_of[small], 2, dead[small])
    assert_equal({k: got[k][small] for k in KEYS}, want, "the small-tree spots around the full pool")
