"""GPU tests of the pre-flop solver (pk_solve_preflop: DESIGN.md section 3.18).  The table is fixed at 1 326 x 1 326, so "small" means few
spots, few iterations and small trees.  The restatement (tests/preflop_solver_spec.py) runs on the DEVICE'S OWN table, fetched once per module
-- the pre-flop suite pins that table to pk_equity and the golden matchups -- and every output is compared with it byte for byte: push / fold
at three stacks through tree_of, a tree with a limp line, the host and the device forms, each output alone, a spot repeated across the
persistent grid, a spot whose tree_of names no tree, m = 0.  The showdown is cross-checked against an independent kernel
(preflop_range_vs_range), and the exploitability must fall."""
import ctypes as C

import numpy as np
import pytest

import preflop_solver_spec as PFS

pytestmark = pytest.mark.gpu

H = PFS.HOLDINGS
KEYS = ("strategy", "value", "br", "status")


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


@pytest.fixture(scope="module")
def table(PK):
    t = PK.preflop_matchups()
    return t.win, t.tie


def random_ranges(rng, m):
    w = rng.integers(0, 65536, (m, 2, H)).astype(np.uint16)
    for row in w.reshape(-1, H):
        row[rng.integers(0, H, 200)] = 0
        row[rng.integers(0, H, 100)] = 65535
    return w


def as_dict(r):
    return {k: np.asarray(getattr(r, k)) for k in KEYS}


def assert_equal(got, want, where):
    for k in KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype and (a == b).all(), (where, k, np.argwhere(a != b)[:4].tolist())


@pytest.fixture(scope="module")
def push_fold(PK, table):
    """three push / fold spots at three stacks through tree_of, and the restatement at 1, 2 and 16 iterations (computed once, shared)"""
    rng = np.random.default_rng(1801)
    trees, tree_of = PK.preflop_trees([12, 40, 5], push_fold=True)
    ranges = random_ranges(rng, 3)
    assert (ranges == 0).any() and (ranges == 65535).any()
    want = {iters: PFS.solve_batch(table, ranges, trees, iters, tree_of) for iters in (1, 2, 16)}
    return trees, tree_of, ranges, want


@pytest.mark.parametrize("iters", [1, 2, 16])
def test_push_fold_at_three_stacks_equals_the_spec(PK, push_fold, iters):
    trees, tree_of, ranges, want = push_fold
    sol = PK.solve_preflop_batch(ranges, trees, iters, tree_of)
    got = as_dict(sol)
    assert not got["status"].any() and sol.valid.all() and got["strategy"].shape == (3, 2, 4, H)
    assert (got["strategy"].astype(np.int64).sum(axis=2) == PFS.ONE).all() and (got["br"] >= got["value"]).all()
    assert_equal(got, want[iters], "push / fold, %d iterations" % iters)
    one = sol[1]
    assert one.tree is trees[1] and one.probabilities(2).shape == (2, H) and one.by_class(0).shape == (2, 13, 13)
    assert one.exploitability == PFS.exploitability(ranges[1], want[iters]["value"][1], want[iters]["br"][1])


def test_each_output_alone_and_the_device_form(PK, push_fold):
    from pokerl_amd import _lib as L
    from pokerl_amd import hipmem
    from pokerl_amd import solver as S
    trees, tree_of, ranges, want = push_fold
    want, m, D = want[2], 3, 2
    rows = S._TreeRows(trees, 64)
    shapes = {"strategy": ((m, D, 4, H), np.uint16), "value": ((m, 2, H), np.int64), "br": ((m, 2, H), np.int64)}
    for key in shapes:                                                          # the host form, one output at a time
        out = {k: (np.full(s, 7, t) if k == key else None) for k, (s, t) in shapes.items()}
        status = np.full(m, 7, np.uint8)
        L.check(L.lib().pk_solve_preflop(0, m, L.ptr(ranges), *rows.args(), L.ptr(tree_of), 2, L.ptr(out["strategy"]), L.ptr(out["value"]), L.ptr(out["br"]),
                                         L.ptr(status)))
        assert (out[key] == want[key]).all() and not status.any(), key
    status = np.full(m, 7, np.uint8)                                            # status alone
    L.check(L.lib().pk_solve_preflop(0, m, L.ptr(ranges), *rows.args(), L.ptr(tree_of), 2, None, None, None, L.ptr(status)))
    assert not status.any()
    # the device form on a caller's stream: everything, then each output alone
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    ins = [hipmem.DeviceBuffer(x.nbytes).upload(x) for x in (ranges, tree_of)]
    sizes = {"strategy": m * D * 4 * H * 2, "value": m * 2 * H * 8, "br": m * 2 * H * 8, "status": m}
    for wanted in (("strategy", "value", "br"), ("strategy",), ("value",), ("br",), ()):
        outs = {k: hipmem.DeviceBuffer(sizes[k]) for k in wanted + ("status",)}
        ptr = {k: (outs[k].ptr if k in outs else None) for k in sizes}
        S.solve_preflop_d(m, ins[0].ptr, trees, 2, tree_of=ins[1].ptr, strategy_d=ptr["strategy"], value_d=ptr["value"], br_d=ptr["br"],
                          status_d=ptr["status"], stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        for k in wanted:
            shape, dtype = shapes[k]
            assert (outs[k].download(dtype, int(np.prod(shape))).reshape(shape) == want[k]).all(), (wanted, k)
        assert not outs["status"].download(np.uint8, m).any()
        for b in outs.values():
            b.free()
    assert hip.hipStreamDestroy(stream) == 0
    for b in ins:
        b.free()


def test_a_tree_with_a_limp_line_and_several_showdowns(PK, table):
    tree = PK.preflop_tree(12, 1, 2, 0, (1.0,), 2)
    assert sum(int(k) == 4 for k in tree.kind) >= 4 and tree.label(int(tree.child[int(tree.child[0][1])][0])) == "0:call 1:check"
    ranges = random_ranges(np.random.default_rng(1802), 2)
    got = as_dict(PK.solve_preflop_batch(ranges, tree, 8))
    assert_equal(got, PFS.solve_batch(table, ranges, tree, 8), "preflop_tree(12), 8 iterations")
    one = PK.solve_preflop(ranges[1], tree, 8)
    assert (one.strategy == got["strategy"][1]).all() and (one.value == got["value"][1]).all() and (one.br == got["br"][1]).all()


def test_a_showdown_against_range_vs_range(PK):
    """One decision, one showdown: value[p][h] is the showdown formula in Python integers from preflop_range_vs_range's sums for the
    other player's weights -- an independent kernel over the same table."""
    from pokerl_amd.solver import RiverTree
    FF = 0xFF
    pot, c = 7, 25
    tree = RiverTree([0, 4], [[1, FF, FF, FF], [FF] * 4], [[3, 5], [c, c]], pot)
    ranges = random_ranges(np.random.default_rng(1803), 1)[0]
    sol = PK.solve_preflop(ranges, tree, 1)
    for p in (0, 1):
        rvr = PK.preflop_range_vs_range(ranges[1 - p])
        for h in range(H):
            E = 16 * (2 * int(rvr.win[h]) + int(rvr.tie[h]))
            assert int(rvr.tot[h]) % PFS.BOARDS == 0
            S = 16 * (int(rvr.tot[h]) // PFS.BOARDS)
            assert int(sol.value[p, h]) == ((pot + 2 * c) * E) // PFS.BOARDS - 2 * c * S, (p, h)
    assert (sol.value == sol.br).all() and (sol.strategy[0, 0] == PFS.ONE).all()


def test_no_output_depends_on_the_grid(PK, table):
    """One spot at index 0, at index grid and at index 2 grid among m = 2 grid + 1 push / fold spots of 16 iterations"""
    from pokerl_amd import solver as S
    grid = S.GRID_MAX
    m = 2 * grid + 1
    rng = np.random.default_rng(1804)
    few = random_ranges(rng, 7)
    ranges = few[rng.integers(1, 7, m)]
    ranges[[0, grid, 2 * grid]] = few[0]
    tree = PK.push_fold_tree(15)
    got = as_dict(PK.solve_preflop_batch(ranges, tree, 16))
    assert not got["status"].any()
    for k in ("strategy", "value", "br"):
        assert (got[k][0] == got[k][grid]).all() and (got[k][0] == got[k][2 * grid]).all(), k
    want = PFS.solve_spot(table, few[0], tree, 16)
    for k in ("strategy", "value", "br"):
        assert (got[k][0] == want[k]).all(), k


def test_a_bad_tree_between_valid_spots_and_m_zero(PK, push_fold):
    from pokerl_amd import _lib as L
    from pokerl_amd import solver as S
    trees, tree_of, ranges, want = push_fold
    of = np.array([tree_of[0], 3, tree_of[2], 0xFFFFFFFF], np.uint32)
    r4 = np.concatenate([ranges, ranges[:1]])
    sol = PK.solve_preflop_batch(r4, trees, 2, of)
    got = as_dict(sol)
    assert got["status"].tolist() == [0, L.EQ_BAD_TREE, 0, L.EQ_BAD_TREE]
    for i in (1, 3):
        assert not got["strategy"][i].any() and not got["value"][i].any() and not got["br"][i].any() and not sol.valid[i].any()
    for i in (0, 2):                                                            # the neighbours are what they are without it
        for k in ("strategy", "value", "br"):
            assert (got[k][i] == want[2][k][i]).all(), (i, k)
    assert sol[1].tree is None and sol[1].strategy.shape[0] == 0
    rows = S._TreeRows(trees, 64)
    value, status = np.full((1, 2, H), 7, np.int64), np.full(1, 7, np.uint8)     # m = 0 writes nothing
    L.check(L.lib().pk_solve_preflop(0, 0, L.ptr(ranges), *rows.args(), L.ptr(tree_of), 2, None, L.ptr(value), None, L.ptr(status)))
    assert (value == 7).all() and (status == 7).all()


def test_convergence_on_uniform_ranges(PK, table):
    """push_fold_tree(20), uniform ranges: the exploitability, from the device's own value / br, falls strictly at 16 / 64 / 256 iterations.
    Measured on an MI355X: DESIGN.md section 3.18.  No percentage of the pot and no chart from the literature is asserted."""
    tree = PK.push_fold_tree(20)
    ranges = np.full((2, H), 65535, np.uint16)
    sols = {iters: PK.solve_preflop(ranges, tree, iters) for iters in (16, 64, 256)}
    curve = [sols[i].exploitability for i in (16, 64, 256)]
    print("exploitability at 16 / 64 / 256 iterations: %.6f -> %.6f -> %.6f chips; ev %s" % (*curve, sols[256].ev))
    assert curve[0] > curve[1] > curve[2] > 0
    want = PFS.solve_spot(table, ranges, tree, 64)
    for k in ("strategy", "value", "br"):
        assert (np.asarray(getattr(sols[64], k)) == want[k]).all(), k
    assert abs(sum(sols[256].ev)) < 1e-3                                          # zero-sum up to the floors
