"""CPU tests of the river and turn solvers' tree-per-spot calls (no GPU): the entry points in the header, the
binding and the library; every refusal of a tree names the tree ("tree <k>: " before the one-tree call's text) and is made before any
device is looked at; the row-stride helpers against Python; river_trees / turn_trees; a batch solution's solution[i]; and the new kernels
in the built library's code objects."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import river_solver_spec as RS
import solver_trees_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = RS.HOLDINGS
FF = 0xFF
ENTRY_POINTS = ("pk_solve_river_trees_d", "pk_solve_river_trees", "pk_solve_turn_trees_d", "pk_solve_turn_trees")
HELPERS = ("pk_rs_trees_rows", "pk_ts_trees_rows")


@pytest.fixture(scope="module")
def lib():
    from pokerl_amd import _lib, build
    build.build_lib()
    return _lib


@pytest.fixture(scope="module")
def S():
    from pokerl_amd import solver
    return solver


def river_set(S):
    return [S.river_tree(100, 400), U.forced_river_tree(), U.four_action_river_tree(), U.chain_river_tree(), S.river_tree(40, 30, (1.0,), 1)]


def turn_set(S):
    return [S.turn_tree(100, 400, (1.0,), 1), U.allin_turn_tree(), S.turn_tree(30, 20, (1.0,), 1)]


def call(lib, S, street, trees, change=None, iters=1, ntrees=None, skip=(), m=1, device_form=False):
    """The host (or device) form on one well-formed spot -> (return code, error text); change(rows) edits the packed rows first.  Nothing
    reaches a device when it refuses."""
    rows = S._TreeRows(trees, 64 if street == 5 else 128)
    if change:
        change(rows)
    board, ranges = np.arange(street, dtype=np.uint8)[None].copy(), np.ones((1, 2, H), np.uint16)
    tree_of, status = np.zeros(1, np.uint32), np.zeros(1, np.uint8)
    arr = dict(n=rows.n, kind=rows.kind, child=rows.child, put=rows.put, pot=rows.pot, tree_of=tree_of, board=board, ranges=ranges, status=status)
    p = {k: (None if k in skip else lib.ptr(v)) for k, v in arr.items()}
    name = "pk_solve_%s_trees%s" % ("river" if street == 5 else "turn", "_d" if device_form else "")
    outs = [None] * (3 if street == 5 else 4) + [p["status"]] + ([None] if device_form else [])
    rc = getattr(lib.lib(), name)(0, m, p["board"], None, p["ranges"], len(trees) if ntrees is None else ntrees, p["n"], p["kind"], p["child"], p["put"],
                                  p["pot"], p["tree_of"], iters, *outs)
    return rc, lib.lib().pk_last_error(None).decode(), name


def test_header_declares_and_binding_lists_the_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "pokerl_hip.h")).read()
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRY_POINTS + HELPERS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in lib.SYMBOLS and hasattr(L, name), name
    assert "a tree per spot" in header and re.search(r"#define PK_EQ_BAD_TREE 32u", header) and re.search(r"#define PK_RS_MAX_TREES 65536\b", header)
    assert lib.EQ_BAD_TREE == lib.EQ_BAD_TABLE == 32 and lib.RS_MAX_TREES == 65536
    assert "byte for byte what pk_solve_river / pk_solve_turn give for that spot alone" in header      # the definition
    assert lib.lib().pk_abi_version() == 6                                    # the four existing calls keep their signatures


def set_at(key, index, value):
    def change(rows):
        getattr(rows, key)[index] = value
    return change


@pytest.mark.parametrize("street", [5, 4])
@pytest.mark.parametrize("device_form", [False, True])
def test_a_bad_tree_is_refused_by_its_index_with_the_one_tree_text(lib, S, street, device_form):
    trees = river_set(S) if street == 5 else turn_set(S)
    last = len(trees) - 1
    top = 64 if street == 5 else 128
    cases = [(set_at("kind", (0, 0), 4), 0, "the root is not a decision node"),
             (set_at("n", last, 0), last, "n outside 1 .. %d" % top),
             (set_at("n", 1, top + 1), 1, "n outside 1 .. %d" % top),
             (set_at("pot", 2, 8192), 2, "pot + max put > 8191"),
             (set_at("child", (last, 0, 0), 0), last, "a child index is <= its parent or >= n"),
             (set_at("kind", (1, 1), 6), 1, "a node kind outside 0 .. %d" % (4 if street == 5 else 5))]
    if street == 4:
        cases.append((set_at("put", (1, 3, 0), 7), 1, "a chance node has put[0] != put[1]"))
    for change, k, text in cases:
        rc, err, name = call(lib, S, street, trees, change, device_form=device_form)
        assert rc == lib.PK_E_INVALID_ARG and err == "%s: tree %d: %s" % (name, k, text), (rc, err)
    rc, err, name = call(lib, S, street, trees, device_form=device_form, m=0)  # every tree passes (no spot: nothing runs, no device is needed)
    assert rc in (lib.PK_OK, lib.PK_E_NO_DEVICE), err


@pytest.mark.parametrize("street", [5, 4])
def test_an_unreferenced_bad_tree_is_refused_too(lib, S, street):
    """the one spot names tree 0; tree 2 is the bad one"""
    trees = river_set(S)[:3] if street == 5 else turn_set(S)
    rc, err, name = call(lib, S, street, trees, set_at("kind", (2, 0), 3))
    assert rc == lib.PK_E_INVALID_ARG and err == name + ": tree 2: the root is not a decision node"


@pytest.mark.parametrize("street", [5, 4])
@pytest.mark.parametrize("device_form", [False, True])
def test_the_other_refusals(lib, S, street, device_form):
    trees = river_set(S)[:2] if street == 5 else turn_set(S)[:2]
    for kw, text in ((dict(ntrees=0), "ntrees outside 1 .. 65536"), (dict(ntrees=65537), "ntrees outside 1 .. 65536"), (dict(iters=0), "iters outside 1 .. 4096"),
                     (dict(iters=4097), "iters outside 1 .. 4096"), (dict(m=2 ** 31), "m >= 2^31")) + tuple(
                         (dict(skip=(k,)), "NULL where a pointer is required") for k in ("n", "pot", "tree_of", "kind", "child", "put", "board", "ranges", "status")):
        rc, err, name = call(lib, S, street, trees, device_form=device_form, **kw)
        assert rc == lib.PK_E_INVALID_ARG and err.startswith(name + ": ") and text in err and "tree 0" not in err, (kw, rc, err)


def test_the_row_helpers_agree_with_python(lib, S):
    L = lib.lib()
    rng = np.random.default_rng(0x7472)
    river, turn = river_set(S), turn_set(S)
    for pick in ([0], [1], [1, 2], [2, 1, 4], [3, 1], list(range(5))):
        trees = [river[i] for i in pick]
        rows = S._TreeRows(trees, 64)
        rows.kind[np.arange(len(trees)), -1] = rng.integers(0, 2, len(trees))  # (an entry past n is ignored: the chain tree alone reaches it)
        if 3 in pick:
            rows.kind[pick.index(3), -1] = river[3].kind[-1]
        D = ctypes.c_uint32(99)
        assert L.pk_rs_trees_rows(len(trees), lib.ptr(rows.n), lib.ptr(rows.kind), ctypes.byref(D)) == lib.PK_OK
        assert D.value == max(len(t.decision_nodes) for t in trees), pick
    for pick in ([0], [1], [2], [1, 2], [2, 0, 1]):
        trees = [turn[i] for i in pick]
        rows = S._TreeRows(trees, 128)
        Dt, Dr = ctypes.c_uint32(99), ctypes.c_uint32(99)
        assert L.pk_ts_trees_rows(len(trees), lib.ptr(rows.n), lib.ptr(rows.kind), lib.ptr(rows.child), ctypes.byref(Dt), ctypes.byref(Dr)) == lib.PK_OK
        assert (Dt.value, Dr.value) == (max(len(t.decision_nodes) for t in trees), max(len(t.river_decision_nodes) for t in trees)), pick
    D = ctypes.c_uint32(0)
    n = np.array([3, 0], np.uint32)
    assert L.pk_rs_trees_rows(2, lib.ptr(n), lib.ptr(np.zeros((2, 64), np.uint8)), ctypes.byref(D)) == lib.PK_E_INVALID_ARG
    assert L.pk_last_error(None).decode() == "pk_rs_trees_rows: tree 1: n outside 1 .. 64"
    assert L.pk_rs_trees_rows(0, lib.ptr(n), lib.ptr(np.zeros((2, 64), np.uint8)), ctypes.byref(D)) == lib.PK_E_INVALID_ARG
    assert L.pk_ts_trees_rows(1, lib.ptr(n), None, None, ctypes.byref(D), ctypes.byref(D)) == lib.PK_E_INVALID_ARG
    for child in (2, 0, 20):                                                  # a child index <= its parent (node 2), or >= n
        rows = S._TreeRows(turn[1:2], 128)
        rows.child[0, 2, 1] = child
        assert L.pk_ts_trees_rows(1, lib.ptr(rows.n), lib.ptr(rows.kind), lib.ptr(rows.child), ctypes.byref(D), ctypes.byref(D)) == lib.PK_E_INVALID_ARG
        assert L.pk_last_error(None).decode() == "pk_ts_trees_rows: tree 0: a child index is <= its parent or >= n"


def test_river_trees_and_turn_trees_build_one_tree_per_distinct_pair(S):
    pots = np.array([100, 40, 100, 100, 40, 7])
    stacks = np.array([400, 30, 400, 50, 30, 7])
    trees, tree_of = S.river_trees(pots, stacks)
    assert tree_of.dtype == np.uint32 and tree_of.tolist() == [0, 1, 0, 2, 1, 3] and len(trees) == 4
    for i in range(len(pots)):
        want, got = S.river_tree(int(pots[i]), int(stacks[i])), trees[tree_of[i]]
        assert got.pot == want.pot and (got.kind == want.kind).all() and (got.child == want.child).all() and (got.put == want.put).all()
    one, of = S.river_trees(pots[:3], stacks[:3], (1.0,), 1)
    assert of.tolist() == [0, 1, 0] and one[1].n == S.river_tree(40, 30, (1.0,), 1).n == 9
    tt, of = S.turn_trees(pots, stacks, (1.0,), 1)
    assert of.tolist() == [0, 1, 0, 2, 1, 3] and all(isinstance(t, S.TurnTree) for t in tt)
    want = S.turn_tree(40, 30, (1.0,), 1)
    assert tt[1].pot == 40 and (tt[1].kind == want.kind).all() and (tt[1].put == want.put).all()
    with pytest.raises(ValueError, match="same shape"):
        S.river_trees([1, 2], [3])


def test_tree_rows_and_tree_of(S):
    trees = river_set(S)
    rows = S._TreeRows(trees, 64)
    assert rows.n.tolist() == [39, 3, 11, 64, 9] and rows.kind.shape == (5, 64) and rows.child.shape == (5, 64, 4) and rows.put.shape == (5, 64, 2)
    assert (rows.child[1, 3:] == FF).all() and (rows.kind[1, :3] == trees[1].kind).all() and rows.pot.tolist() == [100, 77, 100, 60, 40]
    assert S._tree_of(None, 5, 5).tolist() == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match="one tree per spot"):
        S._tree_of(None, 5, 4)
    with pytest.raises(ValueError, match=r"shape \[m\]"):
        S._tree_of([0, 1], 5, 3)
    for bad in ([0, -1, 2], [0, 2 ** 32, 1], [0.0, 1.0, 2.0]):                  # nothing wraps around in the cast to uint32
        with pytest.raises(ValueError, match="tree_of must"):
            S._tree_of(np.array(bad), 5, 3)
    assert S._tree_of(np.array([0, 0xFFFFFFFF, 5], np.int64), 5, 3).tolist() == [0, 0xFFFFFFFF, 5]      # (an index that names no tree is the library's to report)
    with pytest.raises(ValueError, match="needs a sequence of trees"):
        S.solve_river_batch(np.zeros((1, 5), np.uint8), np.zeros((1, 2, H), np.uint16), trees[0], 1, tree_of=[0])
    with pytest.raises(ValueError, match="needs tree_of"):
        S.solve_river_d(1, 0, 0, trees, 1)
    with pytest.raises(ValueError, match="more than 64 nodes"):
        S._TreeRows(trees[:1] + [S.RiverTree([0] * 65, [[FF] * 4] * 65, [[0, 0]] * 65, 1)], 64)


def test_a_batch_solution_slices_to_the_spots_own_tree(S):
    """no device: the batch is put together by hand, as solve_river_batch / solve_turn_batch return it"""
    trees = river_set(S)
    tree_of = np.array([1, 3, 0, 7], np.uint32)
    m, Dmax = 4, 32
    rng = np.random.default_rng(0x736c)
    strategy = rng.integers(0, 32768, (m, Dmax, 4, H)).astype(np.uint16)
    value, br = rng.integers(-99, 99, (m, 2, H)), rng.integers(-99, 99, (m, 2, H))
    ranges, valid = np.ones((m, 2, H), np.uint16), np.ones((m, H), bool)
    batch = S.RiverSolution(None, ranges, strategy, value, br, np.array([0, 0, 0, 32], np.uint8), valid, trees, tree_of)
    for i, (k, D) in enumerate(((1, 2), (3, 32), (0, 14))):
        one = batch[i]
        assert one.tree is trees[k] and one.trees is None and one.strategy.shape == (D, 4, H) and (one.strategy == strategy[i, :D]).all()
        assert (one.value == value[i]).all() and one.status == 0
        node = trees[k].decision_nodes[-1]
        assert one.probabilities(node).shape == (trees[k].num_actions(node), H)
        assert isinstance(one.ev[0], float) and isinstance(one.exploitability, float)
    assert batch[3].tree is None and batch[3].strategy.shape == (0, 4, H) and batch[3].status == 32
    with pytest.raises(ValueError, match="index the batch first"):
        batch.ev
    tt = turn_set(S)
    of = np.array([2, 1], np.uint32)
    strategy, rstrat = rng.integers(0, 9, (2, 4, 4, H)).astype(np.uint16), rng.integers(0, 9, (2, 12, 52, 4, H)).astype(np.uint16)
    tb = S.TurnSolution(None, ranges[:2], strategy, rstrat, value[:2], br[:2], np.zeros(2, np.uint8), valid[:2], np.array([9, 9]), tt, of)
    assert tb[0].tree is tt[2] and tb[0].river_strategy.shape == (4, 52, 4, H) and tb[1].river_strategy.shape == (2, 52, 4, H)
    assert (tb[1].river_strategy == rstrat[1, :2]).all() and tb[1].strategy.shape == (3, 4, H)
    assert tb[1].probabilities(tt[1].river_decision_nodes[0], river_card=0x00).shape == (1, H)
    single = S.RiverSolution(trees[0], ranges, strategy, value, br, np.zeros(m, np.uint8), valid)
    assert single[1].tree is trees[0] and single.trees is None                # one tree for the call: as before


def test_the_new_kernels_exist_without_scratch(lib):
    """`.private_segment_fixed_size` == 0 and no spilled VGPR, LDS as the one-tree kernels': the tree-per-spot kernels are the same bodies"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(lib.LIB_PATH)
    new = {k: d for k, d in ks.items() if k.startswith("k_trees_")}
    assert sorted(new) == ["k_trees_prep", "k_trees_river_solve", "k_trees_turn_solve"], sorted(new)
    assert all(d["private_segment"] == 0 and d["vgpr_spill"] == 0 for d in new.values()), new
    assert new["k_trees_river_solve"]["lds"] == ks["k_river_solve"]["lds"] and new["k_trees_turn_solve"]["lds"] == ks["k_turn_solve"]["lds"]
    assert new["k_trees_prep"]["lds"] == 0
    assert all(new[k]["vgprs"] <= 256 for k in new)                           # two waves per SIMD, as __launch_bounds__(512, 2) asks
