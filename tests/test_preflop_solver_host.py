"""The pre-flop solver without a GPU (include/pokerl_hip.h "Pre-flop solver"): the tree builders, every refusal of the
host check with its text -- which is made before any device is looked at --, the entry points in header, binding and library, the kernel's
code object (no scratch), the float witness of tests/preflop_solver_spec.py on a synthetic table, and holding_class / by_class."""
import os
import re
import sys

import numpy as np
import pytest

import preflop_solver_spec as PFS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pk_solve_preflop_d", "pk_solve_preflop")
H = PFS.HOLDINGS
# The largest |integer exploitability - float64 exploitability| over WITNESS_CASES is 8.2e-6 chips (measured on the spec, every value listed in
# DESIGN.md section 3.18); the bound is four times that.  Smaller than the river solver's because the floor of a showdown is taken once on
# (pot + 2c) E / B and a pre-flop tree's reaches start as large.
WITNESS_BOUND = 4 * 8.2e-6
WITNESS_ITERS = (1, 16, 64)


@pytest.fixture(scope="module")
def lib():
    from pokerl_amd import _lib, build
    build.build_lib()
    return _lib


# ------------------------------------------------------------------------------------------------ builders
def test_push_fold_tree():
    from pokerl_amd.solver import push_fold_tree
    t = push_fold_tree(40)
    assert t.n == 5 and t.kind.tolist() == [0, 2, 1, 3, 4] and t.decision_nodes == [0, 2] and t.pot == 0
    assert t.put.tolist() == [[1, 2], [1, 2], [40, 2], [40, 2], [40, 40]]
    assert t.child.tolist() == [[1, 2, 255, 255], [255] * 4, [3, 4, 255, 255], [255] * 4, [255] * 4]
    assert [t.label(i) for i in range(5)] == ["", "0:fold", "0:jam", "0:jam 1:fold", "0:jam 1:call"]
    t = push_fold_tree(300, 50, 100, 10)
    assert t.put[0].tolist() == [50, 100] and t.pot == 20 and t.put[4].tolist() == [300, 300]
    for bad in ((1, 1, 2), (10, 0, 2), (10, 3, 2), (10, 1, 2, -1)):
        with pytest.raises(ValueError):
            push_fold_tree(*bad)


@pytest.mark.parametrize("args, n, decisions", [
    ((200,), 22, 8),
    ((200, 1, 2, 0, (1.0,), 3, False), 11, 4),
    ((12, 1, 2, 0, (1.0,), 2), 16, 6),
    ((40, 1, 2, 0, (0.75, 2.0), 3), 64, 22),
    ((2, 1, 2), 4, 2),
])
def test_preflop_tree_shapes(args, n, decisions):
    from pokerl_amd.solver import preflop_tree
    t = preflop_tree(*args)
    stack = args[0]
    assert t.n == n and len(t.decision_nodes) == decisions and t.n <= 64
    assert t.kind[0] == 0 and t.put[0].tolist() == [1, 2] and t.pot == 0            # the blinds are the root's put
    assert int(t.put.max()) <= stack                                                # amounts are capped at the stack
    shows = [i for i in range(t.n) if t.kind[i] == 4]
    assert shows and all(t.put[i][0] == t.put[i][1] for i in shows)                 # every showdown has equal puts
    assert all(t.num_actions(d) <= 4 for d in t.decision_nodes)


def test_preflop_tree_limp_line_and_labels():
    from pokerl_amd.solver import preflop_tree, preflop_trees
    t = preflop_tree(200)
    assert [t.label(c) for c in t.child[0][:3]] == ["0:fold", "0:call", "0:raise 4"]
    limp = int(t.child[0][1])
    assert t.kind[limp] == 1 and t.put[limp].tolist() == [2, 2]                     # after a limp player 1 acts: check (a showdown) or raise
    check = int(t.child[limp][0])
    assert t.kind[check] == 4 and t.label(check) == "0:call 1:check" and t.put[check].tolist() == [2, 2]
    assert t.kind[int(t.child[limp][1])] == 0
    nolimp = preflop_tree(200, limp=False)
    assert [nolimp.label(c) for c in nolimp.child[0][:2]] == ["0:fold", "0:raise 4"] and nolimp.num_actions(0) == 2
    ante = preflop_tree(200, 1, 2, 3)
    assert ante.pot == 6 and ante.put[0].tolist() == [1, 2]
    with pytest.raises(ValueError, match="more than 64 nodes"):
        preflop_tree(400, 1, 2, 0, (0.5, 1.0), 4)
    trees, of = preflop_trees([40, 20, 40, 6], push_fold=True)
    assert of.tolist() == [0, 1, 0, 2] and [int(t.put[4][0]) for t in trees] == [40, 20, 6] and of.dtype == np.uint32
    trees, of = preflop_trees([12, 12, 30], bet_fractions=(1.0,), max_raises=2)
    assert of.tolist() == [0, 0, 1] and trees[0].n == 16


def test_the_river_and_turn_builders_build_what_they_built_before():
    """betting_round gained the root's `limp` for preflop_tree; with the default it is the old rule.  The digest was taken from the
    builders of the commit before the pre-flop solver, over the arrays, the pot and every label of these trees."""
    import hashlib
    from pokerl_amd import solver as S
    h = hashlib.sha256()
    trees = [S.river_tree(*a) for a in ((100, 400), (100, 50), (1001, 7190, (8.0,), 1), (60, 400, (0.5, 1.0), 1), (7, 3, (0.3, 0.6, 1.0), 2))]
    trees += [S.turn_tree(*a) for a in ((100, 400, (1.0,), 1), (30, 20, (1.0,), 1))]
    for t in trees:
        h.update(t.kind.tobytes() + t.child.tobytes() + t.put.tobytes() + repr([t.pot] + [t.label(i) for i in range(t.n)]).encode())
    assert h.hexdigest() == "90185f16b5ef0772a70a3cc1606371124cfa35e6a919ef44de6a5918f1edaee5"


# ------------------------------------------------------------------------------------------------ the host check
FF = 0xFF
GOOD = dict(kind=[0, 1, 4], child=[[1, FF, FF, FF], [2, FF, FF, FF], [FF] * 4], put=[[1, 2], [2, 2], [2, 2]])


def call(lib, kind, child, put, pot=10, iters=1, n=None, m=1, ntrees=1, skip=(), device=0):
    """pk_solve_preflop with the given tree (in row 0 of the tree arrays) -> (return code, error text); nothing reaches a device when it refuses"""
    K = max(ntrees, 1)
    kd, ch, pt = np.zeros((K, 64), np.uint8), np.full((K, 64, 4), FF, np.uint8), np.zeros((K, 64, 2), np.uint32)
    for k in range(K):                                                               # (every row a copy of the good tree, then row 0 the one under test)
        kd[k, :3], ch[k, :3], pt[k, :3] = GOOD["kind"], GOOD["child"], GOOD["put"]
    kd[0, :len(kind)], ch[0, :len(child)], pt[0, :len(put)] = kind, child, put
    nn, pots = np.full(K, 3, np.uint32), np.full(K, pot, np.uint32)
    nn[0] = len(kind) if n is None else n
    ranges, status = np.ones((1, 2, H), np.uint16), np.zeros(1, np.uint8)
    args = dict(ranges=ranges, n=nn, kind=kd, child=ch, put=pt, pot=pots, status=status)
    p = {k: (None if k in skip else lib.ptr(v)) for k, v in args.items()}
    rc = lib.lib().pk_solve_preflop(device, m, p["ranges"], ntrees, p["n"], p["kind"], p["child"], p["put"], p["pot"], None, iters, None, None, None, p["status"])
    return rc, lib.lib().pk_last_error(None).decode()


@pytest.mark.parametrize("change, text", [
    (dict(kind=[4, 1, 4]), "tree 0: the root is not a decision node"),
    (dict(child=[[1, FF, FF, FF], [1, FF, FF, FF], [FF] * 4]), "tree 0: a child index is <= its parent or >= n"),
    (dict(child=[[1, 2, FF, FF], [2, FF, FF, FF], [FF] * 4]), "tree 0: a non-root node does not have exactly one parent"),
    (dict(kind=[0, 3, 4], child=[[1, FF, FF, FF], [2, FF, FF, FF], [FF] * 4]), "tree 0: a terminal has a child"),
    (dict(child=[[1, FF, FF, FF], [FF] * 4, [FF] * 4]), "tree 0: a decision node has no child"),
    (dict(child=[[FF, 1, FF, FF], [2, FF, FF, FF], [FF] * 4]), "tree 0: a node's children are not packed first"),
    (dict(put=[[1, 2], [2, 2], [5, 4]]), "tree 0: a showdown has put[0] != put[1]"),
    (dict(put=[[1, 2], [2, 2], [8182, 8182]]), "tree 0: pot + max put > 8191"),
    (dict(pot=8192), "tree 0: pot + max put > 8191"),
    (dict(kind=[0, 1, 5]), "tree 0: a chance node (kind 5)"),
    (dict(kind=[0, 5, 4]), "tree 0: a chance node (kind 5)"),
    (dict(kind=[0, 1, 6]), "tree 0: a given node (kind 6)"),
    (dict(kind=[0, 1, 7]), "tree 0: a node kind outside 0 .. 4"),
    (dict(iters=0), "iters outside 1 .. 4096"),
    (dict(iters=4097), "iters outside 1 .. 4096"),
    (dict(n=0), "tree 0: n outside 1 .. 64"),
    (dict(n=65), "tree 0: n outside 1 .. 64"),
    (dict(ntrees=0), "ntrees outside 1 .. 65536"),
    (dict(ntrees=65537), "ntrees outside 1 .. 65536"),
    (dict(m=2 ** 31), "m >= 2^31"),
    (dict(skip=("kind",)), "NULL where a pointer is required"),
    (dict(skip=("child",)), "NULL where a pointer is required"),
    (dict(skip=("put",)), "NULL where a pointer is required"),
    (dict(skip=("n",)), "NULL where a pointer is required"),
    (dict(skip=("pot",)), "NULL where a pointer is required"),
    (dict(skip=("ranges",)), "NULL where a pointer is required"),
    (dict(skip=("status",)), "NULL where a pointer is required"),
])
def test_every_refusal_and_its_text(lib, change, text):
    rc, err = call(lib, **dict(GOOD, **change))
    assert rc == lib.PK_E_INVALID_ARG and err.startswith("pk_solve_preflop: ") and text in err, (rc, err)


def test_the_check_names_the_tree_and_runs_before_any_device_is_looked_at(lib):
    rc, err = call(lib, **dict(GOOD, kind=[0, 1, 5], device=64))                    # (a device index that does not exist: the tree is refused first)
    assert rc == lib.PK_E_INVALID_ARG and "a chance node (kind 5)" in err
    # a bad tree that no spot names is refused too, by its index
    K = 3
    kd, ch, pt = np.zeros((K, 64), np.uint8), np.full((K, 64, 4), FF, np.uint8), np.zeros((K, 64, 2), np.uint32)
    for k in range(K):
        kd[k, :3], ch[k, :3], pt[k, :3] = GOOD["kind"], GOOD["child"], GOOD["put"]
    kd[2, 2] = 6
    nn, pots, ranges, status = np.full(K, 3, np.uint32), np.zeros(K, np.uint32), np.ones((1, 2, H), np.uint16), np.zeros(1, np.uint8)
    L = lib.lib()
    rc = L.pk_solve_preflop(0, 1, lib.ptr(ranges), K, lib.ptr(nn), lib.ptr(kd), lib.ptr(ch), lib.ptr(pt), lib.ptr(pots), None, 1, None, None, None, lib.ptr(status))
    assert rc == lib.PK_E_INVALID_ARG and L.pk_last_error(None).decode().startswith("pk_solve_preflop: tree 2: a given node (kind 6)")
    rc = L.pk_solve_preflop_d(0, 1, lib.ptr(ranges), K, lib.ptr(nn), lib.ptr(kd), lib.ptr(ch), lib.ptr(pt), lib.ptr(pots), None, 0, None, None, None, lib.ptr(status), None)
    assert rc == lib.PK_E_INVALID_ARG and L.pk_last_error(None).decode() == "pk_solve_preflop_d: iters outside 1 .. 4096"


def test_header_declares_and_binding_lists_the_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "pokerl_hip.h")).read()
    import ctypes
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in lib.SYMBOLS and hasattr(L, name), name
    assert "Pre-flop solver" in header and lib.lib().pk_abi_version() == 6
    from pokerl_amd import build
    assert "pk_preflop_solver.hip" in build.SOURCES
    import pokerl_amd
    for name in ("PreflopSolution", "holding_class", "push_fold_tree", "preflop_tree", "preflop_trees", "solve_preflop", "solve_preflop_batch", "solve_preflop_d"):
        assert name in pokerl_amd.__all__ and hasattr(pokerl_amd, name), name


def test_solver_kernel_exists_without_scratch(lib):
    """`.private_segment_fixed_size` == 0 and no spilled VGPR: k_preflop_solve keeps everything per holding in its work space, on purpose"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(lib.LIB_PATH)
    ps = {k: d for k, d in ks.items() if k.startswith("k_preflop_solve")}
    assert sorted(ps) == ["k_preflop_solve"], sorted(ps)
    d = ps["k_preflop_solve"]
    assert d["private_segment"] == 0 and d["vgpr_spill"] == 0, d
    assert 32768 < d["lds"] <= 65536, d["lds"]                                       # (both reach vectors, the showdown's sums, the tree)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3.18" in design and "k_preflop_solve" in design


# ------------------------------------------------------------------------------------------------ the spec, and its float witness
@pytest.fixture(scope="module")
def table():
    t = PFS.synthetic_table(7)
    win, tie = (np.asarray(x, np.int64) for x in t)
    assert not (win * PFS.SHARE).any() and not (tie * PFS.SHARE).any() and (tie == tie.T).all()
    assert ((win + win.T + tie) == PFS.BOARDS * PFS.DISJOINT).all()                 # the real table's structure
    return t


def random_ranges(seed):
    rng = np.random.default_rng(seed)
    ranges = rng.integers(0, 65536, (2, H)).astype(np.uint16)
    for row in ranges:
        row[rng.integers(0, H, 200)] = 0
        row[rng.integers(0, H, 100)] = 65535
    return ranges


def witness_trees():
    from pokerl_amd.solver import preflop_tree, push_fold_tree
    return {"push_fold_tree(20)": push_fold_tree(20), "preflop_tree(12, 1, 2, 0, (1.0,), 2)": preflop_tree(12, 1, 2, 0, (1.0,), 2)}


def test_float_best_response_agrees_with_the_integer_one(table):
    """Integer minus float exploitability, measured on the restatement: push_fold_tree(20) 2.3e-10, 1.2e-7, 1.0e-9 and
    preflop_tree(12, 1, 2, 0, (1.0,), 2) -8.2e-6, 6.9e-7, 1.4e-7 chips at 1 / 16 / 64 iterations (exploitabilities 3.2 ... 0.0026 chips)."""
    ranges, G = random_ranges(11), PFS.weight_matrix(table)
    worst = 0.0
    for name, tree in witness_trees().items():
        curve = []
        for iters in WITNESS_ITERS:
            r = PFS.solve_spot(table, ranges, tree, iters, G=G)
            assert (r["strategy"].astype(np.int64).sum(axis=1) == PFS.ONE).all()
            assert (r["br"] >= r["value"]).all()
            ie = PFS.exploitability(ranges, r["value"], r["br"])
            fe = PFS.float_exploitability(table, ranges, tree, r["strategy"])
            print("%s, %d iterations: integer %.6f, float %.6f, difference %.3e chips" % (name, iters, ie, fe, ie - fe))
            worst = max(worst, abs(ie - fe))
            curve.append(ie)
        assert curve[0] > curve[1] > curve[2] > 0, curve                             # and it converges
    assert worst <= WITNESS_BOUND, worst


def test_a_showdown_is_the_all_in_equity(table):
    """One decision, one showdown: value[p][h] is the showdown formula from the table, in Python integers."""
    from pokerl_amd.solver import RiverTree
    tree = RiverTree([0, 4], [[1, FF, FF, FF], [FF] * 4], [[3, 5], [5, 5]], 7)
    ranges = random_ranges(12)
    r = PFS.solve_spot(table, ranges, tree, 1)
    win, tie = (np.asarray(x, np.int64) for x in table)
    for p in (0, 1):
        rq = [int(x) << 4 for x in ranges[1 - p]]
        for h in (0, 1, 700, 1325):
            E = sum(rq[o] * (2 * int(win[h, o]) + int(tie[h, o])) for o in range(H))
            S = sum(rq[o] for o in range(H) if not PFS.SHARE[h, o])
            assert int(r["value"][p, h]) == (7 + 10) * E // PFS.BOARDS - 10 * S
    assert (r["value"] == r["br"]).all() and (r["strategy"][0, 0] == PFS.ONE).all() and not r["strategy"][0, 1:].any()


def test_batch_strides_and_bad_tree(table):
    from pokerl_amd.solver import push_fold_tree
    trees = [push_fold_tree(6), witness_trees()["preflop_tree(12, 1, 2, 0, (1.0,), 2)"]]
    ranges = np.stack([random_ranges(13), random_ranges(14), random_ranges(15)])
    r = PFS.solve_batch(table, ranges, trees, 1, [0, 2, 1])
    assert r["status"].tolist() == [0, PFS.BAD_TREE, 0] and r["strategy"].shape == (3, 6, 4, H)
    assert not r["strategy"][1].any() and not r["value"][1].any() and not r["br"][1].any() and not r["valid"][1].any()
    assert r["strategy"][0, :2].any() and not r["strategy"][0, 2:].any() and r["strategy"][2, 5].any()
    alone = PFS.solve_spot(table, ranges[0], trees[0], 1)
    assert (r["strategy"][0, :2] == alone["strategy"]).all() and (r["value"][0] == alone["value"]).all()


# ------------------------------------------------------------------------------------------------ holding_class / by_class
def test_holding_class():
    from pokerl_amd.judger import holding_index
    from pokerl_amd.solver import holding_class
    cls = holding_class(np.arange(H))
    grid = np.bincount(cls, minlength=169).reshape(13, 13)
    assert cls.min() == 0 and cls.max() == 168
    assert (np.diag(grid) == 6).all() and (np.tril(grid, -1)[np.tril_indices(13, -1)] == 4).all() and (np.triu(grid, 1)[np.triu_indices(13, 1)] == 12).all()
    # canonical index = 4 * rank0 + suit, rank0 0 the ace: aces 0 .. 3, deuces 4 .. 7, kings 48 .. 51
    def h(a, b):
        a, b = min(a, b), max(a, b)
        return b * (b - 1) // 2 + a
    assert holding_class(h(0, 1)) == 13 * 12 + 12 and isinstance(holding_class(h(0, 1)), int)          # aces
    assert holding_class(h(0, 48)) == 13 * 12 + 11                                    # ace-king suited: (hi, lo)
    assert holding_class(h(0, 49)) == 13 * 11 + 12                                    # ace-king off-suit: (lo, hi)
    assert holding_class(h(4, 5)) == 0 and holding_class(h(7, 11)) == 13 * 1 + 0 and holding_class(h(6, 11)) == 1     # deuces, 32 suited, 32 off-suit
    assert holding_class(holding_index("AS", "KS")) == 13 * 12 + 11 and holding_class(holding_index("2D", "2C")) == 0
    assert holding_index is not None


def test_by_class_on_hand_made_strategies():
    from pokerl_amd.solver import PreflopSolution, holding_class, push_fold_tree
    tree = push_fold_tree(20)
    cls = holding_class(np.arange(H))
    ranges = np.zeros((2, H), np.uint16)
    ranges[0] = 100
    ranges[1] = 7
    aces = np.nonzero(cls == 168)[0]
    ranges[0, aces] = [1, 2, 3, 0, 0, 4]                                               # the actor's weights inside one class
    ranges[0, cls == 0] = 0                                                            # a class the actor never holds
    strategy = np.zeros((2, 4, H), np.uint16)
    strategy[0, 0], strategy[0, 1] = 32768, 0                                          # the root: fold everything ...
    jam = np.zeros(H, np.uint16)
    jam[aces] = [32768, 0, 16384, 32768, 0, 8192]                                      # ... but some of the aces
    strategy[0, 1], strategy[0, 0] = jam, 32768 - jam
    strategy[1, 0], strategy[1, 1] = 8192, 24576                                       # player 1: call three quarters, whatever it holds
    sol = PreflopSolution(tree, ranges, strategy, np.zeros((2, H), np.int64), np.zeros((2, H), np.int64), np.uint8(0), np.ones(H, bool))
    root = sol.by_class(0)
    assert root.shape == (2, 13, 13)
    want = (1 * 1.0 + 2 * 0.0 + 3 * 0.5 + 4 * 0.25) / 10
    assert root[1, 12, 12] == pytest.approx(want) and root[0, 12, 12] == pytest.approx(1 - want)
    assert np.isnan(root[:, 0, 0]).all()                                               # no weight in the class: nan
    assert root[0, 5, 3] == 1.0 and root[1, 5, 3] == 0.0
    call = sol.by_class(2)                                                             # weighted by PLAYER 1's range there
    assert np.allclose(call[1], 0.75) and np.allclose(call[0], 0.25) and not np.isnan(call).any()
    with pytest.raises(ValueError):
        sol.by_class(1)                                                                # not a decision node
