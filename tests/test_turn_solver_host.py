"""CPU tests of the turn solver (no GPU): every refusal of a tree and its text, turn_tree's shapes, the invariants of the numpy
restatement (turn_solver_spec.py) -- rows that sum to one, br >= value, zeros where the definition says so, the regret bound at the
magnitude edge, exploitability that falls -- the float64 best response written from the payoffs against the integer one, the entry points
in the header and the binding, and the kernels in the built library's code objects."""
import os
import re
import sys

import numpy as np
import pytest

import rvr_spec as VS
import turn_solver_spec as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pk_solve_turn_d", "pk_solve_turn")
H = TS.HOLDINGS
FF = 0xFF
# The largest |integer exploitability - float64 exploitability| over WITNESS_CASES below is 5.6e-3 chips (measured on the spec, listed in
# DESIGN.md section 3.13); the bound is four times that.  The gap is what the floors of the reaches (which start at weight << 1 here, not
# << 4) and of the values lose on one pass; it does not compound across iterations.
WITNESS_BOUND = 4 * 5.6e-3
WITNESS_CASES = [(9, 1), (9, 16), (9, 64), (14, 1), (14, 16), (14, 64)]       # (pool, iterations), turn_tree(100, 400, (1.0,), 1)
REGRET_BITS_BOUND = 60                                                        # |R| < 2^59.7 (pokerl_hip.h "Turn solver", BOUNDS)


@pytest.fixture(scope="module")
def lib():
    from pokerl_amd import _lib, build
    build.build_lib()
    return _lib


def witness_tree():
    from pokerl_amd.solver import turn_tree
    return turn_tree(100, 400, (1.0,), 1)


def spot(rng, pool):
    board, _, dead = VS.random_boards(rng, 1, 4, pool)
    return [int(x) for x in board[0, :4]], int(dead[0])


def call(lib, kind, child, put, pot=10, iters=1, n=None, m=1, skip=()):
    """pk_solve_turn with the given tree on one well-formed spot -> (return code, error text); nothing reaches a device when it refuses"""
    kind, child, put = np.asarray(kind, np.uint8), np.asarray(child, np.uint8), np.asarray(put, np.uint32)
    board, dead, ranges, status = np.array([[0x00, 0x01, 0x02, 0x03]], np.uint8), np.zeros(1, np.uint64), np.ones((1, 2, H), np.uint16), np.zeros(1, np.uint8)
    args = dict(board=board, ranges=ranges, kind=kind, child=child, put=put, status=status)
    p = {k: (None if k in skip else lib.ptr(v)) for k, v in args.items()}
    rc = lib.lib().pk_solve_turn(0, m, p["board"], lib.ptr(dead), p["ranges"], len(kind) if n is None else n, p["kind"], p["child"], p["put"], pot, iters,
                                 None, None, None, None, p["status"])
    return rc, lib.lib().pk_last_error(None).decode()


E = [FF] * 4
GOOD = dict(kind=[0, 1, 5, 4], child=[[1, FF, FF, FF], [2, FF, FF, FF], [3, FF, FF, FF], E], put=[[0, 0]] * 4)


@pytest.mark.parametrize("change, text", [
    (dict(kind=[5, 1, 5, 4]), "the root is not a decision node"),
    (dict(kind=[2, 1, 5, 4]), "the root is not a decision node"),
    (dict(child=[[1, FF, FF, FF], [1, FF, FF, FF], [3, FF, FF, FF], E]), "a child index is <= its parent or >= n"),
    (dict(child=[[1, FF, FF, FF], [2, FF, FF, FF], [4, FF, FF, FF], E]), "a child index is <= its parent or >= n"),
    (dict(child=[[1, 2, FF, FF], [2, FF, FF, FF], [3, FF, FF, FF], E]), "a non-root node does not have exactly one parent"),
    (dict(kind=[0, 1, 5, 4, 4], child=GOOD["child"] + [E], put=[[0, 0]] * 5), "a non-root node does not have exactly one parent"),
    (dict(kind=[0, 3, 5, 4]), "a terminal has a child"),
    (dict(child=[[1, FF, FF, FF], E, [3, FF, FF, FF], E]), "a decision node has no child"),
    (dict(child=[[FF, 1, FF, FF], [2, FF, FF, FF], [3, FF, FF, FF], E]), "a node's children are not packed first"),
    (dict(put=[[0, 0], [0, 0], [0, 0], [5, 4]]), "a showdown has put[0] != put[1]"),
    (dict(put=[[0, 0], [0, 0], [0, 0], [8182, 8182]]), "pot + max put > 8191"),
    (dict(pot=8192), "pot + max put > 8191"),
    (dict(kind=[0, 1, 5, 6]), "a node kind outside 0 .. 5"),
    (dict(kind=[0, 1, 5, 4, 4], child=[[1, FF, FF, FF], [2, FF, FF, FF], [3, 4, FF, FF], E, E], put=[[0, 0]] * 5), "a chance node does not have exactly one child"),
    (dict(child=[[1, FF, FF, FF], [2, FF, FF, FF], E, E]), "a chance node does not have exactly one child"),
    (dict(kind=[0, 1, 5, 5, 4], child=[[1, FF, FF, FF], [2, FF, FF, FF], [3, FF, FF, FF], [4, FF, FF, FF], E], put=[[0, 0]] * 5), "a chance node below a chance node"),
    (dict(kind=[0, 1, 5, 0, 5, 4], child=[[1, FF, FF, FF], [2, FF, FF, FF], [3, FF, FF, FF], [4, FF, FF, FF], [5, FF, FF, FF], E], put=[[0, 0]] * 6),
     "a chance node below a chance node"),
    (dict(kind=[0, 1, 4], child=[[1, FF, FF, FF], [2, FF, FF, FF], E], put=[[0, 0]] * 3), "a turn-level showdown"),
    (dict(put=[[0, 0], [0, 0], [5, 4], [5, 5]]), "a chance node has put[0] != put[1]"),
    (dict(iters=0), "iters outside 1 .. 4096"),
    (dict(iters=4097), "iters outside 1 .. 4096"),
    (dict(n=0), "n outside 1 .. 128"),
    (dict(n=129), "n outside 1 .. 128"),
    (dict(skip=("kind",)), "NULL where a pointer is required"),
    (dict(skip=("child",)), "NULL where a pointer is required"),
    (dict(skip=("put",)), "NULL where a pointer is required"),
    (dict(skip=("board",)), "NULL where a pointer is required"),
    (dict(skip=("ranges",)), "NULL where a pointer is required"),
    (dict(skip=("status",)), "NULL where a pointer is required"),
])
def test_every_refusal_and_its_text(lib, change, text):
    rc, err = call(lib, **dict(GOOD, **change))
    assert rc == lib.PK_E_INVALID_ARG and err.startswith("pk_solve_turn: ") and text in err, (rc, err)


def test_the_device_form_refuses_the_same_way(lib):
    one = np.zeros(64, np.uint8)
    kind, child, put = (np.asarray(GOOD[k], t) for k, t in (("kind", np.uint8), ("child", np.uint8), ("put", np.uint32)))
    L = lib.lib()
    rc = L.pk_solve_turn_d(0, 1, lib.ptr(one), None, lib.ptr(one), 4, lib.ptr(kind), lib.ptr(child), lib.ptr(put), 10, 0, None, None, None, None, lib.ptr(one), None)
    assert rc == lib.PK_E_INVALID_ARG and L.pk_last_error(None).decode() == "pk_solve_turn_d: iters outside 1 .. 4096"


def test_header_declares_and_binding_lists_the_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "pokerl_hip.h")).read()
    import ctypes
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in lib.SYMBOLS and hasattr(L, name), name
    assert "Turn solver" in header and "#define PK_TS_MAX_NODES 128" in header


def test_solver_kernels_exist_without_scratch(lib):
    """`.private_segment_fixed_size` == 0 and no spilled VGPR: k_turn_solve keeps everything per holding in its work space, on purpose"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(lib.LIB_PATH)
    ts = {k: d for k, d in ks.items() if k.startswith(("k_turn_solve", "k_ts_prep"))}
    assert sorted(ts) == ["k_ts_prep", "k_turn_solve"], sorted(ts)
    print({k: (d.get("vgpr"), d["lds"]) for k, d in ts.items()})
    assert all(d["private_segment"] == 0 and d["vgpr_spill"] == 0 for d in ts.values()), ts
    assert 32768 < ts["k_turn_solve"]["lds"] <= 65536, ts["k_turn_solve"]["lds"]


def test_the_grid_follows_the_work_space_ceiling(lib):
    from pokerl_amd import solver as S
    small = S.turn_tree(100, 50, (0.5,), 1)
    assert S.turn_grid(small) == 256 and S.turn_grid(small, 3) == 3
    big = S.turn_tree(100, 400, (0.5, 1.0, 2.0), 1, (1.0,), 1)
    nr = int(big.river_level.sum())
    per_group = 423936 + (big.n - nr) * 50688 + nr * 866048                   # pokerl_hip.h "Turn solver", work space
    assert S.turn_grid(big) == (4 << 30) // per_group < 256


@pytest.mark.parametrize("args, n, turn_decisions, river_decisions, widest", [
    ((100, 400, (1.0,), 1), 36, 4, 12, 2),
    ((100, 50, (0.5,), 1), 20, 4, 4, 2),
    ((100, 400, (0.5, 1.0, 2.0), 1, (1.0,), 1), 84, 8, 28, 4),
    ((100, 1000, (1.0,), 0, (1.0,), 1), 12, 2, 4, 2),
    ((100, 400, (1.0,), 1, (1.0,), 0), 18, 4, 6, 2),
])
def test_turn_tree_shapes(lib, args, n, turn_decisions, river_decisions, widest):
    from pokerl_amd import solver as S
    t = S.turn_tree(*args)
    assert (t.n, len(t.decision_nodes), len(t.river_decision_nodes), max(t.num_actions(v) for v in range(t.n))) == (n, turn_decisions, river_decisions, widest)
    assert t.kind.dtype == np.uint8 and t.child.shape == (n, 4) and t.put.dtype == np.uint32 and t.put.shape == (n, 2)
    assert int(t.put.max()) <= args[1] and t.label(0) == ""
    rc, err = call(lib, t.kind, t.child, t.put, pot=t.pot, m=0)               # the library's own check accepts it (no spot: nothing runs)
    assert rc in (lib.PK_OK, lib.PK_E_NO_DEVICE), err
    chances = 0
    for v in range(t.n):
        label = t.label(v).split()
        if t.kind[v] == 4:
            assert t.put[v, 0] == t.put[v, 1] and t.river_level[v], t.label(v)
        if t.kind[v] == 5:                                                    # every turn line that ends in a call or in check-check
            chances += 1
            assert not t.river_level[v] and t.put[v, 0] == t.put[v, 1] and t.num_actions(v) == 1
            assert label[-1].endswith(":call") or label[-2:] == ["0:check", "1:check"], label
            child = int(t.child[v, 0])
            assert t.label(child).split()[-1] == "deal"
            assert t.kind[child] == (4 if t.put[v, 0] == args[1] else 0), label      # all-in: a showdown follows directly
        if t.kind[v] in (2, 3):
            assert t.put[v, t.kind[v] - 2] < t.put[v, 3 - t.kind[v]], t.label(v)      # the folder faced a bet
        if not t.river_level[v] and t.kind[v] != 5 and label and (label[-1].endswith(":call") or label[-2:] == ["0:check", "1:check"]):
            pytest.fail("a turn line ends without a chance node: " + t.label(v))
    assert chances >= (1 if args[3] == 0 else 2)                               # (no bet on the turn: check-check alone)


def test_turn_tree_all_in_and_limits():
    from pokerl_amd import solver as S
    t = S.turn_tree(100, 100, (1.0,), 1)                                      # the pot-size bet is all-in
    allin = [v for v in range(t.n) if t.kind[v] == 5 and t.put[v, 0] == 100]
    assert allin and all(t.kind[t.child[v, 0]] == 4 for v in allin)
    assert t.label(allin[0]) == "0:check 1:bet 100 0:call" or t.label(allin[0]) == "0:bet 100 1:call"
    with pytest.raises(ValueError, match="more than 128 nodes"):
        S.turn_tree(100, 400, (0.5, 1.0), 2)


def test_spec_invariants():
    rng = np.random.default_rng(0x5453)
    tree = TS.as_tree(witness_tree())
    for pool, iters in ((5, 3), (9, 5), (14, 2)):
        board, dead = spot(rng, pool)
        w = rng.integers(0, 65536, (2, H)).astype(np.uint16)
        w[:, rng.integers(0, H, 300)] = 0
        r = TS.solve_spot(board, w, tree, iters, dead)
        v = r["valid"]
        assert r["status"] == 0 and r["P"] == pool and v.sum() == pool * (pool - 1) // 2
        assert (r["strategy"].astype(np.int64).sum(axis=1)[:, v] == TS.ONE).all() and not r["strategy"][:, :, ~v].any()
        assert (r["br"][:, v] >= r["value"][:, v]).all() and not r["br"][:, ~v].any() and not r["value"][:, ~v].any()
        _, gone = TS.check_spot(board, dead)
        rows = r["river_strategy"].astype(np.int64).sum(axis=2)                # [D_r, 52, 1326]
        for k in range(52):
            with_k = (VS.PAIR_A == k) | (VS.PAIR_B == k)
            if k in gone:
                assert not r["river_strategy"][:, k].any()
            else:
                assert (rows[:, k][:, v & ~with_k] == TS.ONE).all() and not r["river_strategy"][:, k][:, :, with_k | ~v].any()


def test_spec_regret_bits_at_the_magnitude_edge():
    """all weights 65 535, pot + put = 8191, P = 12"""
    from pokerl_amd.solver import turn_tree
    rng = np.random.default_rng(0x5458)
    board, dead = spot(rng, 12)
    tree = turn_tree(2731, 5460, (1.0,), 1)
    assert tree.pot + int(tree.put.max()) == 8191
    r = TS.solve_spot(board, np.full((2, H), 65535, np.uint16), tree, 16, dead)
    print("regret_bits", r["regret_bits"])
    assert 0 < r["regret_bits"] <= REGRET_BITS_BOUND


def test_spec_exploitability_falls():
    rng = np.random.default_rng(0x5457)
    tree = witness_tree()
    for pool in (9, 12):
        board, dead = spot(rng, pool)
        w = rng.integers(0, 65536, (2, H)).astype(np.uint16)
        expl = []
        for iters in (16, 64):
            r = TS.solve_spot(board, w, tree, iters, dead)
            expl.append(TS.exploitability(w, r["value"], r["br"], r["valid"], r["P"]))
        assert expl[0] > expl[1] > 0, expl


def witness_gaps():
    rng = np.random.default_rng(0x5456)
    tree = witness_tree()
    gaps = []
    for pool, iters in WITNESS_CASES:
        board, dead = spot(rng, pool)
        w = rng.integers(0, 65536, (2, H)).astype(np.uint16)
        r = TS.solve_spot(board, w, tree, iters, dead)
        exact = TS.exploitability(w, r["value"], r["br"], r["valid"], r["P"])
        gaps.append((pool, iters, exact, exact - TS.float_exploitability(board, w, tree, r["strategy"], r["river_strategy"], dead)))
    return gaps


def test_float_best_response_agrees_with_the_integer_one():
    gaps = witness_gaps()
    for g in gaps:
        print("pool %d, %d iterations: exploitability %.6f chips, integer - float %.3e" % g)
    assert max(abs(g[3]) for g in gaps) <= WITNESS_BOUND, gaps
