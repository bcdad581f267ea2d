"""CPU tests of the river solver (no GPU): every refusal of a tree and its text, river_tree's shapes, the invariants of the numpy
restatement (river_solver_spec.py) -- rows that sum to one, br >= value, exploitability that falls, nuts against air -- the float64 best
response written from the payoffs against the integer one, the entry points in the header and the binding, and the kernels in the built
library's code objects."""
import os
import re
import sys

import numpy as np
import pytest

import river_solver_spec as RS
import rvr_spec as VS
from oracle import loader as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pk_solve_river_d", "pk_solve_river")
H = RS.HOLDINGS
# The largest |integer exploitability - float64 exploitability| over WITNESS_CASES below is 6.8e-4 chips (measured on the spec, listed in
# DESIGN.md section 3.12); the bound is four times that.  The gap is what the floors of the reaches and of the values lose on one pass:
# it grows with the depth of the tree and does not compound across iterations.
WITNESS_BOUND = 4 * 6.8e-4
WITNESS_CASES = [(9, 1), (9, 16), (9, 64), (16, 1), (16, 16), (24, 1), (24, 16), (24, 64)]     # (pool, iterations), default tree


@pytest.fixture(scope="module")
def lib():
    from pokerl_amd import _lib, build
    build.build_lib()
    return _lib


def default_tree():
    from pokerl_amd.solver import river_tree
    return river_tree(100, 400)


def spot(rng, pool):
    board, _, dead = VS.random_boards(rng, 1, 5, pool)
    return [int(x) for x in board[0]], int(dead[0])


def call(lib, kind, child, put, pot=10, iters=1, n=None, m=1, skip=()):
    """pk_solve_river with the given tree on one well-formed spot -> (return code, error text); nothing reaches a device when it refuses"""
    kind, child, put = np.asarray(kind, np.uint8), np.asarray(child, np.uint8), np.asarray(put, np.uint32)
    board, dead, ranges, status = np.array([[0x00, 0x01, 0x02, 0x03, 0x04]], np.uint8), np.zeros(1, np.uint64), np.ones((1, 2, H), np.uint16), np.zeros(1, np.uint8)
    args = dict(board=board, ranges=ranges, kind=kind, child=child, put=put, status=status)
    p = {k: (None if k in skip else lib.ptr(v)) for k, v in args.items()}
    rc = lib.lib().pk_solve_river(0, m, p["board"], lib.ptr(dead), p["ranges"], len(kind) if n is None else n, p["kind"], p["child"], p["put"], pot, iters,
                                  None, None, None, p["status"])
    return rc, lib.lib().pk_last_error(None).decode()


FF = 0xFF
GOOD = dict(kind=[0, 1, 4], child=[[1, FF, FF, FF], [2, FF, FF, FF], [FF] * 4], put=[[0, 0]] * 3)


@pytest.mark.parametrize("change, text", [
    (dict(kind=[4, 1, 4]), "the root is not a decision node"),
    (dict(kind=[2, 1, 4]), "the root is not a decision node"),
    (dict(child=[[1, FF, FF, FF], [1, FF, FF, FF], [FF] * 4]), "a child index is <= its parent or >= n"),
    (dict(child=[[1, FF, FF, FF], [3, FF, FF, FF], [FF] * 4]), "a child index is <= its parent or >= n"),
    (dict(child=[[1, 2, FF, FF], [2, FF, FF, FF], [FF] * 4]), "a non-root node does not have exactly one parent"),
    (dict(kind=[0, 1, 4, 4], child=[[1, FF, FF, FF], [2, FF, FF, FF], [FF] * 4, [FF] * 4], put=[[0, 0]] * 4), "a non-root node does not have exactly one parent"),
    (dict(kind=[0, 3, 4], child=[[1, FF, FF, FF], [2, FF, FF, FF], [FF] * 4]), "a terminal has a child"),
    (dict(child=[[1, FF, FF, FF], [FF] * 4, [FF] * 4]), "a decision node has no child"),
    (dict(child=[[FF, 1, FF, FF], [2, FF, FF, FF], [FF] * 4]), "a node's children are not packed first"),
    (dict(put=[[0, 0], [0, 0], [5, 4]]), "a showdown has put[0] != put[1]"),
    (dict(put=[[0, 0], [0, 0], [8182, 8182]]), "pot + max put > 8191"),
    (dict(pot=8192), "pot + max put > 8191"),
    (dict(put=[[0, 0], [0, 0], [0xFFFFFFFF, 0xFFFFFFFF]]), "pot + max put > 8191"),
    (dict(kind=[0, 1, 5]), "a node kind outside 0 .. 4"),
    (dict(iters=0), "iters outside 1 .. 4096"),
    (dict(iters=4097), "iters outside 1 .. 4096"),
    (dict(n=0), "n outside 1 .. 64"),
    (dict(n=65), "n outside 1 .. 64"),
    (dict(skip=("kind",)), "NULL where a pointer is required"),
    (dict(skip=("child",)), "NULL where a pointer is required"),
    (dict(skip=("put",)), "NULL where a pointer is required"),
    (dict(skip=("board",)), "NULL where a pointer is required"),
    (dict(skip=("ranges",)), "NULL where a pointer is required"),
    (dict(skip=("status",)), "NULL where a pointer is required"),
])
def test_every_refusal_and_its_text(lib, change, text):
    rc, err = call(lib, **dict(GOOD, **change))
    assert rc == lib.PK_E_INVALID_ARG and err.startswith("pk_solve_river: ") and text in err, (rc, err)


def test_the_device_form_refuses_the_same_way(lib):
    one = np.zeros(64, np.uint8)
    kind, child, put = (np.asarray(GOOD[k], t) for k, t in (("kind", np.uint8), ("child", np.uint8), ("put", np.uint32)))
    L = lib.lib()
    rc = L.pk_solve_river_d(0, 1, lib.ptr(one), None, lib.ptr(one), 3, lib.ptr(kind), lib.ptr(child), lib.ptr(put), 10, 0, None, None, None, lib.ptr(one), None)
    assert rc == lib.PK_E_INVALID_ARG and L.pk_last_error(None).decode() == "pk_solve_river_d: iters outside 1 .. 4096"
    rc = L.pk_solve_river_d(0, 2 ** 31, lib.ptr(one), None, lib.ptr(one), 3, lib.ptr(kind), lib.ptr(child), lib.ptr(put), 10, 1, None, None, None, lib.ptr(one), None)
    assert rc == lib.PK_E_INVALID_ARG and "m >= 2^31" in L.pk_last_error(None).decode()


def test_header_declares_and_binding_lists_the_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "pokerl_hip.h")).read()
    import ctypes
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in lib.SYMBOLS and hasattr(L, name), name
    assert "River solver" in header and lib.lib().pk_abi_version() == 6


def test_solver_kernels_exist_without_scratch(lib):
    """`.private_segment_fixed_size` == 0 and no spilled VGPR: k_river_solve keeps everything per holding in its work space, on purpose"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(lib.LIB_PATH)
    rs = {k: d for k, d in ks.items() if k.startswith(("k_river_solve", "k_rs_prep"))}
    assert sorted(rs) == ["k_river_solve", "k_rs_prep"], sorted(rs)
    assert all(d["private_segment"] == 0 and d["vgpr_spill"] == 0 for d in rs.values()), rs
    assert 32768 < rs["k_river_solve"]["lds"] <= 65536, rs["k_river_solve"]["lds"]


@pytest.mark.parametrize("args, n, decisions, widest", [
    ((100, 400), 39, 14, 4),
    ((100, 400, (0.5, 1.0), 0), 3, 2, 1),
    ((100, 400, (0.5, 1.0), 1), 15, 6, 3),
    ((100, 50), 9, 4, 2),
    ((1001, 7190, (8.0,), 1), 9, 4, 2),
])
def test_river_tree_shapes(lib, args, n, decisions, widest):
    from pokerl_amd import solver as S
    t = S.river_tree(*args)
    assert (t.n, len(t.decision_nodes), max(t.num_actions(v) for v in range(t.n))) == (n, decisions, widest)
    assert t.kind.dtype == np.uint8 and t.child.shape == (n, 4) and t.put.dtype == np.uint32 and t.put.shape == (n, 2)
    assert int(t.put.max()) <= args[1] and t.label(0) == ""
    rc, err = call(lib, t.kind, t.child, t.put, pot=t.pot, m=0)               # the library's own check accepts it (no spot: nothing runs)
    assert rc in (lib.PK_OK, lib.PK_E_NO_DEVICE), err
    for v in range(t.n):
        if t.kind[v] == 4:
            assert t.put[v, 0] == t.put[v, 1], t.label(v)
        if t.kind[v] in (2, 3):
            assert t.put[v, t.kind[v] - 2] < t.put[v, 3 - t.kind[v]], t.label(v)      # the folder faced a bet


def test_river_tree_labels_and_limits():
    from pokerl_amd import solver as S
    t = S.river_tree(100, 400)
    labels = [t.label(v) for v in range(t.n)]
    assert labels[1] == "0:check" and "0:check 1:bet 50" in labels and "0:bet 100 1:raise 300 0:call" in labels and len(set(labels)) == t.n
    with pytest.raises(ValueError, match="more than 64 nodes"):
        S.river_tree(100, 4000, (0.25, 0.5, 1.0), 4)


def test_spec_rows_sum_to_one_and_br_is_at_least_value():
    rng = np.random.default_rng(0x5253)
    tree = default_tree()
    for pool, iters in ((4, 3), (9, 5), (20, 2)):
        board, dead = spot(rng, pool)
        w = rng.integers(0, 65536, (2, H)).astype(np.uint16)
        w[:, rng.integers(0, H, 300)] = 0
        r = RS.solve_spot(board, w, tree, iters, dead)
        v = r["valid"]
        assert r["status"] == 0 and v.sum() == pool * (pool - 1) // 2
        assert (r["strategy"].astype(np.int64).sum(axis=1)[:, v] == RS.ONE).all() and not r["strategy"][:, :, ~v].any()
        assert (r["br"][:, v] >= r["value"][:, v]).all() and not r["br"][:, ~v].any() and not r["value"][:, ~v].any()
        zero = v & (w[0] == 0)                                               # a valid holding of weight 0: the uniform row at the root
        assert zero.any() and (r["strategy"][0, 1:3, zero] == RS.ONE // 3).all()


def test_spec_exploitability_falls():
    rng = np.random.default_rng(0x5254)
    board, dead = spot(rng, 12)
    w = rng.integers(0, 65536, (2, H)).astype(np.uint16)
    tree = default_tree()
    expl = []
    for iters in (16, 64, 256):
        r = RS.solve_spot(board, w, tree, iters, dead)
        expl.append(RS.exploitability(w, r["value"], r["br"], r["valid"]))
    assert expl[0] > expl[1] > expl[2] > 0, expl


def test_nuts_against_air():
    """Every holding of player 0's range beats every holding of player 1's: player 0 collects the pot, give or take the exploitability."""
    rng = np.random.default_rng(0x5255)
    board, dead = spot(rng, 20)
    _, gone = RS.check_spot(board, dead)
    hidx, beats, ties, loses = RS.pairwise(board, gone)
    strength = beats.sum(axis=1) - loses.sum(axis=1)
    order = np.argsort(strength, kind="stable")
    air, nuts = order[:50], order[-50:]
    meet = (beats + ties + loses)[np.ix_(nuts, air)] > 0
    assert (beats[np.ix_(nuts, air)] > 0)[meet].all() and meet.any()         # every pair that can meet is won by the nuts
    w = np.zeros((2, H), np.uint16)
    w[0, hidx[nuts]] = rng.integers(1, 65536, 50)
    w[1, hidx[air]] = rng.integers(1, 65536, 50)
    tree = default_tree()
    r = RS.solve_spot(board, w, tree, 64, dead)
    expl = RS.exploitability(w, r["value"], r["br"], r["valid"])
    ev = RS.ev(w, r["value"], r["valid"])
    assert tree.pot - expl <= ev[0] <= tree.pot + expl, (ev, expl)


def witness_gaps():
    rng = np.random.default_rng(0x5256)
    tree = default_tree()
    gaps = []
    for pool, iters in WITNESS_CASES:
        board, dead = spot(rng, pool)
        w = rng.integers(0, 65536, (2, H)).astype(np.uint16)
        r = RS.solve_spot(board, w, tree, iters, dead)
        exact = RS.exploitability(w, r["value"], r["br"], r["valid"])
        gaps.append((pool, iters, exact, exact - RS.float_exploitability(board, w, tree, r["strategy"], dead)))
    return gaps


def test_float_best_response_agrees_with_the_integer_one():
    gaps = witness_gaps()
    for g in gaps:
        print("pool %d, %d iterations: exploitability %.6f chips, integer - float %.3e" % g)
    assert max(abs(g[3]) for g in gaps) <= WITNESS_BOUND, gaps
