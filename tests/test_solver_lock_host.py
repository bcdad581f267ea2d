"""CPU tests of the river and turn solvers' locked calls (no GPU; include/pokerl_hip.h "Locked nodes"): the entry
points in the header, the binding and the library; every refusal's text, made before any device is looked at; iters = 0 accepted; lock's
broadcasting, rows_of and a solution as `locked` in Python; the new kernels in the built library's code objects; and the identities 1-5 of
the definition on the restatement itself (tests/solver_lock_spec.py against river_solver_spec / turn_solver_spec) at P = 9 and 16."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import river_solver_spec as RS
import rvr_spec as VS
import solver_lock_spec as LS
import solver_lock_util as LU
import solver_trees_util as U
import turn_solver_spec as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = RS.HOLDINGS
ENTRY_POINTS = ("pk_solve_river_locked_d", "pk_solve_river_locked", "pk_solve_turn_locked_d", "pk_solve_turn_locked")


@pytest.fixture(scope="module")
def lib():
    from pokerl_amd import _lib, build
    build.build_lib()
    return _lib


@pytest.fixture(scope="module")
def S():
    from pokerl_amd import solver
    return solver


def call(lib, S, street, trees, iters=1, m=1, device_form=False, change=None, lock=True, locked=True, same=False, river=(True, True, False), tree_of=True,
         ntrees=None):
    """One well-formed spot -> (return code, error text, the call's name).  lock / locked: pass the arrays; same: `locked` IS `strategy`;
    river: the same three for the turn's river_ pair.  Nothing reaches a device when the call refuses."""
    rows = S._TreeRows(trees, 64 if street == 5 else 128)
    if change:
        change(rows)
    Dt = max(len(t.decision_nodes) for t in trees)
    board, ranges = np.arange(street, dtype=np.uint8)[None].copy(), np.ones((1, 2, H), np.uint16)
    of, status = np.zeros(1, np.uint32), np.zeros(1, np.uint8)
    lk, ld = np.ones((1, Dt), np.uint8), np.ones((1, Dt, 4, H), np.uint16)
    strategy = ld if same else np.zeros((1, Dt, 4, H), np.uint16)
    args = [lib.ptr(lk) if lock else None, lib.ptr(ld) if locked else None]
    outs = [lib.ptr(strategy)]
    if street == 4:
        Dr = max(len(t.river_decision_nodes) for t in trees)
        rk, rd = np.ones((1, Dr), np.uint8), np.ones((1, Dr, 52, 4, H), np.uint16)
        rstrat = rd if river[2] else np.zeros((1, Dr, 52, 4, H), np.uint16)
        args += [lib.ptr(rk) if river[0] else None, lib.ptr(rd) if river[1] else None]
        outs.append(lib.ptr(rstrat))
    name = "pk_solve_%s_locked%s" % ("river" if street == 5 else "turn", "_d" if device_form else "")
    rc = getattr(lib.lib(), name)(0, m, lib.ptr(board), None, lib.ptr(ranges), len(trees) if ntrees is None else ntrees, lib.ptr(rows.n), lib.ptr(rows.kind),
                                  lib.ptr(rows.child), lib.ptr(rows.put), lib.ptr(rows.pot), lib.ptr(of) if tree_of else None, iters, *args, *outs, None, None,
                                  lib.ptr(status), *([None] if device_form else []))
    return rc, lib.lib().pk_last_error(None).decode(), name


def trees_of(S, street):
    return [S.river_tree(100, 50), U.four_action_river_tree()] if street == 5 else [S.turn_tree(30, 20, (1.0,), 1), U.allin_turn_tree()]


def test_header_declares_and_binding_lists_the_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "pokerl_hip.h")).read()
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in lib.SYMBOLS and hasattr(L, name), name
    for words in ("Locked nodes", "br IGNORES the locks", "Neither R nor A is updated at a locked node", "a refused spot's lock data is never read",
                  "iters may be 0 .. PK_RS_MAX_ITERS"):
        assert words in header, words
    assert lib.lib().pk_abi_version() == 6                                    # only symbols are added


@pytest.mark.parametrize("street", [5, 4])
@pytest.mark.parametrize("device_form", [False, True])
def test_every_refusal_has_its_text(lib, S, street, device_form):
    trees = trees_of(S, street)
    kw = dict(device_form=device_form)
    cases = [(dict(same=True), "locked and strategy are the same buffer"), (dict(locked=False), "lock without locked"), (dict(iters=4097), "iters outside 0 .. 4096"),
             (dict(tree_of=False), "tree_of is NULL with ntrees != 1"), (dict(ntrees=0), "ntrees outside 1 .. 65536"), (dict(m=2 ** 31), "m >= 2^31")]
    if street == 4:
        cases += [(dict(river=(True, True, True)), "river_locked and river_strategy are the same buffer"), (dict(river=(True, False, False)), "river_lock without river_locked")]
    for extra, text in cases:
        rc, err, name = call(lib, S, street, trees, **kw, **extra)
        assert rc == lib.PK_E_INVALID_ARG and (err == "%s: %s" % (name, text) or (text == "m >= 2^31" and err.startswith(name + ": ") and text in err)), (extra, rc, err)

    def bad_root(rows):
        rows.kind[1, 0] = 4
    rc, err, name = call(lib, S, street, trees, change=bad_root, **kw)        # a bad tree behind "tree <k>: ", with the existing text
    assert rc == lib.PK_E_INVALID_ARG and err == name + ": tree 1: the root is not a decision node", err


@pytest.mark.parametrize("street", [5, 4])
@pytest.mark.parametrize("device_form", [False, True])
def test_what_is_accepted(lib, S, street, device_form):
    """m = 0: every check passes, nothing runs and no device is needed"""
    trees = trees_of(S, street)
    for extra in (dict(iters=0), dict(iters=4096), dict(lock=False, locked=False, river=(False, False, False)), dict(lock=False),      # locked without lock: not looked at
                  dict(tree_of=False, ntrees=1)):
        rc, err, _ = call(lib, S, street, trees[:1] if "ntrees" in extra else trees, m=0, device_form=device_form, **extra)
        assert rc in (lib.PK_OK, lib.PK_E_NO_DEVICE), (extra, rc, err)
    rows = S._TreeRows(trees_of(S, 5), 64)                                    # the existing calls keep refusing 0 iterations
    rc = lib.lib().pk_solve_river_trees(0, 0, None, None, None, 1, lib.ptr(rows.n), lib.ptr(rows.kind), lib.ptr(rows.child), lib.ptr(rows.put), lib.ptr(rows.pot),
                                        lib.ptr(np.zeros(1, np.uint32)), 0, None, None, None, None)
    assert rc == lib.PK_E_INVALID_ARG and "iters outside 1 .. 4096" in lib.lib().pk_last_error(None).decode()


def test_rows_of(S):
    t = S.river_tree(100, 400)
    r0, r1 = t.rows_of(0), t.rows_of(1)
    assert r0.dtype == bool and r0.shape == (14,) and (r0 ^ r1).all() and r0[0]
    assert r1.tolist() == [int(t.kind[v]) == 1 for v in t.decision_nodes]
    tt = S.turn_tree(100, 400, (1.0,), 1)
    (a0, b0), (a1, b1) = tt.rows_of(0), tt.rows_of(1)
    assert a0.shape == (4,) and b0.shape == (12,) and (a0 ^ a1).all() and (b0 ^ b1).all()
    assert b1.tolist() == [int(tt.kind[v]) == 1 for v in tt.river_decision_nodes]


def test_lock_broadcasts_and_a_solution_serves_as_locked(S):
    m, D = 3, 14
    one = S._lock_rows(np.arange(D) % 2 == 0, m, D, "lock")
    assert one.shape == (m, D) and one.dtype == np.uint8 and one.flags.c_contiguous and (one == (np.arange(D) % 2 == 0)).all()
    assert (S._lock_rows(np.full((m, D), 7), m, D, "lock") == 1).all()      # any nonzero is a flag
    for bad in (np.ones(D + 1), np.ones((m, D)) * 0.5, np.ones((D, m), bool)):
        with pytest.raises(ValueError, match="lock must be"):
            S._lock_rows(bad, m, D, "lock")
    rng = np.random.default_rng(5)
    strategy = rng.integers(0, 32769, (m, D, 4, H)).astype(np.uint16)
    sol = S.RiverSolution(None, None, strategy, None, None, np.zeros(m, np.uint8), None)
    assert S._locked_rows(sol, m, (D, 4, H), "locked", "strategy").tobytes() == strategy.tobytes()
    assert (S._locked_rows(strategy[0], m, (D, 4, H), "locked", "strategy") == strategy[0]).all()      # one spot's rows: every spot the same
    for bad in (strategy[:, :3], strategy.astype(np.float64), strategy.astype(np.int64) + 65536, -strategy.astype(np.int64) - 1):
        with pytest.raises(ValueError, match="locked must"):
            S._locked_rows(bad, m, (D, 4, H), "locked", "strategy")
    ts = S.TurnSolution(None, None, strategy[:, :4], None, None, None, None, None, None)
    with pytest.raises(ValueError, match="has no river_strategy"):
        S._locked_rows(ts, m, (12, 52, 4, H), "river_locked", "river_strategy")
    with pytest.raises(ValueError, match="come together"):
        S._lock_pair(np.ones(D), None, m, D, (4, H), ("lock", "locked"), "strategy")
    with pytest.raises(ValueError, match="come together"):
        S.solve_river_batch(np.zeros((1, 5), np.uint8), np.zeros((1, 2, H), np.uint16), S.river_tree(100, 400), 1, locked=strategy[:1])
    assert S._lock_pair(None, None, m, D, (4, H), ("lock", "locked"), "strategy") == (None, None)
    import pokerl_amd
    assert all(hasattr(pokerl_amd, n) for n in ("evaluate_river", "evaluate_river_batch", "evaluate_turn", "evaluate_turn_batch"))


def test_the_new_kernels_exist_without_scratch(lib):
    """`.private_segment_fixed_size` == 0 and no spilled VGPR, LDS as the kernels they instantiate: the locked kernels are the same bodies"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(lib.LIB_PATH)
    new = {k: d for k, d in ks.items() if k.startswith("k_lock_")}
    assert sorted(new) == ["k_lock_river_solve", "k_lock_turn_solve"], sorted(new)
    assert all(d["private_segment"] == 0 and d["vgpr_spill"] == 0 for d in new.values()), new
    assert new["k_lock_river_solve"]["lds"] == ks["k_trees_river_solve"]["lds"] == ks["k_river_solve"]["lds"]
    assert new["k_lock_turn_solve"]["lds"] == ks["k_trees_turn_solve"]["lds"] == ks["k_turn_solve"]["lds"]
    assert all(new[k]["vgprs"] <= 256 for k in new)                           # two waves per SIMD, as __launch_bounds__(512, 2) asks


# ------------------------------------------------------------------------------------------------ the identities, on the restatement
def river_spot(S, seed, P):
    rng = np.random.default_rng(seed)
    board, _, dead = VS.random_boards(rng, 1, 5, P)
    return [int(c) for c in board[0]], LU.random_ranges(rng, 1)[0], int(dead[0]), rng


def turn_spot(S, seed, P):
    rng = np.random.default_rng(seed)
    board, _, dead = VS.random_boards(rng, 1, 4, P)
    return [int(c) for c in board[0, :4]], LU.random_ranges(rng, 1)[0], int(dead[0]), rng


def same(a, b, keys):
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


RK = ("strategy", "value", "br", "valid")
TK = ("strategy", "river_strategy", "value", "br", "valid")


def test_river_identities_on_the_restatement(S):
    tree = S.river_tree(100, 400)
    board, ranges, dead, rng = river_spot(S, 0x10c3, 16)                      # (the GPU test's spot)
    plain = RS.solve_spot(board, ranges, tree, 64, dead)
    free = RS.solve_spot(board, ranges, tree, 3, dead)
    same(LS.solve_river_spot(board, ranges, tree, 3, None, None, dead), free, RK)                                        # 1
    same(LS.solve_river_spot(board, ranges, tree, 3, np.zeros(14), np.full((14, 4, H), 0xFFFF), dead), free, RK)
    same(LS.solve_river_spot(board, ranges, tree, 0, np.ones(14), plain["strategy"], dead), plain, RK)                   # 2
    lock, gaps = tree.rows_of(1), []                                                                                     # 3
    for iters in (0, 16, 64, 256):
        r = LS.solve_river_spot(board, ranges, tree, iters, lock, plain["strategy"], dead)
        assert (r["br"][0] == plain["br"][0]).all() and (r["strategy"][lock] == plain["strategy"][lock]).all()
        gaps.append(LS.gap(ranges, r["value"], r["br"], 0))
    assert all(a > b for a, b in zip(gaps, gaps[1:])), gaps
    locked = LU.random_weights(rng, (1, 14, 4, H))                                                                         # 4
    flags = tree.rows_of(0).astype(np.uint8)[None]
    a = LS.solve_river_spot(board, ranges, tree, 2, flags[0], locked[0], dead)
    _, poisoned = LU.poison_unread(flags, locked, [tree], [0], a["valid"][None])
    assert (poisoned != locked).mean() > 0.5
    same(LS.solve_river_spot(board, ranges, tree, 2, flags[0], poisoned[0], dead), a, RK)
    same(LS.solve_river_spot(board, ranges, tree, 2, flags[0], (locked[0] >> 1) * 2, dead), LS.solve_river_spot(board, ranges, tree, 2, flags[0], locked[0] >> 1, dead), RK)   # 5


def test_turn_identities_on_the_restatement(S):
    tree = S.turn_tree(100, 400, (1.0,), 1)
    board, ranges, dead, rng = turn_spot(S, 0x10c4, 9)                        # (the GPU test's spot)
    plain = TS.solve_spot(board, ranges, tree, 16, dead)
    free = TS.solve_spot(board, ranges, tree, 2, dead)
    same(LS.solve_turn_spot(board, ranges, tree, 2, dead=dead), free, TK)                                                # 1
    same(LS.solve_turn_spot(board, ranges, tree, 0, np.ones(4), plain["strategy"], np.ones(12), plain["river_strategy"], dead), plain, TK)      # 2
    (lock, rlock), gaps = tree.rows_of(1), []                                                                            # 3
    for iters in (0, 16, 64):
        r = LS.solve_turn_spot(board, ranges, tree, iters, lock, plain["strategy"], rlock, plain["river_strategy"], dead)
        assert (r["br"][0] == plain["br"][0]).all() and (r["strategy"][lock] == plain["strategy"][lock]).all()
        assert (r["river_strategy"][rlock] == plain["river_strategy"][rlock]).all()
        gaps.append(LS.gap(ranges, r["value"], r["br"], 0))
    assert all(a > b for a, b in zip(gaps, gaps[1:])), gaps
    locked, rlocked = LU.random_weights(rng, (1, 4, 4, H)), LU.random_weights(rng, (1, 12, 52, 4, H))                      # 4
    f, rf = (x.astype(np.uint8)[None] for x in tree.rows_of(0))
    a = LS.solve_turn_spot(board, ranges, tree, 2, f[0], locked[0], rf[0], rlocked[0], dead)
    A = np.array([x for y in range(52) for x in range(y)])
    B = np.array([y for y in range(52) for x in range(y)])
    pool = [set(A[a["valid"]].tolist()) | set(B[a["valid"]].tolist())]
    _, p1 = LU.poison_unread(f, locked, [tree], [0], a["valid"][None])
    _, p2 = LU.poison_unread(rf, rlocked, [tree], [0], a["valid"][None], river=True, pool=pool)
    assert (p2 != rlocked).mean() > 0.5
    same(LS.solve_turn_spot(board, ranges, tree, 2, f[0], p1[0], rf[0], p2[0], dead), a, TK)
    same(LS.solve_turn_spot(board, ranges, tree, 2, f[0], (locked[0] >> 1) * 2, rf[0], (rlocked[0] >> 1) * 2, dead),
         LS.solve_turn_spot(board, ranges, tree, 2, f[0], locked[0] >> 1, rf[0], rlocked[0] >> 1, dead), TK)              # 5
