"""CPU tests of the river and turn solvers' re-solving calls (no GPU; include/pokerl_hip.h "Re-solving"): the entry
points in the header, the binding and the library; every refusal's text, made before any device is looked at; node kind 6 refused by every
older entry point with its old text; subtree, river_subtree and gadget_tree; the Python wrappers' bounds; the two new kernels in the built
library's code objects; the definition's own identities on the restatement (tests/resolve_spec.py) at P = 9; and what safe re-solving is
for: the opponent's excess over its promised values falls with the iterations of the gadget solve."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import resolve_spec as RZ
import river_solver_spec as RS
import rvr_spec as VS
import solver_lock_spec as LS
import solver_lock_util as LU
import solver_trees_util as U
import turn_solver_spec as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = RS.HOLDINGS
ENTRY_POINTS = ("pk_solve_river_resolve_d", "pk_solve_river_resolve", "pk_solve_turn_resolve_d", "pk_solve_turn_resolve")


@pytest.fixture(scope="module")
def lib():
    from pokerl_amd import _lib, build
    build.build_lib()
    return _lib


@pytest.fixture(scope="module")
def S():
    from pokerl_amd import solver
    return solver


def call(lib, S, street, trees, iters=1, m=1, device_form=False, change=None, ranges=True, reach=True, given=True, at=True, outs=(True, True, True),
         reach_is_out=False, given_is=None, lock_same=False):
    """One well-formed spot -> (return code, error text, the call's name).  The booleans: pass the array or NULL; outs: node_reach,
    node_value, node_br; reach_is_out: `reach` IS node_reach; given_is: the name of the output `given` IS.  Nothing reaches a device
    when the call refuses."""
    rows = S._TreeRows(trees, 64 if street == 5 else 128)
    if change:
        change(rows)
    Dt = max(len(t.decision_nodes) for t in trees)
    board, rg = np.arange(street, dtype=np.uint8)[None].copy(), np.ones((1, 2, H), np.uint16)
    of, status, node = np.zeros(1, np.uint32), np.zeros(1, np.uint8), np.zeros(1, np.uint8)
    lk, ld = np.ones((1, Dt), np.uint8), np.ones((1, Dt, 4, H), np.uint16)
    strategy = ld if lock_same else np.zeros((1, Dt, 4, H), np.uint16)
    o = {k: np.zeros((1, 2, H), np.int64) for k in ("value", "br", "node_value", "node_br")}
    nreach = np.zeros((1, 2, H), np.uint32)
    rc_in = nreach if reach_is_out else np.ones((1, 2, H), np.uint32)
    gv = o[given_is] if given_is else np.zeros((1, 2, H), np.int64)
    p = lib.ptr
    locks = [p(lk), p(ld)] + ([None, None] if street == 4 else [])
    news = [p(rc_in) if reach else None] + ([p(gv) if given else None] if street == 5 else []) + [p(node) if at else None] + ([p(node)] if street == 4 else [])
    outputs = [p(strategy)] + ([None] if street == 4 else []) + [p(o["value"]), p(o["br"]), p(nreach) if outs[0] else None, p(o["node_value"]) if outs[1] else None,
                                                               p(o["node_br"]) if outs[2] else None, p(status)]
    name = "pk_solve_%s_resolve%s" % ("river" if street == 5 else "turn", "_d" if device_form else "")
    rc = getattr(lib.lib(), name)(0, m, p(board), None, p(rg) if ranges else None, len(trees), p(rows.n), p(rows.kind), p(rows.child), p(rows.put), p(rows.pot),
                                  p(of), iters, *locks, *news, *outputs, *([None] if device_form else []))
    return rc, lib.lib().pk_last_error(None).decode(), name


def trees_of(S, street):
    if street == 5:
        return [S.river_tree(100, 50), S.gadget_tree(U.four_action_river_tree(), 1)]
    return [S.turn_tree(30, 20, (1.0,), 1), U.allin_turn_tree()]


def test_header_declares_and_binding_lists_the_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "pokerl_hip.h")).read()
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in lib.SYMBOLS and hasattr(L, name), name
    for words in ("Re-solving", "ROOT REACHES", "NODE OUTPUTS", "GIVEN TERMINAL", "ROOT PUT", "min(reach[i][p][h], LIM)", "clamp(given[i][p][h], +-(2^45 - 1))",
                  "`at` is NULL exactly when all three node outputs are", "at_card is not read for a"):
        assert words in header, words
    assert lib.lib().pk_abi_version() == 6                                    # only symbols are added


@pytest.mark.parametrize("street", [5, 4])
@pytest.mark.parametrize("device_form", [False, True])
def test_every_refusal_has_its_text(lib, S, street, device_form):
    trees = trees_of(S, street)
    kw = dict(device_form=device_form)
    both = "at comes with node_reach, node_value or node_br, and only with one of them"
    cases = [(dict(at=False), both), (dict(outs=(False, False, False)), both), (dict(reach_is_out=True), "reach and node_reach are the same buffer"),
             (dict(lock_same=True), "locked and strategy are the same buffer"), (dict(iters=4097), "iters outside 0 .. 4096"),
             (dict(ranges=False, reach=False), "NULL where a pointer is required (board, ranges, n, kind, child, put, pot, tree_of, status)"),
             (dict(m=2 ** 31), "m >= 2^31")]
    if street == 5:
        cases += [(dict(given=False), "a tree has a given node and given is NULL")]
        cases += [(dict(given_is=k), "given and an output are the same buffer") for k in ("value", "br", "node_value", "node_br")]
    for extra, text in cases:
        rc, err, name = call(lib, S, street, trees, **kw, **extra)
        assert rc == lib.PK_E_INVALID_ARG and (err == "%s: %s" % (name, text) or (text == "m >= 2^31" and err.startswith(name + ": ") and text in err)), (extra, rc, err)

    def kind_at(k, v, value):
        def change(rows):
            rows.kind[k, v] = value
        return change
    leaf = next(v for v in range(trees[0].n) if trees[0].kind[v] > 1 and trees[0].kind[v] != 5)
    if street == 5:
        tree_cases = [(kind_at(1, 3, 6), "tree 1: more than one given node"), (kind_at(0, leaf, 7), "tree 0: a node kind outside 0 .. 4 and not 6"),
                      (kind_at(0, leaf, 5), "tree 0: a node kind outside 0 .. 4 and not 6"), (kind_at(1, 0, 6), "tree 1: the root is not a decision node")]
    else:
        tree_cases = [(kind_at(0, leaf, 6), "tree 0: a node kind outside 0 .. 5")]              # a given node in the turn solver is out of scope
    for change, text in tree_cases:
        rc, err, name = call(lib, S, street, trees, change=change, **kw)
        assert rc == lib.PK_E_INVALID_ARG and err == "%s: %s" % (name, text), (text, err)


@pytest.mark.parametrize("street", [5, 4])
@pytest.mark.parametrize("device_form", [False, True])
def test_what_is_accepted(lib, S, street, device_form):
    """m = 0: every check passes, nothing runs and no device is needed"""
    trees = trees_of(S, street)
    cases = [dict(iters=0), dict(ranges=False), dict(reach=False), dict(at=False, outs=(False, False, False)), dict(outs=(False, True, False))]
    if street == 5:
        cases.append(dict(given=False, change=lambda rows: rows.kind.__setitem__((1, 1), 2)))        # no given node left: given may be NULL
    for extra in cases:
        rc, err, _ = call(lib, S, street, trees, m=0, device_form=device_form, **extra)
        assert rc in (lib.PK_OK, lib.PK_E_NO_DEVICE), (extra, rc, err)


def test_kind_6_is_refused_by_the_older_entry_points_with_their_text(lib, S):
    g = S.gadget_tree(S.river_tree(100, 50), 1)
    rows, p, L = S._TreeRows([g], 64), lib.ptr, lib.lib()
    of = np.zeros(1, np.uint32)
    one = (g.n, p(g.kind), p(g.child), p(g.put), g.pot)
    calls = {"pk_solve_river": lambda: L.pk_solve_river(0, 0, None, None, None, *one, 1, None, None, None, None),
             "pk_solve_river_d": lambda: L.pk_solve_river_d(0, 0, None, None, None, *one, 1, None, None, None, None, None),
             "pk_solve_river_trees": lambda: L.pk_solve_river_trees(0, 0, None, None, None, *rows.args(), p(of), 1, None, None, None, None),
             "pk_solve_river_trees_d": lambda: L.pk_solve_river_trees_d(0, 0, None, None, None, *rows.args(), p(of), 1, None, None, None, None, None),
             "pk_solve_river_locked": lambda: L.pk_solve_river_locked(0, 0, None, None, None, *rows.args(), p(of), 1, None, None, None, None, None, None),
             "pk_solve_river_locked_d": lambda: L.pk_solve_river_locked_d(0, 0, None, None, None, *rows.args(), p(of), 1, None, None, None, None, None, None, None)}
    for name, f in calls.items():
        assert f() == lib.PK_E_INVALID_ARG, name
        err = L.pk_last_error(None).decode()
        assert err == name + (": tree 0" if "trees" in name or "locked" in name else "") + ": a node kind outside 0 .. 4", err
    with pytest.raises(Exception, match="a node kind outside 0 .. 4"):          # ... and through Python, where nothing new is asked for
        S.solve_river_batch(np.zeros((0, 5), np.uint8), np.zeros((0, 2, H), np.uint16), g, 1)


def test_subtree_river_subtree_and_gadget_tree(S):
    t = S.river_tree(100, 400)
    for node in t.decision_nodes:
        sub, rows = t.subtree(node)
        keep = [node]
        for v in keep:
            keep += [int(c) for c in t.child[v] if c != S.NO_CHILD]
        keep.sort()
        assert sub.n == len(keep) and sub.pot == t.pot and (sub.kind == t.kind[keep]).all() and (sub.put == t.put[keep]).all()
        assert [keep[c] for c in sub.child[0] if c != S.NO_CHILD] == [int(c) for c in t.child[node] if c != S.NO_CHILD]
        assert rows.tolist() == [t.decision_nodes.index(v) for v in keep if t.kind[v] <= 1] and len(rows) == len(sub.decision_nodes)
        assert all(c == S.NO_CHILD or v < c < sub.n for v in range(sub.n) for c in sub.child[v])
    whole, rows = t.subtree(0)
    assert (whole.kind == t.kind).all() and (whole.child == t.child).all() and rows.tolist() == list(range(14))
    bet = int(t.child[0][1])                                                  # after a bet: the root's put is not 0, and survives the round trip
    sub, _ = t.subtree(bet)
    assert sub.put[0].tolist() == t.put[bet].tolist() and sub.put[0].max() > 0 and sub.label(1).startswith("1:")
    again, rows = sub.subtree(0)
    assert (again.put == sub.put).all() and again.pot == 100 and rows.tolist() == list(range(len(sub.decision_nodes)))
    with pytest.raises(ValueError, match="not a decision node"):
        t.subtree(next(v for v in range(t.n) if t.kind[v] > 1))
    g = S.gadget_tree(sub, 1)
    assert g.n == sub.n + 2 and g.kind[:2].tolist() == [1, S.KIND_GIVEN] and g.child[0].tolist() == [1, 2, 255, 255] and (g.child[1] == 255).all()
    assert (g.kind[2:] == sub.kind).all() and (g.put[2:] == sub.put).all() and g.put[0].tolist() == sub.put[0].tolist() and g.pot == sub.pot
    assert (g.child[2:][sub.child != 255] == sub.child[sub.child != 255] + 2).all() and (g.child[2:][sub.child == 255] == 255).all()
    assert g.decision_nodes[0] == 0 and g.decision_nodes[1:] == [v + 2 for v in sub.decision_nodes] and g.label(1) == "1:terminate"
    with pytest.raises(ValueError, match="more than 64 nodes"):
        S.gadget_tree(S.RiverTree(np.r_[np.zeros(1), np.full(62, 4)], np.full((63, 4), 255), np.zeros((63, 2)), 1), 0)      # 63 + 2 nodes
    with pytest.raises(ValueError, match="opponent must be 0 or 1"):
        S.gadget_tree(sub, 2)
    tt = S.turn_tree(100, 400, (1.0,), 1)
    d = tt.decision_nodes[1]
    ts, rows, rrows = tt.subtree(d)
    assert isinstance(ts, S.TurnTree) and ts.pot == tt.pot and ts.put[0].tolist() == tt.put[d].tolist()
    assert len(rows) == len(ts.decision_nodes) and len(rrows) == len(ts.river_decision_nodes) and rows[0] == 1
    assert [int(tt.kind[tt.river_decision_nodes[r]]) for r in rrows] == [int(ts.kind[v]) for v in ts.river_decision_nodes]
    with pytest.raises(ValueError, match="not a turn-level decision node"):
        tt.subtree(tt.river_decision_nodes[0])
    r = tt.river_decision_nodes[3]
    rs, rows = tt.river_subtree(r)
    assert type(rs) is S.RiverTree and rs.pot == tt.pot and rs.put[0].tolist() == tt.put[r].tolist() and rows[0] == 3 and len(rows) == len(rs.decision_nodes)
    with pytest.raises(ValueError, match="not a river-level decision node"):
        tt.river_subtree(0)
    import pokerl_amd
    assert all(hasattr(pokerl_amd, n) for n in ("gadget_tree", "resolve_river", "KIND_GIVEN"))


def test_the_python_wrappers_refuse_what_the_device_forms_clamp(S):
    t = S.river_tree(100, 50)
    board, reach = np.zeros((1, 5), np.uint8), np.zeros((1, 2, H), np.int64)
    reach[0, 1, 7] = S.REACH_MAX + 1
    with pytest.raises(ValueError, match="reach must lie in 0 .. 1048575"):
        S.solve_river_batch(board, None, t, 1, reach=reach)
    given = np.zeros((1, 2, H), np.int64)
    given[0, 0, 3] = -S.GIVEN_MAX - 1
    with pytest.raises(ValueError, match="given must lie within"):
        S.solve_river_batch(board, None, S.gadget_tree(t, 0), 1, reach=np.zeros((1, 2, H), np.uint32), given=given)
    reach[0, 1, 7] = S.TURN_REACH_MAX + 1
    with pytest.raises(ValueError, match="reach must lie in 0 .. 131071"):
        S.solve_turn_batch(board[:, :4], None, S.turn_tree(30, 20, (1.0,), 1), 1, reach=reach)
    with pytest.raises(ValueError, match="ranges or reach"):
        S.solve_river_batch(board, None, t, 1)
    with pytest.raises(ValueError, match="at must"):
        S.solve_river_batch(board, np.zeros((1, 2, H), np.uint16), t, 1, at=[0, 1])
    sol = S.RiverSolution(t, np.ones((2, H), np.uint16), None, np.ones((2, H), np.int64), None, np.uint8(0), np.ones(H, bool))
    assert sol.node_reach is None and sol.node_value is None and sol.node_br is None and sol.reach is None
    same = S.RiverSolution(t, None, None, np.ones((2, H), np.int64), None, np.uint8(0), np.ones(H, bool), reach=np.full((2, H), 16, np.uint32))
    assert sol.ev == same.ev                                                  # a reach of 16 per unit of weight: the same chips


def test_the_new_kernels_exist_without_scratch(lib):
    """`.private_segment_fixed_size` == 0 and no spilled VGPR; LDS within the kernels they instantiate (59 728 / 60 944 bytes)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(lib.LIB_PATH)
    new = {k: d for k, d in ks.items() if k.startswith("k_resolve_")}
    assert sorted(new) == ["k_resolve_prep", "k_resolve_river_solve", "k_resolve_turn_solve"], sorted(new)
    assert all(d["private_segment"] == 0 and d["vgpr_spill"] == 0 for d in new.values()), new
    assert new["k_resolve_river_solve"]["lds"] <= 59728 and new["k_resolve_river_solve"]["lds"] == ks["k_lock_river_solve"]["lds"]
    assert new["k_resolve_turn_solve"]["lds"] <= 60944 and new["k_resolve_turn_solve"]["lds"] == ks["k_lock_turn_solve"]["lds"]
    assert new["k_resolve_prep"]["lds"] == 0
    assert all(new[k]["vgprs"] <= 256 for k in new)                           # two waves per SIMD, as __launch_bounds__(512, 2) asks


# ------------------------------------------------------------------------------------------------ the identities, on the restatement
def river_spot(seed, P):
    rng = np.random.default_rng(seed)
    board, _, dead = VS.random_boards(rng, 1, 5, P)
    return [int(c) for c in board[0]], LU.random_ranges(rng, 1)[0], int(dead[0]), rng


def turn_spot(seed, P):
    rng = np.random.default_rng(seed)
    board, _, dead = VS.random_boards(rng, 1, 4, P)
    return [int(c) for c in board[0, :4]], LU.random_ranges(rng, 1)[0], int(dead[0]), rng


def same(a, b, keys):
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_river_identities_on_the_restatement(S):
    tree = S.river_tree(100, 400)
    board, ranges, dead, _ = river_spot(0x3161, 9)
    lock = LS.solve_river_spot(board, ranges, tree, 3, None, None, dead)
    a = RZ.solve_river_spot(board, None, tree, 3, dead=dead, reach=ranges.astype(np.uint32) << 4, at=0)
    same(a, lock, ("strategy", "value", "br", "valid"))                        # reach = ranges << 4 is the locked call
    assert (a["node_value"] == a["value"]).all() and (a["node_br"] == a["br"]).all()                   # at = root
    assert (a["node_reach"] == (ranges.astype(np.uint32) << 4) * a["valid"]).all()
    for node in tree.decision_nodes[1:4] + [tree.n - 1]:                      # subtree consistency, the last node a terminal
        x = RZ.solve_river_spot(board, ranges, tree, 3, dead=dead, at=node)
        if tree.kind[node] > 1:
            assert (x["node_br"] == x["node_value"]).all()
            continue
        sub, rows = tree.subtree(node)
        y = RZ.solve_river_spot(board, None, sub, 0, np.ones(len(rows)), x["strategy"][rows], dead, reach=x["node_reach"], at=0)
        assert (y["value"] == x["node_value"]).all() and (y["br"] == x["node_br"]).all() and (y["node_reach"] == x["node_reach"]).all(), node
    sub, rows = tree.subtree(int(tree.child[0][1]))                           # the gadget: follow is the subtree alone, terminate the given values
    g = S.gadget_tree(sub, 1)
    reach = RZ.solve_river_spot(board, ranges, tree, 3, dead=dead, at=int(tree.child[0][1]))["node_reach"]
    given = np.random.default_rng(5).integers(-(1 << 46), 1 << 46, (2, H))
    given[0] = 0                                                              # (the hero is promised nothing: its value at the gadget's root is the subtree's)
    row0 = np.zeros((len(g.decision_nodes), 4, H), np.int64)
    flags = np.zeros(len(g.decision_nodes))
    flags[0], row0[0, 1] = 1, 1
    follow = RZ.solve_river_spot(board, None, g, 16, flags, row0, dead, reach=reach, given=given)
    alone = RZ.solve_river_spot(board, None, sub, 16, dead=dead, reach=reach)
    assert (follow["strategy"][1:] == alone["strategy"]).all() and (follow["value"] == alone["value"]).all() and (follow["br"][0] == alone["br"][0]).all()
    assert (follow["br"][1] == np.maximum(np.clip(given[1], -RZ.GIVEN_LIM, RZ.GIVEN_LIM), alone["br"][1]) * alone["valid"]).all()      # br ignores the lock
    row0[0, 0], row0[0, 1] = 1, 0
    stop = RZ.solve_river_spot(board, None, g, 2, flags, row0, dead, reach=reach, given=given)
    assert (stop["value"][1] == np.clip(given[1], -RZ.GIVEN_LIM, RZ.GIVEN_LIM) * stop["valid"]).all()
    inside = RZ.solve_river_spot(board, None, g, 2, flags, row0, dead, reach=reach, given=given, at=2)
    assert not inside["node_value"][0].any() and not inside["node_reach"][1].any()     # the opponent never follows: the hero's values in the subtree are 0


def test_turn_identities_on_the_restatement(S):
    tree = S.turn_tree(30, 20, (1.0,), 1)
    board, ranges, dead, _ = turn_spot(0x3162, 9)
    lock = LS.solve_turn_spot(board, ranges, tree, 2, dead=dead)
    a = RZ.solve_turn_spot(board, None, tree, 2, dead=dead, reach=ranges.astype(np.uint32) << 1, at=0)
    same(a, lock, ("strategy", "river_strategy", "value", "br", "valid"))
    assert (a["node_value"] == a["value"]).all() and (a["node_br"] == a["br"]).all() and (a["node_reach"] == (ranges.astype(np.uint32) << 1) * a["valid"]).all()
    chance = next(v for v in range(tree.n) if tree.kind[v] == 5)                # the chance-sum identity over all pool cards
    child = int(tree.child[chance][0])
    at_chance = RZ.solve_turn_spot(board, ranges, tree, 2, dead=dead, at=chance)
    _, gone = TS.check_spot(board, dead)
    total = {k: np.zeros((2, H), np.int64) for k in ("node_value", "node_br")}
    for k in range(52):
        if k in gone:
            continue
        x = RZ.solve_turn_spot(board, ranges, tree, 2, dead=dead, at=child, at_card=int(VS.CANON[k]))
        assert x["status"] == 0 and not x["node_value"][:, (VS.PAIR_A == k) | (VS.PAIR_B == k)].any()
        for key in total:
            total[key] += x[key]
    assert (total["node_value"] == at_chance["node_value"]).all() and (total["node_br"] == at_chance["node_br"]).all() and at_chance["node_value"].any()
    bad = RZ.solve_turn_spot(board, ranges, tree, 2, dead=dead, at=child, at_card=int(board[0]))
    assert bad["status"] == RZ.BAD_CARD and not bad["value"].any()
    assert RZ.solve_turn_spot(board, ranges, tree, 2, dead=dead, at=tree.n)["status"] == RZ.BAD_TREE
    assert RZ.solve_turn_spot(board, ranges, tree, 2, dead=dead, at=chance, at_card=0xFF)["status"] == 0          # not read at a turn-level node


# ------------------------------------------------------------------------------------------------ safe re-solving does what it is for
SAFE_SEED = 0x5afe0


def safe_resolving_figures(S, seed=SAFE_SEED):
    """One seeded P = 12 river spot, the default tree, the node after player 0's first bet: the opponent (player 1, to act there) is
    promised node_br[1] of a 256-iteration solve; the hero's strategy is re-solved through the gadget at 16 / 64 / 256 iterations and
    without it (unsafe, 256 iterations); each is judged by resolve_spec.excess -> (the three excesses, the unsafe one), in chips."""
    tree = S.river_tree(100, 400)
    board, ranges, dead, _ = river_spot(seed, 12)
    node = int(tree.child[0][1])
    first = RZ.solve_river_spot(board, ranges, tree, 256, dead=dead, at=node)
    sub, _ = tree.subtree(node)
    opponent = 1
    promised, reach = first["node_br"][opponent], first["node_reach"].astype(np.int64)
    flat = reach.copy()
    flat[opponent] = int(reach[opponent].max()) * first["valid"]              # (resolve_river's convention)
    given = np.zeros((2, H), np.int64)
    given[opponent] = promised
    g = S.gadget_tree(sub, opponent)
    out = []
    for iters in (16, 64, 256):
        r = RZ.solve_river_spot(board, None, g, iters, dead=dead, reach=flat, given=given)
        out.append(RZ.excess(board, sub, reach, r["strategy"][1:], opponent, promised, dead))
    unsafe = RZ.solve_river_spot(board, None, sub, 256, dead=dead, reach=reach)
    return out, RZ.excess(board, sub, reach, unsafe["strategy"], opponent, promised, dead)


def test_safe_resolving_lowers_the_opponents_excess(S):
    safe, unsafe = safe_resolving_figures(S)
    print("the opponent's excess over its promised values, chips: safe at 16 / 64 / 256 iterations %r, unsafe at 256 %r" % (safe, unsafe))
    assert safe[0] > safe[1] > safe[2] >= 0.0, safe
