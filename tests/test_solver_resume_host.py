"""Host-side tests of the resuming calls (pk_solve_river_resume / pk_solve_turn_resume: include/pokerl_hip.h "Resuming a solve", DESIGN.md
section 3.17), no GPU: the header and the binding, every refusal text of the host checks (they run before any device is looked at), the
new kernels' code-object figures, and identities (i) and (ii) on the restatement itself (tests/resume_spec.py against tests/resolve_spec.py)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import resolve_spec as RZ
import resume_spec as RM
import river_solver_spec as RS
import rvr_spec as VS
import solver_lock_util as LU
import solver_trees_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = RS.HOLDINGS
ENTRY_POINTS = ("pk_solve_river_resume_d", "pk_solve_river_resume", "pk_solve_turn_resume_d", "pk_solve_turn_resume")
NAMES = {5: ("regret", "average"), 4: ("regret", "average", "river_regret", "river_average")}
TOGETHER = {5: "regret and average come together", 4: "regret, average, river_regret and river_average come together"}
ALONE = {5: "t0 without regret and average", 4: "t0 without regret, average, river_regret and river_average"}
ALIAS = "a state array is another argument of the call"


@pytest.fixture(scope="module")
def lib():
    from pokerl_amd import _lib, build
    build.build_lib()
    return _lib


@pytest.fixture(scope="module")
def S():
    from pokerl_amd import solver
    return solver


def trees_of(S, street):
    return [S.river_tree(100, 50), S.gadget_tree(U.four_action_river_tree(), 1)] if street == 5 else [S.turn_tree(30, 20, (1.0,), 1), U.allin_turn_tree()]


def call(lib, S, street, iters=1, m=1, device_form=False, t0=True, state=None, alias=None):
    """One well-formed spot -> (return code, error text, the call's name).  state: which of the street's state arrays are passed (None:
    all); alias = (a state array's name, another argument's name): the two are ONE buffer.  Nothing reaches a device when the call refuses."""
    trees = trees_of(S, street)
    rows = S._TreeRows(trees, 64 if street == 5 else 128)
    Dt = max(len(t.decision_nodes) for t in trees)
    Dr = max(len(t.river_decision_nodes) for t in trees) if street == 4 else 0
    a = dict(board=np.arange(street, dtype=np.uint8)[None].copy(), ranges=np.ones((1, 2, H), np.uint16), tree_of=np.zeros(1, np.uint32), lock=np.ones((1, Dt), np.uint8),
             locked=np.ones((1, Dt, 4, H), np.uint16), reach=np.ones((1, 2, H), np.uint32), given=np.zeros((1, 2, H), np.int64), at=np.zeros(1, np.uint8),
             at_card=np.zeros(1, np.uint8), t0=np.zeros(1, np.uint32), regret=np.zeros((1, Dt, 4, H), np.int64), average=np.zeros((1, Dt, 4, H), np.int64),
             river_regret=np.zeros((1, max(Dr, 1), 52, 4, H), np.int64), river_average=np.zeros((1, max(Dr, 1), 52, 4, H), np.int64),
             strategy=np.zeros((1, Dt, 4, H), np.uint16), value=np.zeros((1, 2, H), np.int64), br=np.zeros((1, 2, H), np.int64),
             node_reach=np.zeros((1, 2, H), np.uint32), node_value=np.zeros((1, 2, H), np.int64), node_br=np.zeros((1, 2, H), np.int64), status=np.zeros(1, np.uint8))
    if alias:
        a[alias[1]] = a[alias[0]]
    p = lambda k: lib.ptr(a[k])
    st = [p(k) if (state is None or k in state) else None for k in NAMES[street]]
    locks = [p("lock"), p("locked")] + ([None, None] if street == 4 else [])
    news = [p("reach")] + ([p("given")] if street == 5 else []) + [p("at")] + ([p("at_card")] if street == 4 else [])
    outputs = [p("strategy")] + ([None] if street == 4 else []) + [p(k) for k in ("value", "br", "node_reach", "node_value", "node_br", "status")]
    name = "pk_solve_%s_resume%s" % ("river" if street == 5 else "turn", "_d" if device_form else "")
    rc = getattr(lib.lib(), name)(0, m, p("board"), None, p("ranges"), len(trees), lib.ptr(rows.n), lib.ptr(rows.kind), lib.ptr(rows.child), lib.ptr(rows.put),
                                  lib.ptr(rows.pot), p("tree_of"), iters, *locks, *news, p("t0") if t0 else None, *st, *outputs, *([None] if device_form else []))
    return rc, lib.lib().pk_last_error(None).decode(), name


def test_header_declares_and_binding_lists_the_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "pokerl_hip.h")).read()
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in lib.SYMBOLS and hasattr(L, name), name
    for words in ("Resuming a solve", "#define PK_EQ_BAD_ITER 16u", "t = t0[i] + 1 .. t0[i] + iters", "RMAX = 2^58 - 1, AMAX = 2^44 - 1", "RMAX = 2^60 - 1, AMAX = 2^41 - 1",
                  "ITS STATE IS NOT TOUCHED", "With none the call IS the resolve call"):
        assert words in header, words
    assert lib.lib().pk_abi_version() == 6 and lib.EQ_BAD_ITER == 16            # only symbols are added


@pytest.mark.parametrize("street", [5, 4])
@pytest.mark.parametrize("device_form", [False, True])
def test_every_refusal_has_its_text(lib, S, street, device_form):
    names = NAMES[street]
    cases = [(dict(state=names[:1]), TOGETHER[street]), (dict(state=names[1:]), TOGETHER[street]), (dict(state=()), ALONE[street]),
             (dict(alias=("regret", "average")), ALIAS), (dict(alias=("average", "value")), ALIAS), (dict(alias=("regret", "node_br")), ALIAS),
             (dict(iters=4097), "iters outside 0 .. 4096")]
    if street == 4:
        cases += [(dict(state=names[:2]), TOGETHER[4]), (dict(state=names[:3]), TOGETHER[4]), (dict(alias=("river_regret", "river_average")), ALIAS),
                  (dict(alias=("river_average", "regret")), ALIAS)]
    else:
        cases += [(dict(alias=("regret", "given")), ALIAS)]
    for extra, text in cases:
        rc, err, name = call(lib, S, street, device_form=device_form, **extra)
        assert rc == lib.PK_E_INVALID_ARG and err == "%s: %s" % (name, text), (extra, rc, err)
    # without state the call is the resolve call, which speaks under its own name
    rc, err, name = call(lib, S, street, device_form=device_form, t0=False, state=(), iters=4097)
    assert rc == lib.PK_E_INVALID_ARG and err == "%s: iters outside 0 .. 4096" % name.replace("resume", "resolve"), err


@pytest.mark.parametrize("street", [5, 4])
@pytest.mark.parametrize("device_form", [False, True])
def test_what_is_accepted(lib, S, street, device_form):
    """m = 0: every check passes, nothing runs and no device is needed"""
    for extra in (dict(iters=0), dict(t0=False), dict(t0=False, state=()), dict(iters=4096)):
        rc, err, _ = call(lib, S, street, m=0, device_form=device_form, **extra)
        assert rc in (lib.PK_OK, lib.PK_E_NO_DEVICE), (extra, rc, err)


def test_the_new_kernels_exist_without_scratch(lib):
    """`.private_segment_fixed_size` == 0 and no spilled VGPR; LDS as the kernels they instantiate"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(lib.LIB_PATH)
    new = {k: d for k, d in ks.items() if k.startswith("k_resume_")}
    assert sorted(new) == ["k_resume_prep", "k_resume_river_solve", "k_resume_turn_solve"], sorted(new)
    assert all(d["private_segment"] == 0 and d["vgpr_spill"] == 0 for d in new.values()), new
    assert new["k_resume_river_solve"]["lds"] <= 65536 and new["k_resume_river_solve"]["lds"] == ks["k_resolve_river_solve"]["lds"]
    assert new["k_resume_turn_solve"]["lds"] <= 65536 and new["k_resume_turn_solve"]["lds"] == ks["k_resolve_turn_solve"]["lds"]
    assert new["k_resume_prep"]["lds"] == 0
    assert all(new[k]["vgprs"] <= 256 for k in new)                           # two waves per SIMD, as __launch_bounds__(512, 2) asks
    assert not [k for k in ks if k.startswith(("k_river_solve", "k_turn_solve", "k_trees_")) and "resume" in k]


def test_python_takes_and_refuses_state(S):
    tree = S.river_tree(100, 50)
    D = len(tree.decision_nodes)
    assert S.solver_state_bytes(tree, 3) == 2 * 3 * D * 4 * H * 8
    t = S.turn_tree(30, 20, (1.0,), 1)
    assert S.solver_state_bytes([t, U.allin_turn_tree()], 2) == 2 * 2 * (len(t.decision_nodes) + 52 * len(t.river_decision_nodes)) * 4 * H * 8
    z = np.zeros((D, 4, H), np.int64)
    st = S.SolverState(z, z.copy(), 7)
    assert st.nbytes == 2 * z.nbytes and "t=7" in repr(st)
    t0, regret, average = S._state_arrays(st, False, 2, D)
    assert t0.tolist() == [7, 7] and regret.shape == (2, D, 4, H) and regret is not z and S._state_arrays(None, False, 2, D) is None
    assert [a.shape for a in S._state_arrays(None, True, 2, D, 3)[1:]] == [(2, D, 4, H)] * 2 + [(2, 3, 52, 4, H)] * 2
    for bad in ((z, z), (z[:1], z, 0), (z, z, -1), (z.astype(np.float64), z, 0)):
        with pytest.raises(ValueError):
            S._state_arrays(bad, False, 2, D)
    with pytest.raises(ValueError, match="of this solver"):
        S._state_arrays(st, False, 2, D, 3)                                   # a river state handed to the turn solver


# ------------------------------------------------------------------------------------------------ the identities, on the restatement
def same(a, b, keys):
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_river_identities_on_the_restatement(S):
    rng = np.random.default_rng(0x3791)
    board, _, dead = VS.random_boards(rng, 1, 5, 9)
    cards, d = [int(c) for c in board[0]], int(dead[0])
    tree = S.river_tree(100, 50)
    D = len(tree.decision_nodes)
    ranges = LU.random_ranges(rng, 1)[0]
    lock = tree.rows_of(1)
    locked = LU.random_weights(rng, (D, 4, H))
    keys = ("strategy", "value", "br", "node_reach", "node_value", "node_br", "status")
    sentinel = np.full((D + 2, 4, H), 77, np.int64)
    plain = RZ.solve_river_spot(cards, ranges, tree, 5, lock, locked, d, at=1)
    whole = RM.solve_river_spot(cards, ranges, tree, 5, lock, locked, d, at=1, regret=sentinel, average=sentinel)
    same(whole, plain, keys)                                                  # (i)
    assert whole["t"] == 5 and not whole["regret"][D:].any() and not whole["regret"][:D][lock].any() and whole["regret"][:D][~lock].any()
    a = RM.solve_river_spot(cards, ranges, tree, 2, lock, locked, d, at=1, regret=sentinel, average=sentinel)
    b = RM.solve_river_spot(cards, ranges, tree, 3, lock, locked, d, at=1, t0=2, regret=a["regret"], average=a["average"])
    same(b, whole, keys + ("regret", "average"))                              # (ii)
    kept = RM.solve_river_spot(cards, ranges, tree, 3, lock, locked, d, at=1, t0=2, regret=np.where(a["regret"] == 0, 77, a["regret"]), average=a["average"])
    assert (kept["regret"][D:] == 77).all() and (kept["regret"][:D][lock] == 77).all()                  # what is not read survives a continued call
    over = RM.solve_river_spot(cards, ranges, tree, 1, lock, locked, d, t0=4096, regret=sentinel, average=sentinel)
    assert over["status"] == RM.BAD_ITER and (over["regret"] == 77).all() and not over["strategy"].any() and over["t"] == 0
    dup = RM.solve_river_spot(cards[:4] + cards[:1], ranges, tree, 1, lock, locked, d, t0=0, regret=sentinel, average=sentinel)
    assert dup["status"] == RS.DUP_CARD and (dup["regret"] == 77).all()


def test_turn_identities_on_the_restatement(S):
    rng = np.random.default_rng(0x3792)
    board, _, dead = VS.random_boards(rng, 1, 4, 6)
    cards, d = [int(c) for c in board[0, :4]], int(dead[0])
    tree = U.allin_turn_tree()
    ranges = LU.random_ranges(rng, 1)[0]
    rlock, rlocked = np.array([False, True]), LU.random_weights(rng, (2, 52, 4, H))
    keys = ("strategy", "river_strategy", "value", "br", "status")
    kw = dict(river_lock=rlock, river_locked=rlocked, dead=d)
    sent = dict(regret=np.full((3, 4, H), 77, np.int64), average=np.full((3, 4, H), 77, np.int64), river_regret=np.full((2, 52, 4, H), 77, np.int64),
                river_average=np.full((2, 52, 4, H), 77, np.int64))
    plain = RZ.solve_turn_spot(cards, ranges, tree, 4, **kw)
    whole = RM.solve_turn_spot(cards, ranges, tree, 4, **kw, **sent)
    same(whole, plain, keys)                                                  # (i)
    assert not whole["river_regret"][1].any() and whole["river_average"][0].any() and (whole["river_average"][0].reshape(52, -1).any(axis=1)).sum() == 6
    a = RM.solve_turn_spot(cards, ranges, tree, 1, **kw, **sent)
    b = RM.solve_turn_spot(cards, ranges, tree, 3, **kw, t0=1, **{k: a[k] for k in sent})
    same(b, whole, keys + RM.TURN_STATE_KEYS)                                 # (ii)
