"""GPU tests of the solvers' arithmetic where a comparison with a numpy int64 restatement alone cannot see an error (include/pokerl_hip.h
"River solver": STRATEGY FROM NON-NEGATIVE INTEGERS, and the BOUNDS paragraphs of "River solver", "Turn solver" and "Resuming a solve").
Exact throughout.
(a) THE RULE THROUGH `average`: a resuming call with t0 > 0 and iters = 0 returns the rule applied to the caller's accumulators, so the
    operand tables of tests/solver_rule_cases.py -- every shift, every power-of-two boundary of the largest entry, entries the shift erases,
    the divisor 2^33 - 4, quotients on, just under and just over an integer, values beyond both clamps -- go through rs_sigma / rs_div on
    the device, one tuple per (row, holding) and on the turn per (row, river card, holding), and must give rule_exact (ten lines of Python
    integers) of the clamped tuple.
(b) THE RULE THROUGH `regret`: iters = 1 with a root reach of exactly ONE returns (t0 + 1) x rule(clamp(regret)) in the root row's average.
(c) THE BOUNDS CORNER: pot + put = 8191, every weight 65535, the state at RMAX / AMAX, t0 = 4093 and 3 iterations, against
    tests/resume_spec.py live (river P = 47, turn P = 12) and at the turn's P = 48 against tests/golden/solver_arith/turn_corner_p48.npz,
    which a Python-integer witness agreed with before it was written (tests/test_solver_arithmetic_host.py holds the same witness against
    the restatement at the river corner).
(d) FULL DEPTH: 4096 iterations in one call against the plain restatements, and the chains that end at t = 4096.
In (a) - (c) the whole output and the whole state also equal tests/resume_spec.py."""
import hashlib
import os

import numpy as np
import pytest

import river_solver_spec as RS
import solver_resolve_util as RU
import solver_resume_util as MU
import solver_rule_cases as RC
import solver_trees_util as U
import turn_solver_spec as TS

pytestmark = pytest.mark.gpu

H = RS.HOLDINGS
RIVER_OUT = ("strategy", "value", "br", "status", "regret", "average")
TURN_OUT = ("strategy", "river_strategy", "value", "br", "status", "regret", "average", "river_regret", "river_average")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solver_arith", "turn_corner_p48.npz")


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


@pytest.fixture(scope="module")
def S():
    from pokerl_amd import solver
    return solver


def device(S, street, call, iters=None, t0=None, state=None):
    """the resuming call on the device with the arguments of solver_rule_cases.rule_call / corner_call"""
    iters = call["iters"] if iters is None else iters
    t0 = call["t0"] if t0 is None else t0
    state = call["state"] if state is None else state
    if street == 5:
        return MU.river_call(S, call["board"], call["dead"], call["trees"], call["tree_of"], iters, ranges=call["ranges"], t0=t0, regret=state[0], average=state[1])
    return MU.turn_call(S, call["board"], call["dead"], call["trees"], call["tree_of"], iters, ranges=call["ranges"], t0=t0, state=state)


def same(got, want, where, keys):
    RU.assert_equal(got, want, where, keys)
    assert not np.asarray(want["status"]).any(), where


# ------------------------------------------------------------------------------------------------ (a) the rule through `average`
def test_a_river_rule_through_average(PK, S):
    """P = 47; the forced tree (1 action), the default tree (2, 3 and 4 actions) and the four-action tree in one call"""
    trees = [U.forced_river_tree(), PK.river_tree(100, 400), U.four_action_river_tree()]
    call = RC.rule_call(5, trees, "average", 7, 47)
    assert RC.covered(call["where"], {n: RC.table("river_A", n) for n in (1, 2, 3, 4)})
    got = device(S, 5, call)
    assert RC.rule_wanted(call, got) == []
    same(got, RC.spec_of(5, call), "iters = 0 from the tables", RIVER_OUT)


@pytest.mark.parametrize("which", ["built", "four-action"])
def test_a_turn_rule_through_average_at_both_levels(PK, S, which):
    """P = 14 (the live restatement: under a second); turn_tree(100, 400, (1.0,), 1) and the hand-made tree with 1 .. 4 actions at both levels"""
    tree = PK.turn_tree(100, 400, (1.0,), 1) if which == "built" else RC.four_action_turn_tree()
    call = RC.rule_call(4, [tree], "average", 9, 14)
    nacts = {tree.num_actions(v) for v in tree.decision_nodes + tree.river_decision_nodes}
    assert RC.covered(call["where"] + call["river_where"], {n: RC.table("turn_A", n) for n in nacts}) and nacts == ({2} if which == "built" else {1, 2, 3, 4})
    assert RC.covered(call["river_where"], {n: RC.table("turn_A", n) for n in {tree.num_actions(v) for v in tree.river_decision_nodes}})
    got = device(S, 4, call)
    assert RC.rule_wanted(call, got) == []
    same(got, RC.spec_of(4, call), "iters = 0 from the tables", TURN_OUT)


# ------------------------------------------------------------------------------------------------ (b) the rule through `regret`
@pytest.mark.parametrize("t0", [1, 4095])
def test_b_river_rule_through_regret(PK, S, t0):
    """every weight 2048: the root reach is exactly ONE, so the root row's average is (t0 + 1) x the rule of the clamped regrets; roots of 1,
    2, 3 and 4 actions, each taking its whole table"""
    trees = [U.forced_river_tree(), RC.nine_node_tree(), PK.river_tree(100, 400), U.four_action_river_tree()]
    assert [t.num_actions(0) for t in trees] == [1, 2, 3, 4]
    call = RC.rule_call(5, trees, "regret", t0, 47)
    roots = [{k: v for k, v in put.items() if k[0] == (0,)} for put in call["where"]]
    assert RC.covered(roots, {n: RC.table("river_R", n) for n in (1, 2, 3, 4)})
    got = device(S, 5, call)
    assert RC.rule_wanted(call, got) == []
    same(got, RC.spec_of(5, call), "one iteration from the tables", RIVER_OUT)


@pytest.mark.parametrize("t0", [1, 4095])
def test_b_turn_rule_through_regret(PK, S, t0):
    """every weight 16384 (<< 1: ONE); a two-action root (turn_tree(30, 20, (1.0,), 1), whose four river-level rows keep the fifteen spots the
    root row needs small) and the four-action root of the hand-made tree, one call each"""
    for tree, n in ((PK.turn_tree(30, 20, (1.0,), 1), 2), (RC.four_action_turn_tree(), 4)):
        assert tree.num_actions(0) == n
        call = RC.rule_call(4, [tree], "regret", t0, 14)
        roots = [{k: v for k, v in put.items() if k[0] == (0,)} for put in call["where"]]
        assert RC.covered(roots, {n: RC.table("turn_R", n)})
        got = device(S, 4, call)
        assert RC.rule_wanted(call, got) == []
        same(got, RC.spec_of(4, call), "one iteration from the tables", TURN_OUT)


# ------------------------------------------------------------------------------------------------ (c) the bounds corner
@pytest.mark.parametrize("variant", ["top", "swing", "mix"])
def test_c_river_bounds_corner(S, variant):
    call = RC.corner_call(5, 47, variant)
    got, want = device(S, 5, call), RC.spec_of(5, call)
    same(got, want, "the river corner, " + variant, RIVER_OUT)
    read = MU.river_read_mask(call["board"], call["dead"], call["trees"], None)
    assert want["valid"].sum() == 1081 and (got["regret"][read] >= 0).all() and got["regret"][read].max() >= RC.lim_of("river_R") and got["average"][read].max() > RC.lim_of("river_A")


@pytest.mark.parametrize("variant", ["top", "swing", "mix"])
def test_c_turn_bounds_corner_live(S, variant):
    call = RC.corner_call(4, 12, variant)
    got, want = device(S, 4, call), RC.spec_of(4, call)
    same(got, want, "the turn corner at P = 12, " + variant, TURN_OUT)
    assert got["river_regret"].max() >= RC.lim_of("turn_R") and got["value"].any()


def test_c_turn_bounds_corner_full_pool_fixture(S):
    """P = 48: the restatement's result, which the Python-integer witness equalled (tests/golden/solver_arith/make.py)"""
    fx = np.load(GOLDEN)
    call = RC.corner_call(4, 48, "top")
    assert fx["board"].tolist() == call["board"][0].tolist() and int(fx["dead"]) == int(call["dead"][0]) and int(fx["t0"]) == 4093 and int(fx["iters"]) == 3
    assert fx["tree_args"].tolist() == [2731, 5460, 1] and int(fx["weight"]) == 65535
    got = device(S, 4, call)
    assert got["status"].tolist() == [int(fx["status"])] == [0]
    for k in ("strategy", "value", "br"):
        assert got[k].dtype == fx[k].dtype and (got[k][0] == fx[k]).all(), (k, np.argwhere(got[k][0] != fx[k])[:4].tolist())
    for k in ("river_strategy", "regret", "average", "river_regret", "river_average"):
        assert hashlib.sha256(np.ascontiguousarray(got[k][0]).tobytes()).hexdigest() == str(fx["sha256_" + k]), k


# ------------------------------------------------------------------------------------------------ (d) full depth
def chain(S, street, call, splits):
    m = len(call["board"])
    state = MU.sentinel_state(m, len(call["trees"][0].decision_nodes)) if street == 5 else \
        MU.turn_sentinel_state(m, len(call["trees"][0].decision_nodes), len(call["trees"][0].river_decision_nodes))
    done, r = 0, None
    for it in splits:
        r = device(S, street, call, it, np.full(m, done, np.uint32), state)
        state, done = tuple(r[k] for k in (RIVER_OUT[-2:] if street == 5 else TURN_OUT[-4:])), done + it
    return r


def test_d_river_full_depth(S):
    """P = 6, pot + put = 8191, every weight 65535, 4096 iterations in one call against river_solver_spec (2.4 s live); 4095 + 1 and
    2048 + 2048 leave the same bytes, the state included"""
    board, dead, _, _ = RC.one_spot(5, 6, 0x51AC)
    call = dict(board=board[None], dead=np.array([dead], np.uint64), trees=[RC.nine_node_tree()], tree_of=None, ranges=np.full((1, 2, H), 65535, np.uint16))
    whole = chain(S, 5, call, (4096,))
    want = RS.solve_batch(call["board"], call["ranges"], call["trees"][0], 4096, call["dead"])
    RU.assert_equal(whole, want, "4096 iterations in one call", ("strategy", "value", "br", "status"))
    assert want["status"].tolist() == [0] and want["valid"].sum() == 15 and whole["regret"].any() and whole["average"].max() > 1 << 36
    for splits in ((4095, 1), (2048, 2048)):
        RU.assert_equal(chain(S, 5, call, splits), whole, repr(splits), RIVER_OUT)


def smallest_turn_tree():
    """seven nodes, one river-level decision with a reply: a forced check, the river card, check or bet 4095 into 4096, fold or call"""
    P0, P1, F1, SD, CH = 0, 1, 3, 4, 5
    return RC.tree_from((P0, (0, 0), [(CH, (0, 0), [(P0, (0, 0), [(SD, (0, 0), []), (P1, (4095, 0), [(F1, (4095, 0), []), (SD, (4095, 4095), [])])])])]), 4096, True)


def test_d_turn_full_depth(S):
    """P = 5, the smallest tree with a river-level decision, every weight 65535: 4096 iterations in one call against turn_solver_spec.  The
    live restatement takes 7.5 s for the 4096 iterations on the CPU (0.47 s per 256), so the full depth is what runs; 4095 + 1 and
    2048 + 2048 end at t = 4096 with the same bytes, the state of both levels included"""
    board, dead, _, _ = RC.one_spot(4, 5, 0x51AD)
    call = dict(board=board[None], dead=np.array([dead], np.uint64), trees=[smallest_turn_tree()], tree_of=None, ranges=np.full((1, 2, H), 65535, np.uint16))
    whole = chain(S, 4, call, (4096,))
    want = TS.solve_batch(call["board"], call["ranges"], call["trees"][0], 4096, call["dead"])
    RU.assert_equal(whole, want, "4096 iterations in one call", ("strategy", "river_strategy", "value", "br", "status"))
    assert want["status"].tolist() == [0] and want["P"].tolist() == [5] and whole["river_regret"].any() and whole["river_average"].max() > 1 << 33
    for splits in ((4095, 1), (2048, 2048)):
        RU.assert_equal(chain(S, 4, call, splits), whole, repr(splits), TURN_OUT)
