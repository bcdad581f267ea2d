"""The solvers' arithmetic without a GPU (include/pokerl_hip.h "River solver" / "Turn solver" / "Resuming a solve": STRATEGY FROM NON-NEGATIVE
INTEGERS and the BOUNDS paragraphs).  Every other test of the solvers compares with a numpy int64 restatement, which wraps where a kernel
wraps; here (i) the operand tables of tests/solver_rule_cases.py meet the conditions they were built for and the restatement's rule
equals the ten-line Python-integer rule on every tuple of them, and (ii) a Python-integer walk (tests/solver_witness.py), which cannot
wrap, equals tests/resume_spec.py in every output and state entry at the bounds corner -- the largest pot, every weight 65535, the state at
the clamps, t0 = 4093 and three iterations to t = 4096 -- and every quantity the header bounds stays below the figure the header states
for it.  The figures are printed (pytest -s) and stand in DESIGN.md sections 3.12, 3.13 and 3.17."""
import os

import numpy as np
import pytest

import river_solver_spec as RS
import solver_rule_cases as RC
import solver_witness as SW

KEYS = {5: ("strategy", "value", "br", "regret", "average"),
        4: ("strategy", "river_strategy", "value", "br", "regret", "average", "river_regret", "river_average")}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solver_arith", "turn_corner_p48.npz")


@pytest.mark.parametrize("nact", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", RC.KINDS)
def test_the_tables_hold_what_they_were_built_for(kind, nact):
    """every power-of-two boundary of the largest entry from 2^30 to the clamp (so every shift), the companions, the entries the shift
    erases, S = nact (2^31 - 1), the uniform row, remainders 0, 1 and S - 1 at three shifts, values beyond both clamps"""
    n = RC.check_table(kind, nact)
    assert n == len(RC.table(kind, nact)) and RC.table(kind, nact) == RC.table(kind, nact)          # seeded: the same table every time
    if nact == 4:
        assert any(sum(x >> RC.shift_of(max(X)) for x in X) == (1 << 33) - 4 for X in map(lambda t: RC.clamp(t, kind), RC.table(kind, nact)))


@pytest.mark.parametrize("kind", RC.KINDS)
def test_the_restatements_rule_equals_the_exact_rule_on_every_table(kind):
    for nact in (1, 2, 3, 4):
        tab = [RC.clamp(X, kind) for X in RC.table(kind, nact)]
        got = RS.strategy_from(np.array(tab, np.int64).T)
        want = np.array([RC.rule_exact(list(X)) for X in tab], np.int64).T
        assert got.shape == want.shape and (got == want).all(), (kind, nact, [tab[i] for i in np.argwhere((got != want).any(axis=0))[:3, 0]])
        assert (want.sum(axis=0) == RC.ONE).all() and (want >= 0).all()


def test_the_exact_rule_by_hand():
    assert RC.rule_exact([0, 0, 0]) == [10924, 10922, 10922]                  # the uniform row: the remainder to slot 0
    assert RC.rule_exact([5]) == [32768] and RC.rule_exact([0]) == [32768]
    assert RC.rule_exact([1, 3]) == [8192, 24576]
    assert RC.rule_exact([(1 << 31) - 1] * 4) == [8192] * 4                    # the divisor 2^33 - 4
    assert RC.rule_exact([1 << 40, (1 << 9) - 1]) == [32768, 0]               # sh = 10: the companion vanishes
    assert RC.rule_exact([1 << 40, 1 << 10]) == [32768, 0] and RC.rule_exact([1 << 40, 1 << 25]) == [32768, 0] and RC.rule_exact([1 << 40, 1 << 26]) == [32767, 1]
    assert RC.rule_exact([1, 2, 3]) == [32768 - 10922 - 16384, 10922, 16384]


@pytest.mark.parametrize("kind", RC.KINDS)
def test_the_double_quotient_is_the_floor_on_every_table(kind):
    """rs_div's first step: with a correctly rounded division (Python's float is IEEE double) the quotient of a numerator < 2^46 by a divisor
    < 2^33 truncates to the exact floor -- it is at most 2^15, doubles there are 2^-37 apart and a quotient that is no integer lies at least
    2^-33 below the next one -- so the correction step changes nothing unless the division is not correctly rounded"""
    for nact in (2, 3, 4):
        for X in (RC.clamp(t, kind) for t in RC.table(kind, nact)):
            sh = RC.shift_of(max(X))
            S = sum(x >> sh for x in X)
            for x in X:
                num = (x >> sh) << 15
                assert S == 0 or (num < 1 << 46 and S < 1 << 33 and int(float(num) / float(S)) == num // S), (X, x)


def test_the_packer_places_every_tuple_where_it_is_read():
    import solver_trees_util as U
    from pokerl_amd.solver import river_tree
    trees = [U.forced_river_tree(), river_tree(100, 400), U.four_action_river_tree()]
    call = RC.rule_call(5, trees, "average", 7, 47)
    assert RC.covered(call["where"], {n: RC.table("river_A", n) for n in (1, 2, 3, 4)})
    A = call["state"][1]
    assert A.shape == (len(call["where"]), 14, 4, RC.H) and (A == RC.SENTINEL).any()
    for i, put in enumerate(call["where"]):
        for ((row,), h), X in list(put.items())[::97]:
            assert A[i, row, :len(X), h].tolist() == list(X) and (A[i, row, len(X):, h] == RC.SENTINEL).all()
    turn = RC.rule_call(4, [RC.four_action_turn_tree()], "average", 7, 14)
    assert RC.covered(turn["where"] + turn["river_where"], {n: RC.table("turn_A", n) for n in (1, 2, 3, 4)})
    Ar = turn["state"][3]
    for i, put in enumerate(turn["river_where"]):
        for ((row, card), h), X in list(put.items())[::53]:
            assert card in turn["pool"] and Ar[i, row, card, :len(X), h].tolist() == list(X)
    reg = RC.rule_call(5, [RC.nine_node_tree()], "regret", 4095, 47)           # the ROOT row alone takes its whole table
    roots = [{k: v for k, v in put.items() if k[0] == (0,)} for put in reg["where"]]
    assert RC.covered(roots, {2: RC.table("river_R", 2)}) and (reg["ranges"] == 2048).all() and not reg["state"][1].any()


def agree(street, variant, pool):
    call = RC.corner_call(street, pool, variant)
    want = RC.spec_of(street, call)
    got, rec = SW.run_call(street, call)
    assert not want["status"].any() and want["t"].tolist() == [4096]
    for k in KEYS[street]:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (variant, k, np.argwhere(got[k] != want[k])[:4].tolist())
    print("street %d, P = %d, %s: below 2^x, x = %r" % (street, pool, variant, rec.bits()))
    SW.check_bounds(street, rec)
    return call, want, rec


@pytest.mark.parametrize("variant", ["top", "swing", "mix"])
def test_river_corner_python_integers_equal_the_restatement_and_stay_in_bounds(variant):
    """pot + put = 8191, P = 47, every weight 65535, the state at RMAX / AMAX, t = 4094 .. 4096.  Measured (x of 'below 2^x'; the header's
    figure in brackets): a reach 20.0 [20], a sum of reaches 30.08 [31], a terminal's |u| 43.02 [45], any |u| 43.63 [45], |sum sigma u| 58.13
    [60], a regret's step 43.02 [46], |R| 58.0 [59, from the clamp], A 44.0 [45], the rule's numerator 46.0 [46] and divisor 32.0 [33]."""
    call, want, rec = agree(5, variant, 47)
    assert want["valid"].sum() == 1081
    assert rec["reach"] == 65535 << 4 and rec["regret"] >= RC.lim_of("river_R") and rec["average"] > RC.lim_of("river_A")
    if variant == "top":
        assert rec["divisor"] == 2 * ((1 << 31) - 1) and rec["numerator"] == ((1 << 31) - 1) << 15


@pytest.mark.parametrize("variant, pool", [("top", 40), ("swing", 20), ("mix", 12)])
def test_turn_corner_python_integers_equal_the_restatement_and_stay_in_bounds(variant, pool):
    """pot + put = 8191, every weight 65535, the state of both levels at TURN_RMAX / TURN_AMAX, t = 4094 .. 4096; P = 40 is what runs here
    in under a minute (P = 48: the fixture of tests/golden/solver_arith, whose generator runs this same comparison before it writes).
    Measured at P = 48 (the header's figure in brackets): a reach 17.0 [17], a sum of reaches 27.14 [27.2], a river-level terminal's |u|
    38.95 [41.2], the chance node's and a turn-level fold's |u| 45.34 [46.7], any |u| 46.09 [46.7], |sum sigma u| 60.27 [61.7], a regret's
    step 43.88 [47.7], |R| 60.0 [60.3, from the clamp], A 41.0 [42], the rule's numerator 46.0 [46] and divisor 32.0 [33]."""
    call, want, rec = agree(4, variant, pool)
    assert int(want["P"][0]) == pool and rec["reach"] == 65535 << 1 and rec["regret"] >= RC.lim_of("turn_R")


def test_the_fixture_is_what_its_generator_writes():
    """the P = 48 turn corner: its inputs are corner_call's (so the GPU test and the CPU build are given the call the witness was)"""
    fx = np.load(GOLDEN)
    call = RC.corner_call(4, 48, "top")
    assert fx["board"].tolist() == call["board"][0].tolist() and int(fx["dead"]) == int(call["dead"][0]) == 0
    assert fx["tree_args"].tolist() == [2731, 5460, 1] and int(fx["t0"]) == 4093 and int(fx["iters"]) == 3 and int(fx["weight"]) == 65535
    assert int(fx["status"]) == 0 and fx["strategy"].shape == (4, 4, RC.H) and fx["value"].shape == (2, RC.H) and fx["br"].any()
    assert all(len(str(fx["sha256_" + k])) == 64 for k in ("river_strategy", "regret", "average", "river_regret", "river_average"))
    assert os.path.getsize(GOLDEN) < 100 << 10
