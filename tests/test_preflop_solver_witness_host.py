"""The pre-flop solver's 64-bit bounds at their corner (include/pokerl_hip.h "Pre-flop solver", BOUNDS), no GPU: the
Python-integer walk of tests/preflop_solver_witness.py against the numpy int64 restatement of tests/preflop_solver_spec.py on a push / fold tree
with pot + put = 8 191, every weight 65 535, iterations 4 094 .. 4 096 from regrets and accumulators as large as 4 093 iterations can have
left them, and the three extreme tables (every disjoint pair won, tied, lost).  Equal in every output, and every recorded value inside its
bound."""
import numpy as np
import pytest

import preflop_solver_spec as PFS
import preflop_solver_witness as W

H = PFS.HOLDINGS
KIND, CHILD = [0, 2, 1, 3, 4], [[1, 2], [], [3, 4], [], []]
PUT, POT = [[1, 2], [1, 2], [8190, 2], [8190, 2], [8190, 8190]], 1            # pot + max put = 8 191, pot + 2c = 16 381
T0, ITERS = 4093, 3
STEP_MAX, REACH = (1 << 46) - 1, 65535 << 4
# measured by this test, as "below 2^x" (the largest over the three tables), beside the header's bound
MEASURED = {"E": 51.97, "product": 65.97, "u": 44.26, "sigma_u": 59.26, "step": 43.68, "regret": 58.0, "average": 43.0}


def corner_state():
    """regrets up to 4 093 steps of the largest size, accumulators up to 4 093 iterations of the whole reach; zeros and small entries between"""
    R, A = {}, {}
    for d in (0, 2):
        R[d] = [[0 if (h + a) % 11 == 0 else (T0 * STEP_MAX) >> ((7 * a + h) % 5 * 9) for h in range(H)] for a in range(2)]
        A[d] = [[((T0 * (T0 + 1) // 2) * REACH) >> ((a + h) % 3 * 20) for h in range(H)] for a in range(2)]
    return R, A


def spec_tree():
    child = [c + [0xFF] * (4 - len(c)) for c in CHILD]
    return PFS.Tree(KIND, child, PUT, POT)


@pytest.mark.parametrize("name, g", [("all-win", 2 * PFS.BOARDS), ("all-tie", PFS.BOARDS), ("all-lose", 0)])
def test_the_walk_in_python_integers_equals_the_restatement_at_the_corner(name, g):
    weights = [[65535] * H, [65535] * H]
    R, A = corner_state()
    sigma, value, br, rec = W.walk(KIND, CHILD, PUT, POT, g, weights, R, A, T0, ITERS)
    win = PFS.DISJOINT * (PFS.BOARDS if name == "all-win" else 0)
    tie = PFS.DISJOINT * (PFS.BOARDS if name == "all-tie" else 0)
    assert ((2 * win + tie) == g * PFS.DISJOINT).all()
    R0, A0 = corner_state()
    state = ({d: np.array(R0[d], np.int64) for d in R0}, {d: np.array(A0[d], np.int64) for d in A0}, T0)
    r = PFS.solve_spot((win.astype(np.uint32), tie.astype(np.uint32)), np.array(weights, np.uint16), spec_tree(), ITERS, state=state)
    for row, d in enumerate((0, 2)):
        assert r["strategy"][row, :2].tolist() == sigma[d] and not r["strategy"][row, 2:].any()
    assert [[int(x) for x in v] for v in r["value"]] == value
    assert [[int(x) for x in v] for v in r["br"]] == br
    for key, bound in W.BOUNDS.items():
        print("%-8s %-8s below 2^%.4f (bound 2^%d)" % (name, key, W.below(rec[key]), bound))
        assert rec[key] < (1 << bound), (key, rec[key])
        assert W.below(rec[key]) <= MEASURED[key] + 0.01, (key, W.below(rec[key]))          # ... and what DESIGN.md lists is what was seen
    if name == "all-win":
        assert rec["product"] >= (1 << 64) and rec["E"] > (1 << 51)                           # the product does pass 64 bits: the split is needed
