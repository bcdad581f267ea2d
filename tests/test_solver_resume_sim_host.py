"""The resuming kernels' real bodies -- k_rs_prep / k_ts_prep, k_trees_prep, k_resolve_prep, k_resume_prep and k_resume_river_solve /
k_resume_turn_solve, the text of pokerl_amd/csrc/pk_river_solver.hip and pk_turn_solver.hip -- run on the CPU as workgroups of 8 x 64
lanes (tools/host_sim/equity_sim.cpp -DPK_ES_ONLY=20 / 21 on wg_shim.h: every collective a checked rendezvous, LDS refilled with garbage
before every workgroup, PK_IDX on every LDS and work-space subscript, every array -- the state arrays too -- an allocation of exactly its
size).  No GPU.  Every case runs at a grid of 1, so that ONE workgroup takes the spots in turn and the state, the t0 or stale regrets of
the spot before would show.  Every state array is pre-filled with a sentinel, which must come back wherever the definition says the entry
is not written.  Every output and the whole state are compared byte for byte with tests/resume_spec.py: nothing expected comes from a
kernel.  The same cases under ASan + UBSan and TSan: tools/host_sim/sanitize_equity.sh --only sum-.
The ARITHMETIC cases (river_arith_cases / turn_arith_cases, case functions of their own because a state at the clamps holds no sentinel): the
operand tables of tests/solver_rule_cases.py through the rule and the bounds corner, so that what tests/test_hip_solver_arithmetic.py
gives the device is never compared with the device only; under UBSan (--only arith-) a signed overflow in the kernel bodies stops the run."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "host_sim"))

import equity_cases as EC        # noqa: E402
import resume_spec as RM         # noqa: E402
import solver_resume_util as MU  # noqa: E402

RIVER = [c for c in EC.river_resume_cases() if c.quick]
TURN = [c for c in EC.turn_resume_cases() if c.quick]
RIVER_ARITH = [c for c in EC.river_arith_cases() if c.quick]
TURN_ARITH = [c for c in EC.turn_arith_cases() if c.quick]


def build(tmp_path_factory, only, tag):
    if not shutil.which("g++"):
        pytest.fail("g++ not found: the CPU build of the kernel bodies needs it")
    out = tmp_path_factory.mktemp("equity_sim_" + tag)
    exe = str(out / ("equity_sim_" + tag))
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-DPK_HOST_SIM", "-I", os.path.join(ROOT, "tools", "host_sim", "stub"),
                        "-include", os.path.join(ROOT, "tools", "host_sim", "wg_shim.h"), "-DPK_ES_ONLY=%d" % only,
                        os.path.join(ROOT, "tools", "host_sim", "equity_sim.cpp"), "-o", exe], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe, str(out)


@pytest.fixture(scope="module")
def river_sim(tmp_path_factory):
    return build(tmp_path_factory, 20, "rsum")


@pytest.fixture(scope="module")
def turn_sim(tmp_path_factory):
    return build(tmp_path_factory, 21, "tsum")


def field(case, key):
    return np.asarray(case.arrays[key][1])


@pytest.mark.parametrize("cases, family, prefix", [(RIVER, "riverresume", "rsum-"), (TURN, "turnresume", "tsum-")])
def test_the_cases_cover_what_a_resumed_solve_can_get_wrong(cases, family, prefix):
    by = {c.name: c for c in cases}
    assert all(c.family == family and c.name.startswith(prefix) and int(field(c, "grid")[0]) == 1 for c in cases) and len(cases) >= 8
    assert not {c.name for c in EC.all_cases()} & set(by)                     # not part of all_cases()
    sent = np.uint64(MU.SENTINEL)
    assert all((field(c, "regret") == sent).any() for c in cases)             # every state array holds the sentinel somewhere
    assert field(by[prefix + "t0-after-zero-and-back"], "t0").tolist()[:3] == [0, 3, 0] and field(by[prefix + "zero-after-t0"], "t0").tolist()[1] == 0
    bad = by[prefix + "refused-bad-iter-dup-card-between"]
    want = bad.expected()
    st = want["status"].tolist()
    assert st[0] == 0 and st[-1] == 0 and st.count(RM.BAD_ITER) >= 1 and 2 in st and 32 in st
    for i, s in enumerate(st):
        if s:                                                                 # a refused spot: outputs 0, the state as it came
            assert not want["value"][i].any() and (want["regret"][i] == field(bad, "regret")[i]).all() and (want["average"][i] == field(bad, "average")[i]).all()
    locked = by[prefix + "locked-rows-keep-their-state"]
    want, lock = locked.expected(), field(locked, "lock").astype(bool)
    assert (want["regret"][0][lock[0]] == sent).all() and not want["regret"][1][lock[1]].any() and field(locked, "t0").tolist()[:2] == [2, 0]
    assert int(field(by[prefix + "iters0"], "iters")[0]) == 0
    over = field(by[prefix + "state-beyond-both-clamps"], "regret").view(np.int64)
    assert (over == np.iinfo(np.int64).min).any() and (over == np.iinfo(np.int64).max).any() and (over < 0).any()
    big = by[prefix + "large-after-small"]
    n, of = field(big, "n"), field(big, "tree_of")
    assert int(n[of[1]]) > int(n[of[0]])
    rows = by[prefix + ("pools-4-9-33" if family == "riverresume" else "pools-5-9-20")].expected()["strategy"][:, 0].astype(np.int64)
    pools = (rows.sum(axis=1) == 32768).sum(axis=1).tolist()                 # a valid holding's root row sums to ONE
    assert pools == ([6, 36, 528] if family == "riverresume" else [10, 36, 190])                     # C(P, 2) valid holdings


@pytest.mark.parametrize("case", RIVER, ids=[c.name for c in RIVER])
def test_river_kernel_as_512_lane_workgroups_vs_spec(river_sim, case):
    exe, work = river_sim
    bad, sec, log = EC.run_case(exe, case, work, timeout=300)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: riverresume done" in log and "LDS bytes" in log


@pytest.mark.parametrize("case", TURN, ids=[c.name for c in TURN])
def test_turn_kernel_as_512_lane_workgroups_vs_spec(turn_sim, case):
    exe, work = turn_sim
    bad, sec, log = EC.run_case(exe, case, work, timeout=300)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: turnresume done" in log and "LDS bytes" in log


def test_the_arithmetic_cases_carry_the_tables_and_the_corner():
    import solver_rule_cases as RC
    names = {c.name for c in EC.river_arith_cases() + EC.turn_arith_cases()}
    assert not names & {c.name for c in EC.all_cases() + EC.river_resume_cases() + EC.turn_resume_cases()} and len(RIVER_ARITH) == 6 and len(TURN_ARITH) >= 2
    assert "tarith-corner-p48-fixture" in names and all(int(field(c, "grid")[0]) == 1 for c in RIVER_ARITH + TURN_ARITH)
    by = {c.name: c for c in RIVER_ARITH}
    avg = field(by["rarith-rule-average"], "average").view(np.int64).reshape(-1, 14, 4, 1326)
    placed = {tuple(int(v) for v in avg[i, row, :n, h]) for i in range(len(avg)) for row, n in ((0, 1),) for h in range(1326)}
    assert int(field(by["rarith-rule-average"], "iters")[0]) == 0 and (avg == np.iinfo(np.int64).min).any() and (avg == np.iinfo(np.int64).max).any()
    assert len(placed) > 1 and (RC.lim_of("river_A"),) in placed
    top = by["rarith-corner-top"]
    assert (field(top, "regret").view(np.int64) == RC.lim_of("river_R")).all() and field(top, "t0").tolist() == [4093] and int(field(top, "iters")[0]) == 3
    assert (field(top, "ranges") == 65535).all() and field(top, "pot").tolist() == [1001] and int(field(top, "put").max()) == 7190


@pytest.mark.parametrize("case", RIVER_ARITH, ids=[c.name for c in RIVER_ARITH])
def test_river_arithmetic_as_512_lane_workgroups_vs_spec_and_exact_rule(river_sim, case):
    exe, work = river_sim
    bad, sec, log = EC.run_case(exe, case, work, timeout=300)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: riverresume done" in log


@pytest.mark.parametrize("case", TURN_ARITH, ids=[c.name for c in TURN_ARITH])
def test_turn_arithmetic_as_512_lane_workgroups_vs_spec_and_exact_rule(turn_sim, case):
    exe, work = turn_sim
    bad, sec, log = EC.run_case(exe, case, work, timeout=600)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: turnresume done" in log
