"""The locked solver kernels' real bodies -- k_rs_prep / k_ts_prep, k_trees_prep and k_lock_river_solve / k_lock_turn_solve, the text of
pokerl_amd/csrc/pk_river_solver.hip and pk_turn_solver.hip -- run on the CPU as workgroups of 8 x 64 lanes (tools/host_sim/equity_sim.cpp
-DPK_ES_ONLY=16 / 17 on wg_shim.h: every collective a checked rendezvous, LDS refilled with garbage before every workgroup, PK_IDX on every
LDS and work-space subscript, every array -- the lock arrays too -- an allocation of exactly its size, work arrays and outputs pre-filled).
No GPU.  Every case runs at a grid of 1, so that ONE workgroup takes the spots in turn and a stale sigma, stale flags or stale packed
regret words of the spot before would show.  Every output is compared byte for byte with tests/solver_lock_spec.py: nothing expected
comes from a kernel.  What the definition says is not read holds 0xFFFF in every case (equity_cases.lock_arrays).  The same cases under
ASan + UBSan and TSan: tools/host_sim/sanitize_equity.sh --only lock-."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "host_sim"))

import equity_cases as EC        # noqa: E402

RIVER = [c for c in EC.river_lock_cases() if c.quick]
TURN = [c for c in EC.turn_lock_cases() if c.quick]


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
    return build(tmp_path_factory, 16, "rlock")


@pytest.fixture(scope="module")
def turn_sim(tmp_path_factory):
    return build(tmp_path_factory, 17, "tlock")


def field(case, key):
    return np.asarray(case.arrays[key][1])


@pytest.mark.parametrize("cases, family, prefix, pools", [(RIVER, "riverlock", "rlock-", (4, 9, 33)), (TURN, "turnlock", "tlock-", (5, 9, 20))])
def test_the_cases_cover_what_a_lock_can_get_wrong(cases, family, prefix, pools):
    by = {c.name: c for c in cases}
    assert all(c.family == family and c.name.startswith(prefix) and int(field(c, "grid")[0]) == 1 for c in cases) and len(cases) >= 7
    others = {c.name for c in EC.all_cases()} | {c.name for c in EC.river_trees_cases()} | {c.name for c in EC.turn_trees_cases()}
    assert not others & set(by)                                               # not part of all_cases(), no name taken twice
    seq = by[prefix + "free-all-p1-all-free"]                                 # fully locked after free and the reverse, one player between
    lock = field(seq, "lock")
    assert not lock[0].any() and lock[1].all() and lock[2].any() and not lock[2].all() and lock[3].all() and not lock[4].any()
    assert seq.arrays["tree_of"][1] is None and int(field(seq, "ntrees")[0]) == 1      # one tree, no tree_of
    bad = by[prefix + "refused-with-ffff-between"]
    st = bad.expected()["status"].tolist()
    assert st[0] == 0 and st[1] not in (0, 32) and st[2] == 32 and st[3] == 0 and (field(bad, "locked")[1:3] == 0xFFFF).all() and (field(bad, "lock")[1:3] == 0xFF).all()
    zero = by[prefix + "all-zero-rows-are-uniform"]
    assert field(zero, "lock")[0].all() and not (field(zero, "locked")[0][..., :1, :] != 0).any()
    want = zero.expected()["strategy"][0]                                     # a locked all-zero row: the uniform row at every valid holding
    valid = want[0, 0] != 0
    assert valid.any() and set(np.unique(want[0, 0][valid]).tolist()) <= {32768, 16384, 32768 - 2 * (32768 // 3), 8192}
    assert int(field(by[prefix + "iters0"], "iters")[0]) == 0
    assert by[prefix + "lock-null"].arrays.get("lock") is None
    sizes = next(c for c in cases if "pools" in c.name)
    assert tuple(int(x) for x in (52 - np.array([bin(int(d)).count("1") for d in field(sizes, "dead")]) - field(sizes, "board").shape[1])) == pools
    big = by[prefix + "large-after-small-locks-past-its-rows"]
    n, of, lock = field(big, "n"), field(big, "tree_of"), field(big, "lock")
    assert int(n[of[1]]) > int(n[of[0]]) and lock[0].sum() > 0 and lock.shape[1] > 2      # rows the small tree does not have carry flags


@pytest.mark.parametrize("case", RIVER, ids=[c.name for c in RIVER])
def test_river_kernel_as_512_lane_workgroups_vs_spec(river_sim, case):
    exe, work = river_sim
    bad, sec, log = EC.run_case(exe, case, work, timeout=300)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: riverlock done" in log and "LDS bytes" in log


@pytest.mark.parametrize("case", TURN, ids=[c.name for c in TURN])
def test_turn_kernel_as_512_lane_workgroups_vs_spec(turn_sim, case):
    exe, work = turn_sim
    bad, sec, log = EC.run_case(exe, case, work, timeout=300)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: turnlock done" in log and "LDS bytes" in log
