"""The pre-flop solver kernel's real body -- k_preflop_solve, the text of pokerl_amd/csrc/pk_preflop_solver.hip -- run on the CPU as workgroups
of 8 x 64 lanes (tools/host_sim/equity_sim.cpp -DPK_ES_ONLY=22 on wg_shim.h: every collective a checked rendezvous, LDS refilled with garbage
before every workgroup, PK_IDX on every LDS and work-space subscript, every array -- the packed trees and the work space too -- an allocation
of exactly its size, work arrays and outputs pre-filled).  No GPU.  Every case runs at a grid of 1, so that ONE workgroup takes the spots in
turn and a stale tree, stale regrets or stale LDS of the spot before would show.  The table is the driver's fixed pattern, which has none of
the real table's structure.  Every output is compared byte for byte with tests/preflop_solver_spec.py on the same pattern: nothing expected
comes from a kernel.  The same cases under ASan + UBSan and TSan: tools/host_sim/sanitize_equity.sh --only pfsolve."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "host_sim"))

import equity_cases as EC        # noqa: E402

CASES = [c for c in EC.pfsolve_cases() if c.quick]
BAD_TREE = 32


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ not found: the CPU build of the kernel bodies needs it")
    out = tmp_path_factory.mktemp("equity_sim_pfsolve")
    exe = str(out / "equity_sim_pfsolve")
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-DPK_HOST_SIM", "-I", os.path.join(ROOT, "tools", "host_sim", "stub"),
                        "-include", os.path.join(ROOT, "tools", "host_sim", "wg_shim.h"), "-DPK_ES_ONLY=22",
                        os.path.join(ROOT, "tools", "host_sim", "equity_sim.cpp"), "-o", exe], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe, str(out)


def field(case, key):
    return np.asarray(case.arrays[key][1])


def test_the_cases_cover_what_the_kernel_can_get_wrong():
    by = {c.name: c for c in CASES}
    assert all(c.family == "pfsolve" and c.name.startswith("pfsolve-") and int(field(c, "grid")[0]) == 1 for c in CASES)
    others = {c.name for c in EC.all_cases()} | {c.name for c in EC.river_cases()} | {c.name for c in EC.river_trees_cases()}
    assert not others & set(by)                                               # not part of all_cases(), no name taken twice
    mixed = by["pfsolve-pushfold-after-64-before-3"]
    n, of = field(mixed, "n"), field(mixed, "tree_of")
    assert [int(n[k]) for k in of] == [64, 5, 3, 5]                           # push / fold after the 64-node tree and before the 3-node one
    bad = by["pfsolve-bad-tree-between"]
    st, of, K = bad.expected()["status"].tolist(), field(bad, "tree_of").tolist(), int(field(bad, "ntrees")[0])
    assert st == [0, BAD_TREE, 0, BAD_TREE, 0] and of[1] == K and of[3] == 0xFFFFFFFF
    want = bad.expected()
    assert not want["strategy"][1].any() and not want["value"][1].any() and want["strategy"][2].any() and want["value"][2].any()
    assert not field(by["pfsolve-empty-range"], "ranges").reshape(2, 2, -1)[0, 1].any()
    one = field(by["pfsolve-one-holding"], "ranges").reshape(2, 2, -1)
    assert np.count_nonzero(one[0, 0]) == 1 and np.count_nonzero(one[1, 1]) == 1
    assert {int(field(c, "iters")[0]) for c in CASES} >= {1, 2, 3}
    assert "tree_of" not in by["pfsolve-empty-range"].arrays                  # tree_of NULL: tree 0 everywhere


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_kernel_as_512_lane_workgroups_vs_spec(sim, case):
    exe, work = sim
    bad, sec, log = EC.run_case(exe, case, work, timeout=600)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: pfsolve done" in log and "LDS bytes" in log
