"""The river solver's real kernel bodies -- k_rs_prep and k_river_solve, the text of pokerl_amd/csrc/pk_river_solver.hip -- run on the CPU as
workgroups of 8 x 64 lanes, the width the kernel is compiled for (tools/host_sim/equity_sim.cpp -DPK_ES_ONLY=12 on wg_shim.h: every
collective a checked rendezvous, LDS refilled with garbage before every workgroup, PK_IDX on every LDS and work-space subscript, every array
an allocation of exactly its size, work arrays and outputs pre-filled).  No GPU.  Every output is compared with tests/river_solver_spec.py
byte for byte (tools/host_sim/equity_cases.py river_cases(): nothing expected comes from a kernel).  The same cases under ASan + UBSan and
TSan: tools/host_sim/sanitize_equity.sh --only rsolve."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "host_sim"))

import equity_cases as EC        # noqa: E402

CASES = [c for c in EC.river_cases() if c.quick]


@pytest.fixture(scope="module")
def equity_sim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ not found: the CPU build of the kernel bodies needs it")
    out = tmp_path_factory.mktemp("equity_sim_rsolve")
    exe = str(out / "equity_sim_rsolve")
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-DPK_HOST_SIM", "-I", os.path.join(ROOT, "tools", "host_sim", "stub"),
                        "-include", os.path.join(ROOT, "tools", "host_sim", "wg_shim.h"), "-DPK_ES_ONLY=12",
                        os.path.join(ROOT, "tools", "host_sim", "equity_sim.cpp"), "-o", exe], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe, str(out)


def pools(case):
    board, dead = case.arrays["board"][1], case.arrays["dead"][1]
    return [52 - 5 - bin(int(d)).count("1") for d in dead]


def test_the_cases_cover_what_the_kernel_can_get_wrong():
    by = {c.name: c for c in CASES}
    assert all(c.family == "riversolve" for c in CASES) and len(CASES) >= 10
    others = {c.name for c in EC.all_cases()} | {c.name for c in EC.hero_hist_cases()} | {c.name for c in EC.cluster_cases()}
    assert not others & set(by)
    grid1 = by["rsolve-pools-grid1"]
    assert int(grid1.arrays["grid"][1][0]) == 1 and pools(grid1) == [4, 9, 33, 46]          # one workgroup, the pools following each other
    assert {int(c.arrays["iters"][1][0]) for c in CASES} >= {1, 2}
    st = by["rsolve-refused-between"].expected()["status"].tolist()
    assert int(by["rsolve-refused-between"].arrays["grid"][1][0]) == 1 and st[0] == 0 and st[1] != 0 and st[2] == 0
    ties = by["rsolve-all-ties"]
    for board, dead in zip(ties.arrays["board"][1], ties.arrays["dead"][1]):                 # the board plays for everyone
        _, beats, split, loses = EC.RVS.pairwise([int(x) for x in board], EC.RVS.check_spot([int(x) for x in board], int(dead))[1])
        assert split.any() and not beats.any() and not loses.any()
    assert not ties.expected()["status"].any()
    z = by["rsolve-one-range-zero"]
    ranges = z.arrays["ranges"][1]
    assert not ranges[0, 1].any() and not ranges[1, 0].any() and ranges[0, 0].any()
    assert not z.expected()["value"].view("int64")[0, 0].any()
    assert max(int(c.arrays["n"][1][0]) for c in CASES) == 39 and any(c.arrays["child"][1][0, 3] != 0xFF for c in CASES)   # a four-action root


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_kernel_as_512_lane_workgroups_vs_spec(equity_sim, case):
    exe, work = equity_sim
    bad, sec, log = EC.run_case(exe, case, work, timeout=300)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: riversolve done" in log and "LDS bytes" in log
