"""The turn solver's real kernel bodies -- k_ts_prep and k_turn_solve, the text of pokerl_amd/csrc/pk_turn_solver.hip -- run on the CPU as
workgroups of 8 x 64 lanes, the width the kernel is compiled for (tools/host_sim/equity_sim.cpp -DPK_ES_ONLY=13 on wg_shim.h: every
collective a checked rendezvous, LDS refilled with garbage before every workgroup, PK_IDX on every LDS and work-space subscript, every array
an allocation of exactly its size, work arrays and outputs pre-filled).  No GPU.  Every output, river_strategy included, is compared with
tests/turn_solver_spec.py byte for byte (tools/host_sim/equity_cases.py turn_cases(): nothing expected comes from a kernel).  The same
cases, and the full-pool fixture, under ASan + UBSan and TSan: tools/host_sim/sanitize_equity.sh --only tsolve."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "host_sim"))

import equity_cases as EC        # noqa: E402

ALL = EC.turn_cases()
CASES = [c for c in ALL if c.quick]


@pytest.fixture(scope="module")
def equity_sim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ not found: the CPU build of the kernel bodies needs it")
    out = tmp_path_factory.mktemp("equity_sim_tsolve")
    exe = str(out / "equity_sim_tsolve")
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-DPK_HOST_SIM", "-I", os.path.join(ROOT, "tools", "host_sim", "stub"),
                        "-include", os.path.join(ROOT, "tools", "host_sim", "wg_shim.h"), "-DPK_ES_ONLY=13",
                        os.path.join(ROOT, "tools", "host_sim", "equity_sim.cpp"), "-o", exe], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe, str(out)


def pools(case):
    return [52 - 4 - bin(int(d)).count("1") for d in case.arrays["dead"][1]]


def test_the_cases_cover_what_the_kernel_can_get_wrong():
    by = {c.name: c for c in ALL}
    assert all(c.family == "turnsolve" and c.name.startswith("tsolve-") and int(c.arrays["grid"][1][0]) == 1 for c in ALL) and len(CASES) >= 8
    others = {c.name for c in EC.all_cases()} | {c.name for c in EC.river_cases()}
    assert not others & set(by)                                               # its own function, not folded into all_cases()
    assert pools(by["tsolve-pools-grid1"]) == [5, 9, 20, 33]                  # one workgroup, the pools following each other
    assert {int(c.arrays["iters"][1][0]) for c in CASES} >= {1, 2, 3}
    st = by["tsolve-refused-between"].expected()["status"].tolist()
    assert st[0] == 0 and st[1] != 0 and st[2] == 0
    plays = by["tsolve-board-plays"]
    assert not plays.expected()["status"].any()
    for board, dead in zip(plays.arrays["board"][1], plays.arrays["dead"][1]):   # some river card makes the board play for everyone
        _, gone = EC.TSS.check_spot([int(x) for x in board], int(dead))
        sp = EC.TSS.spot_of([int(x) for x in board], gone)
        assert any((res != 0).any() and not ((res == 1) | (res == 2)).any() for _, _, res in sp.river)
        assert any(((res == 1) | (res == 2)).any() for _, _, res in sp.river)
    z = by["tsolve-one-range-zero"]
    ranges = z.arrays["ranges"][1]
    assert not ranges[0, 1].any() and not ranges[1, 0].any() and ranges[0, 0].any()
    assert not z.expected()["value"].view("int64")[0, 0].any()
    kind = [int(k) for k in z.arrays["kind"][1]]
    tree = EC.TSS.as_tree(EC.turn_feature_tree())
    assert kind == tree.kind and z.arrays["child"][1][0, 3] != 0xFF            # a four-action root
    folds = [v for v in range(tree.n) if tree.kind[v] in (2, 3)]
    assert any(tree.river[v] for v in folds) and any(not tree.river[v] for v in folds)
    assert any(tree.kind[v] == 5 and tree.kind[tree.child[v][0]] == 4 for v in range(tree.n))       # all-in: chance -> showdown
    full = by["tsolve-p48-fixture"]
    assert not full.quick and pools(full) == [48] and "river_strategy" not in full.outputs


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_kernel_as_512_lane_workgroups_vs_spec(equity_sim, case):
    exe, work = equity_sim
    bad, sec, log = EC.run_case(exe, case, work, timeout=300)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: turnsolve done" in log and "LDS bytes" in log
