"""The showdown EV's real kernel bodies -- k_ev_prep<N, TABLE>, k_ev<N>, k_ev_finish, the text of pokerl_amd/csrc/pk_equity_ev.hip -- run on
the CPU as workgroups of 8 waves x 64 lanes (tools/host_sim/equity_sim.cpp -DPK_ES_ONLY=7 on wg_shim.h: every collective a checked
rendezvous, LDS refilled with garbage before every workgroup, PK_IDX on every LDS subscript, every array an allocation of exactly its size,
work arrays and outputs pre-filled).  No GPU.  Every output array is compared with tests/ev_spec.py (tools/host_sim/equity_cases.py
ev_cases(): nothing expected comes from a kernel): the integers by exact equality, `amount` and `ev` bit for bit (they travel as their bit
patterns).  The same cases under ASan + UBSan and TSan: tools/host_sim/sanitize_equity.sh."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "host_sim"))

import equity_cases as EC   # noqa: E402
import ev_spec as EV        # noqa: E402

CASES = [c for c in EC.ev_cases() if c.quick]


@pytest.fixture(scope="module")
def equity_sim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ not found: the CPU build of the kernel bodies needs it")
    out = tmp_path_factory.mktemp("equity_sim_ev")
    exe = str(out / "equity_sim_ev")
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-DPK_HOST_SIM", "-I", os.path.join(ROOT, "tools", "host_sim", "stub"),
                        "-include", os.path.join(ROOT, "tools", "host_sim", "wg_shim.h"), "-DPK_ES_ONLY=7",
                        os.path.join(ROOT, "tools", "host_sim", "equity_sim.cpp"), "-o", exe], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe, str(out)


def test_the_cases_cover_what_the_kernel_can_get_wrong():
    names = {c.name for c in CASES}
    assert all(c.family == "ev" for c in CASES) and len(CASES) >= 8
    assert not {c.name for c in EC.all_cases()} & {c.name for c in EC.ev_cases()}
    # a grid of 1 (stale LDS, stale level tables), a refused spot between valid ones, the smallest spot with a second group of levels
    assert {"ev-N2-grid1", "ev-N3-grid1", "ev-N3-refused-between", "ev-N5-two-groups"} <= names
    for name in ("ev-N2-grid1", "ev-N3-grid1", "ev-N5-two-groups"):
        c = next(c for c in CASES if c.name == name)
        assert int(c.arrays["grid"][1][0]) == 1
        nlev = (c.expected()["level_seat"] != EV.NO_LEVEL).sum(axis=1)
        assert len(set(nlev.tolist())) >= 3, nlev                       # spots with different numbers of levels follow each other
    mid = next(c for c in CASES if c.name == "ev-N3-refused-between").expected()
    assert mid["status"].tolist() == [0, EV.BAD_BET, 0, 2, 0, 4, 0, EV.BAD_BET, 0] and all(mid["boards"][i] > 0 for i in (0, 2, 4, 6, 8))
    # five live seats on a ladder: levels 0 .. 3 are compared -- level 3 lies in the second group of three -- and level 4 is the last stand
    two = next(c for c in CASES if c.name == "ev-N5-two-groups").expected()
    assert (two["level_seat"][0] != EV.NO_LEVEL).all() and all(int(two["share"][0][i].sum()) == EV.SHARE_UNIT * int(two["boards"][0]) for i in range(5))
    assert np.count_nonzero(two["share"][0][4]) == 1 and np.count_nonzero(two["share"][0][3]) == 2


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_kernel_as_8_wave_workgroups_vs_spec(equity_sim, case):
    exe, work = equity_sim
    bad, sec, log = EC.run_case(exe, case, work, timeout=300)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: ev done" in log and "LDS bytes" in log
