"""The ranged showdown EV's real kernel bodies -- k_evw_prep<N, TABLE>, k_evw<N, RC>, k_evw_finish, the text of pokerl_amd/csrc/pk_ev_ranged.hip,
with k_eqw_cdf of pk_equity_ranged.hip -- run on the CPU as workgroups of 8 waves x 64 lanes (tools/host_sim/equity_sim.cpp -DPK_ES_ONLY=11 on
wg_shim.h: every collective a checked rendezvous, LDS refilled with garbage before every workgroup, PK_IDX on every LDS subscript, every array
an allocation of exactly its size, work arrays and outputs pre-filled).  No GPU.  Every output array is compared with tests/ranged_ev_spec.py
(tools/host_sim/equity_cases.py ranged_ev_cases(): nothing expected comes from a kernel): the integers by exact equality, `amount` and `ev` bit
for bit (they travel as their bit patterns).  The same cases under ASan + UBSan and TSan: tools/host_sim/sanitize_equity.sh."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "host_sim"))

import equity_cases as EC      # noqa: E402
import ranged_ev_spec as XS    # noqa: E402

CASES = [c for c in EC.ranged_ev_cases() if c.quick]


@pytest.fixture(scope="module")
def equity_sim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ not found: the CPU build of the kernel bodies needs it")
    out = tmp_path_factory.mktemp("equity_sim_evw")
    exe = str(out / "equity_sim_evw")
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-DPK_HOST_SIM", "-I", os.path.join(ROOT, "tools", "host_sim", "stub"),
                        "-include", os.path.join(ROOT, "tools", "host_sim", "wg_shim.h"), "-DPK_ES_ONLY=11",
                        os.path.join(ROOT, "tools", "host_sim", "equity_sim.cpp"), "-o", exe], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe, str(out)


def case(name):
    return next(c for c in CASES if c.name == name)


def test_the_cases_cover_what_the_kernel_can_get_wrong():
    names = {c.name for c in CASES}
    assert all(c.family == "rangedev" and c.name.startswith("evw-") for c in EC.ranged_ev_cases()) and len(CASES) >= 12
    others = EC.all_cases() + EC.ranged_cases() + EC.ev_cases()
    assert not {c.name for c in others} & {c.name for c in EC.ranged_ev_cases()}
    assert not [c.name for c in EC.ranged_ev_cases() if "ranged" in c.name or "ev-" in c.name]      # (--only ranged / --only ev- do not pick them up)
    # N = 2 and 3 at a grid of 1 (stale LDS, stale level tables): spots with different numbers of levels follow each other
    for name in ("evw-N2-S65-grid1", "evw-N3-grid1"):
        c = case(name)
        assert int(c.arrays["grid"][1][0]) == 1
        nlev = (c.expected()["level_seat"] != XS.NO_LEVEL).sum(axis=1)
        assert len(set(nlev.tolist())) >= 3, nlev
    # a refused spot (BAD_BET and BAD_CARD) between valid ones
    mid = case("evw-N3-refused-between").expected()
    assert mid["status"].tolist() == [0, XS.BAD_BET, 0, 1, 0, 4, 0, XS.BAD_BET, 0] and all(mid["accepted"][i] > 0 for i in (0, 2, 4, 6, 8))
    # five live seats on a ladder with two hidden seats: levels 0 .. 3 are compared -- level 3 lies in the second group of three
    two = case("evw-N5-two-groups").expected()
    acc = int(two["accepted"][0])
    assert acc > 0 and (two["level_seat"][0] != XS.NO_LEVEL).all() and all(int(two["share"][0][i].sum()) == XS.SHARE_UNIT * acc for i in range(5))
    assert np.count_nonzero(two["share"][0][4]) == 1
    assert sum(1 for p in range(5) if int(case("evw-N5-two-groups").arrays["holes"][1][0, p, 0]) == 0xFF) == 2
    # N = 9 with RC = 16, N = 16 on a ladder (two-level groups, eight of them)
    nine, sixteen = case("evw-N9-R16"), case("evw-N16-ladder")
    assert int(nine.arrays["R"][1][0]) == 16 and int(sixteen.arrays["N"][1][0]) == 16
    e16 = sixteen.expected()
    assert (e16["level_seat"][0] != XS.NO_LEVEL).all() and e16["accepted"][0] > 0 and (e16["share"][0].sum(axis=1) > 0).all()
    # R = 0 with range_of NULL; an all-zero range (accepted 0: group 0 still runs, nothing is evaluated); S = 200 and several chunks
    r0 = case("evw-N3-R0")
    assert int(r0.arrays["R"][1][0]) == 0 and r0.arrays["range_of"][1] is None and r0.arrays["weights"][1] is None
    dead = case("evw-N3-dead-range").expected()
    assert dead["status"].tolist() == [0, 0, 0] and dead["accepted"][1] == 0 and dead["accepted"][0] > 0 and (dead["level_seat"][1] != XS.NO_LEVEL).all()
    assert not dead["ev"][1].any()
    assert int(case("evw-N3-S200").arrays["samples"][1][0]) == 200 and int(case("evw-N3-S1200-grid1-nonce0").arrays["samples"][1][0]) > 2 * 512


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_kernel_as_8_wave_workgroups_vs_spec(equity_sim, case):
    exe, work = equity_sim
    bad, sec, log = EC.run_case(exe, case, work, timeout=300)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: rangedev done" in log and "LDS bytes" in log
