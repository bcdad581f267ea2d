"""The ranged sampled equity's real kernel bodies -- k_eqw_cdf, k_eqw_prep, k_eqw<N, RC>, the text of pokerl_amd/csrc/pk_equity_ranged.hip -- run
on the CPU as workgroups of 8 waves x 64 lanes (tools/host_sim/equity_sim.cpp -DPK_ES_ONLY=6 on wg_shim.h: every collective a checked
rendezvous, LDS refilled with garbage before every workgroup, PK_IDX on every LDS subscript, every array an allocation of exactly its size,
outputs pre-filled).  No GPU.  Every output array is compared, by exact integer equality, with tests/equity_ranged_spec.py
(tools/host_sim/equity_cases.py ranged_cases(): nothing expected comes from a kernel).  The same cases under ASan + UBSan and TSan:
tools/host_sim/sanitize_equity.sh."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "host_sim"))

import equity_cases as EC   # noqa: E402

CASES = [c for c in EC.ranged_cases() if c.quick]


@pytest.fixture(scope="module")
def equity_sim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ not found: the CPU build of the kernel bodies needs it")
    out = tmp_path_factory.mktemp("equity_sim_ranged")
    exe = str(out / "equity_sim_ranged")
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-DPK_HOST_SIM", "-I", os.path.join(ROOT, "tools", "host_sim", "stub"),
                        "-include", os.path.join(ROOT, "tools", "host_sim", "wg_shim.h"), "-DPK_ES_ONLY=6",
                        os.path.join(ROOT, "tools", "host_sim", "equity_sim.cpp"), "-o", exe], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe, str(out)


def test_the_cases_cover_what_the_kernel_can_get_wrong():
    names = {c.name for c in CASES}
    assert all(c.family == "ranged" for c in CASES) and len(CASES) >= 10
    assert not {c.name for c in EC.all_cases()} & {c.name for c in EC.ranged_cases()}
    # stale LDS on a grid of 1, a refused spot between valid ones, H = 16
    assert {"ranged-N2-S1200-grid1-nonce0", "ranged-N6-refused-between", "ranged-N16-H16-R16"} <= names
    h16 = next(c for c in CASES if c.name == "ranged-N16-H16-R16")
    assert int(h16.arrays["grid"][1][0]) == 1 and (h16.expected()["accepted"][:2] == 130).all()
    mid = next(c for c in CASES if c.name == "ranged-N6-refused-between").expected()
    assert mid["status"].tolist() == [0, 2, 0] and mid["accepted"][0] > 0 and mid["accepted"][2] > 0


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_kernel_as_8_wave_workgroups_vs_spec(equity_sim, case):
    exe, work = equity_sim
    bad, sec, log = EC.run_case(exe, case, work, timeout=300)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: ranged done" in log and "LDS bytes" in log
