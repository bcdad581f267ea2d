"""The equity kernels' real bodies -- k_equity<N>, k_eqs<N>, k_eqr, k_rvr, k_hist and their preparation kernels, the text of
pokerl_amd/csrc/pk_equity*.hip -- run on the CPU as workgroups of 8 waves x 64 lanes: tools/host_sim/equity_sim.cpp on wg_shim.h (a fibre per
lane, every shuffle / readfirstlane / wave_barrier a checked rendezvous of the wave and __syncthreads one of the workgroup, LDS refilled with
garbage before every workgroup, PK_IDX on every LDS subscript, every array an allocation of exactly its size, outputs pre-filled).  No GPU.
Every output array is compared, by exact integer equality, with the numpy specs (tools/host_sim/equity_cases.py: nothing expected comes from a
kernel).  The full matrix under ASan + UBSan and under TSan is tools/host_sim/sanitize_equity.sh (profiles/equity_sim_sanitizers.txt); here
plain g++ builds, one executable per family compiled side by side, and the cases marked quick: the pad sizes of the sort on river spots and
the small ones on turn spots, the flop walk, every weight form, bins 1 / 7 / 32, stale LDS on a grid of 1, refused spots in between, the
take = 4 fetch regime, three Philox blocks, every status bit and the table form's bad indices.

Measured here (8 CPUs, plain -O1 builds; the driver plus the spec, per case): rvr-turn-small-grid1-spot-w 2.2 s and
hist-turn-small-grid1-spot-w 2.3 s (4 090 barriers of 512 lanes each, 2.0 s of it in the driver), range-table-form-observer-2 1.5 s,
rvr-river-bounds-grid1 0.9 s, hist-river-bounds-grid1 0.8 s, rvr-table-form 0.7 s, every other case below 0.7 s; the five builds side by side
6 s, the self-test's 1.6 s; the module 23 s."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "host_sim"))

import equity_cases as EC   # noqa: E402

FAMILIES = {"equity": 1, "sampled": 2, "range": 3, "rvr": 4, "hist": 5}      # -DPK_ES_ONLY of tools/host_sim/equity_sim.cpp
CASES = [c for c in EC.all_cases() if c.quick]


@pytest.fixture(scope="module")
def equity_sim(tmp_path_factory):
    """{family: executable}"""
    if not shutil.which("g++"):
        pytest.fail("g++ not found: the CPU build of the kernel bodies needs it")
    out = tmp_path_factory.mktemp("equity_sim")
    exe = {fam: str(out / ("equity_sim_" + fam)) for fam in FAMILIES}
    jobs = {fam: subprocess.Popen(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-DPK_HOST_SIM", "-I", os.path.join(ROOT, "tools", "host_sim", "stub"),
                                   "-include", os.path.join(ROOT, "tools", "host_sim", "wg_shim.h"), "-DPK_ES_ONLY=%d" % part,
                                   os.path.join(ROOT, "tools", "host_sim", "equity_sim.cpp"), "-o", exe[fam]],
                                  cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for fam, part in FAMILIES.items()}
    for fam, job in jobs.items():
        _, err = job.communicate()
        assert job.returncode == 0, (fam, err[-4000:])
    return exe, str(out)


def test_the_quick_cases_cover_every_family():
    assert {c.family for c in CASES} == set(FAMILIES) and len(CASES) >= 30


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_kernel_as_8_wave_workgroups_vs_spec(equity_sim, case):
    exe, work = equity_sim
    bad, sec, log = EC.run_case(exe[case.family], case, work, timeout=300)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: %s done" % case.family in log and "LDS bytes" in log


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wg_shim") / "wg_shim_selftest")
    subprocess.run(["g++", "-std=c++20", "-O1", "-DPK_HOST_SIM", "-I", os.path.join(ROOT, "tools", "host_sim", "stub"), "-include",
                    os.path.join(ROOT, "tools", "host_sim", "wg_shim.h"), os.path.join(ROOT, "tools", "host_sim", "wg_shim_selftest.cpp"), "-o", exe], check=True, cwd=ROOT)
    return exe


@pytest.mark.parametrize("mode,status,says", [
    ("ok", 0, "wg_shim_selftest ok: done"),
    ("split-barrier", 3, "lanes of one workgroup meet at DIFFERENT __syncthreads"),
    ("split-wave", 3, "split between a wave collective and __syncthreads"),
    ("left-lane", 3, "shuffle from a lane that is not active: source lane 5"),
    ("index", -6, "index out of range: box: 8, limit 8"),
])
def test_the_shim_reports_and_never_hangs(selftest, mode, status, says):
    """wg_shim.h on kernels small enough to read: shuffles in 32 and 64 bits, atomics, garbage LDS in every workgroup, lanes that leave; a
    barrier or a collective in divergent control flow and a shuffle from a lane that has left end the program with status 3 and the sites;
    PK_IDX aborts with the array's name."""
    r = subprocess.run([selftest, mode], capture_output=True, text=True, timeout=60)
    assert r.returncode == status and says in r.stdout + r.stderr, (r.returncode, r.stdout[-1000:], r.stderr[-1000:])
