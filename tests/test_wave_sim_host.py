"""The table kernels' real body (rollout_body of pk_table_kernels.hpp) run 64 lanes wide on the CPU -- tools/host_sim/wave_sim.cpp on
wave_shim.h: one thread per lane, every ballot / readlane / shuffle / barrier a checked rendezvous, LDS a garbage-filled heap object of
exactly sizeof(LDS), index checks on the evaluator's table and the showdown queue -- against the oracle.  No GPU.  The full matrix
(every family, seat counts up to 16, under ASan + UBSan and TSan) is tools/host_sim/sanitize_wave.sh; here plain g++ builds of five
instantiations, one small configuration each: k_rollout_tab<6> (split, deferring launches), k_rollout_allin_tab<9> (equal stacks:
every seat of every lane in the showdown, two hands per lane, the dummy slot), k_step<6> (the lone-table paths) -- wave_sim.cpp's part 100
-- and two of the wide seat counts from the parts the file already has: k_step<16> (part 10: two np.sum blocks, the policy nibble in bits
60 .. 63) and k_rollout<13> (part 2; the file has no step case at 13 seats).  One executable per part, compiled side by side: each part
takes about as long as part 100.  The step kernels' body also runs the actions of the oracle's never-fold caller (wave_sim --deep:
oracle/rng_spec.py POLICY_DEEP on per-seat fractional stacks, 120 steps) -- k_step<6>, k_step<16> and k_step_async<6> (part 11) finishing
hands raised on every street, with side pots built over several streets."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


PARTS = (100, 10, 2, 11)         # -DPK_WS_PART of tools/host_sim/wave_sim.cpp


@pytest.fixture(scope="module")
def wave_sim(tmp_path_factory):
    """{part: executable}"""
    if not shutil.which("g++") or not shutil.which("gcc"):
        pytest.fail("g++ / gcc not found: the CPU build of the kernel bodies needs them")
    out = tmp_path_factory.mktemp("wave_sim")
    obj = str(out / "oracle.o")
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-c", os.path.join(ROOT, "oracle", "pokerl_oracle.c"), "-o", obj], check=True, cwd=ROOT)
    exe = {part: str(out / ("wave_sim_%d" % part)) for part in PARTS}
    jobs = {part: subprocess.Popen(["g++", "-std=c++20", "-O1", "-pthread", "-ffp-contract=off", "-DPK_HOST_SIM", "-include", os.path.join(ROOT, "tools", "host_sim", "wave_shim.h"),
                                    "-DPK_WS_PART=%d" % part, "-DPK_WS_MAIN", os.path.join(ROOT, "tools", "host_sim", "wave_sim.cpp"), obj, "-o", exe[part]],
                                   cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for part in PARTS}
    for part, job in jobs.items():
        _, err = job.communicate()
        assert job.returncode == 0, (part, err[-4000:])
    return exe


@pytest.mark.parametrize("part,family,n", [(100, "tab", 6), (100, "allin_tab", 9), (100, "step", 6), (10, "step", 16), (2, "rollout", 13)],
                         ids=["tab-6", "allin_tab-9", "step-6", "step-16", "rollout-13"])
def test_kernel_body_64_lanes_wide_vs_oracle(wave_sim, part, family, n):
    r = subprocess.run([wave_sim[part], family, str(n), "--quick"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "%s N=%d: 1 runs" % (family, n) in r.stdout and "wave-sim == oracle" in r.stdout and "wave_sim: 1 cases == oracle" in r.stdout, r.stdout
    assert "MISMATCH" not in r.stdout


@pytest.mark.parametrize("part,family,n", [(100, "step", 6), (10, "step", 16), (11, "step_async", 6)], ids=["step-6", "step-16", "step_async-6"])
def test_step_body_on_deep_hands_vs_oracle(wave_sim, part, family, n):
    """The run itself fails where no hand ended at the river among three or more seats; the count is in its line."""
    r = subprocess.run([wave_sim[part], family, str(n), "--quick", "--deep", "--steps", "120"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "%s N=%d deep: 1 runs" % (family, n) in r.stdout and "wave-sim == oracle" in r.stdout and "wave_sim: 1 cases == oracle" in r.stdout, r.stdout
    assert "MISMATCH" not in r.stdout and "120 steps" in r.stdout
