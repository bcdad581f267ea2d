"""The table kernels' real body (rollout_body of pk_table_kernels.hpp) run 64 lanes wide on the CPU -- tools/host_sim/wave_sim.cpp on
wave_shim.h: one thread per lane, every ballot / readlane / shuffle / barrier a checked rendezvous, LDS a garbage-filled heap object of
exactly sizeof(LDS), index checks on the evaluator's table and the showdown queue -- against the oracle.  No GPU.  The full matrix
(every family, seat counts up to 16, under ASan + UBSan and TSan) is tools/host_sim/sanitize_wave.sh; here a plain g++ build of three
instantiations, one small configuration each: k_rollout_tab<6> (split, deferring launches), k_rollout_allin_tab<9> (equal stacks:
every seat of every lane in the showdown, two hands per lane, the dummy slot) and k_step<6> (the lone-table paths)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def wave_sim(tmp_path_factory):
    if not shutil.which("g++") or not shutil.which("gcc"):
        pytest.fail("g++ / gcc not found: the CPU build of the kernel bodies needs them")
    out = tmp_path_factory.mktemp("wave_sim")
    obj, exe = str(out / "oracle.o"), str(out / "wave_sim")
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-c", os.path.join(ROOT, "oracle", "pokerl_oracle.c"), "-o", obj], check=True, cwd=ROOT)
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-pthread", "-ffp-contract=off", "-DPK_HOST_SIM", "-include", os.path.join(ROOT, "tools", "host_sim", "wave_shim.h"),
                        "-DPK_WS_PART=100", "-DPK_WS_MAIN", os.path.join(ROOT, "tools", "host_sim", "wave_sim.cpp"), obj, "-o", exe],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("family,n", [("tab", 6), ("allin_tab", 9), ("step", 6)])
def test_kernel_body_64_lanes_wide_vs_oracle(wave_sim, family, n):
    r = subprocess.run([wave_sim, family, str(n), "--quick"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "%s N=%d: 1 runs" % (family, n) in r.stdout and "wave-sim == oracle" in r.stdout and "wave_sim: 1 cases == oracle" in r.stdout, r.stdout
    assert "MISMATCH" not in r.stdout
