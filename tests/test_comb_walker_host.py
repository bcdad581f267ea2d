"""The combination walker of the equity kernels (pk::Comb, pokerl_amd/csrc/pk_equity_common.hpp: the one unranking loop and the one carry
ladder k_equity<N>, k_ev<N>, k_eqr and k_hero_hist step their boards and card sets with) against a plain enumeration, on the CPU:
tools/host_sim/comb_selftest.cpp, a stand-alone program on the host-sim stub, built with g++ and run directly -- once plain, once under
ASan + UBSan.  No GPU.  Both forms the kernels instantiate, <5, 0> and <4, 2>, with every number of frozen levels f they use (0 .. 5,
0 .. 2) and pools of n .. n + 4 cards (n = L - f live levels: the walk's ends and a carry at every depth) and of 47 (a full-pool flop):
start(rank) is the rank-th subset in lexicographic order for every rank, next() from rank 0 visits all C(P, n) of them in order and
calls its callable exactly when a level above the last one changed, and past the last subset the state is 62 / 63 at the last two levels --
indices of the pool's 64 LDS slots still.  54 cases, 1 926 001 subsets; 0.2 s plain, 0.5 s sanitized, 3 s for the two builds."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("build,flags", [("plain", []), ("asan-ubsan", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])])
def test_walker_vs_plain_enumeration(tmp_path, build, flags):
    if not shutil.which("g++"):
        pytest.fail("g++ not found: the CPU build of the walker needs it")
    exe = str(tmp_path / "comb_selftest")
    subprocess.run(["g++", "-std=c++20", "-O1", "-DPK_HOST_SIM", "-I", os.path.join(ROOT, "tools", "host_sim", "stub"), "-include",
                    os.path.join(ROOT, "tools", "host_sim", "wg_shim.h")] + flags + [os.path.join(ROOT, "tools", "host_sim", "comb_selftest.cpp"), "-o", exe],
                   check=True, cwd=ROOT)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    print(r.stdout[-500:], r.stderr[-3000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "comb_selftest: 54 cases, 1926001 subsets, 0 failed checks" in r.stdout
