"""The seat and serial arithmetic of a betting pass -- ActionRing::half_of (one bit-field extract at offset `serial << 4`) and Table<N>'s cyclic
seat walks (rotr / window_of on the seat mask twice over, wrap / unwrap by unsigned minimum, first_playing, scan, scan_first) of pk_device.hpp --
compiled for the CPU (tools/host_sim/seat_arith_sim.cpp on hip_shim.h) and held against the plain forms they replaced, exhaustively: half_of on
every 16-bit pattern in either half at both parities (2^17 cases, each under serials whose upper bits must drop out), the walks on every
(mask, active, current) at every seat count 2 .. 16.  Once as a plain build and once with -fsanitize=address,undefined (a stand-alone program).
No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": [], "asan_ubsan": ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


@pytest.mark.parametrize("build", list(BUILDS))
def test_seat_arithmetic_matches_the_plain_forms(tmp_path, build):
    if not shutil.which("g++"):
        pytest.fail("g++ not found: the CPU build of pk_device.hpp needs it")
    exe = str(tmp_path / "seat_arith_sim")
    r = subprocess.run(["g++", "-std=c++20", "-O1"] + BUILDS[build] + ["-DPK_HOST_SIM", "-include", os.path.join(ROOT, "tools", "host_sim", "hip_shim.h"),
                        os.path.join(ROOT, "tools", "host_sim", "seat_arith_sim.cpp"), "-o", exe], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    lines = r.stdout.split("\n")[:-1]
    assert lines[0] == "half_of: %d cases" % 2 ** 17 and lines[-1] == "seat_arith_sim: ok", lines
    assert lines[1:-1] == ["N=%d: %d cases" % (n, 2 ** n * n * n) for n in range(2, 17)], lines
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
