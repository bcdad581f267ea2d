"""The pre-flop kernels' real bodies -- k_pfm_rank and k_pfm_count, and their readers k_pfm_prep, k_pfm_hero and k_pfm_rvr, the text of
pokerl_amd/csrc/pk_preflop.hip -- run on the CPU as workgroups of 256 lanes, the width they are compiled for (tools/host_sim/equity_sim.cpp -DPK_ES_ONLY=10 on wg_shim.h: every barrier a checked
rendezvous, LDS refilled with garbage before every workgroup, PK_IDX on every LDS subscript, on every key and on every matchup cell, the key
work space an allocation of exactly one chunk, outputs pre-filled).  No GPU.  Every one of the 2 x 1326 x 1326 outputs is compared with
tests/preflop_spec.py by exact equality (tools/host_sim/equity_cases.py preflop_cases(): nothing expected comes from a kernel).  The readers
run on a fixed pattern for a table, so that they are checked on their own."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "host_sim"))

import equity_cases as EC        # noqa: E402

CASES = [c for c in EC.preflop_cases() if c.quick]


@pytest.fixture(scope="module")
def equity_sim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ not found: the CPU build of the kernel bodies needs it")
    out = tmp_path_factory.mktemp("equity_sim_preflop")
    exe = str(out / "equity_sim_preflop")
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-DPK_HOST_SIM", "-I", os.path.join(ROOT, "tools", "host_sim", "stub"),
                        "-include", os.path.join(ROOT, "tools", "host_sim", "wg_shim.h"), "-DPK_ES_ONLY=10",
                        os.path.join(ROOT, "tools", "host_sim", "equity_sim.cpp"), "-o", exe], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe, str(out)


def test_the_cases_cover_what_the_kernels_can_get_wrong():
    assert all(c.family in ("preflop", "pfhero", "pfrvr") for c in EC.preflop_cases()) and len(CASES) >= 11
    others = {c.name for c in EC.all_cases()} | {c.name for c in EC.cluster_cases()} | {c.name for c in EC.hero_hist_cases()}
    assert not others & {c.name for c in EC.preflop_cases()}
    by = {c.name: c for c in CASES}
    num = lambda c, k: int(c.arrays[k][1][0])
    assert num(by["preflop-one-board-first"], "first") == 0 and num(by["preflop-one-board-last"], "first") == 2598959
    big = by["preflop-100-boards-chunk40"]
    first, n, chunk = num(big, "first"), num(big, "n"), num(big, "chunk")
    assert first % chunk and n % chunk and n > 2 * chunk and chunk % 32          # starts mid-chunk, several chunks, ragged chunk, ragged slice
    assert num(by["preflop-accumulate-33-boards"], "accumulate") == 1
    small = by["preflop-40-boards-chunk5"]                                       # a chunk below one staged run of boards: the key work space is 5 boards
    assert num(small, "chunk") < 32 < num(small, "n") and num(small, "accumulate") == 0
    # the readers: one workgroup for several spots, per-spot weights, a refused spot between good ones, status alone, the table form, two weight rows
    assert num(by["pfhero-grid1-five-spots"], "grid") == 1 and num(by["pfhero-grid1-five-spots"], "m") > 1
    assert num(by["pfhero-spot-weights-grid2"], "per_spot") == 1
    st = by["pfhero-no-weights-refused-between"].expected()["status"].tolist()
    assert st[0] == 0 and st[1] == 1 and st[3] == 0 and st[4] == 2
    assert by["pfhero-status-alone"].outputs == ("status",)
    tf = by["pfhero-table-form-observer-2"].expected()["status"].tolist()
    assert 16 in tf and 32 in tf and 0 in tf
    assert num(by["pfrvr-two-rows"], "m") == 2
    w = big.expected()
    assert w["win"].any() and w["tie"].any() and not w["win"].diagonal().any() and not w["tie"].diagonal().any()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_kernels_as_256_lane_workgroups_vs_spec(equity_sim, case):
    exe, work = equity_sim
    bad, sec, log = EC.run_case(exe, case, work, timeout=300)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: %s done" % case.family in log and "LDS bytes" in log
