"""The hero histogram's real kernel bodies -- k_eqr_prep, k_hero_hist_counts, k_hero_hist, the text of pokerl_amd/csrc/pk_equity_range.hip and
pk_equity_hist_hero.hip -- run on the CPU as workgroups of 512 lanes, the width the kernel is compiled for (tools/host_sim/equity_sim.cpp
-DPK_ES_ONLY=9 on wg_shim.h: every collective a checked rendezvous, LDS refilled with garbage before every workgroup, PK_IDX on every LDS
subscript, every array an allocation of exactly its size, work arrays and outputs pre-filled).  No GPU.  Every output is compared with
tests/hero_hist_spec.py by exact equality (tools/host_sim/equity_cases.py hero_hist_cases(): nothing expected comes from a kernel).  The same
cases and the slower ones under ASan + UBSan and TSan: tools/host_sim/sanitize_equity.sh --only herohist."""
import math
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "host_sim"))

import equity_cases as EC        # noqa: E402

CASES = [c for c in EC.hero_hist_cases() if c.quick]


@pytest.fixture(scope="module")
def equity_sim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ not found: the CPU build of the kernel bodies needs it")
    out = tmp_path_factory.mktemp("equity_sim_herohist")
    exe = str(out / "equity_sim_herohist")
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-DPK_HOST_SIM", "-I", os.path.join(ROOT, "tools", "host_sim", "stub"),
                        "-include", os.path.join(ROOT, "tools", "host_sim", "wg_shim.h"), "-DPK_ES_ONLY=9",
                        os.path.join(ROOT, "tools", "host_sim", "equity_sim.cpp"), "-o", exe], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe, str(out)


def shapes(case):
    """[(nb, P after the hero)] of an explicit case, from its arrays."""
    hero, board, nboard, dead = (case.arrays[k][1] for k in ("hero", "board", "nboard", "dead"))
    return [(int(nb), 52 - 2 - int(nb) - bin(int(d)).count("1")) for nb, d in zip(nboard, dead)]


def test_the_cases_cover_what_the_kernel_can_get_wrong():
    names = {c.name for c in CASES}
    assert all(c.family == "herohist" for c in EC.hero_hist_cases()) and len(CASES) >= 9
    others = {c.name for c in EC.all_cases()} | {c.name for c in EC.cluster_cases()}
    assert not others & {c.name for c in EC.hero_hist_cases()}
    by = {c.name: c for c in CASES}
    bounds = by["herohist-bounds-grid1"]
    sets = [math.comb(p, 7 - nb) for nb, p in shapes(bounds)]
    assert int(bounds.arrays["grid"][1][0]) == 1 and len(sets) >= 2          # one workgroup, several spots: the counters are cleared
    assert 1 in sets and any(1 < s < 512 for s in sets) and any(s > 512 and s % 512 for s in sets)
    assert any(nb == 5 for nb, _ in shapes(bounds)) and by["herohist-river-alone"].expected()["completions"].tolist() == [1]
    two = by["herohist-two-spots-grid1"]
    assert int(two.arrays["grid"][1][0]) == 1 and len(shapes(two)) == 2 and not two.expected()["status"].any()
    assert int(by["herohist-grid1-spot-w"].arrays["per_spot"][1][0]) == 1                       # per-spot weights
    st = by["herohist-refused-between"].expected()["status"].tolist()
    assert st[0] == 0 and st[1] != 0 and st[2] == 0                          # a refused spot between good ones
    z = by["herohist-zero-weights"].expected()
    assert not z["hist"].any() and (z["void"] == z["completions"]).all() and z["completions"].all()
    bits = 0
    for s in by["herohist-status-bits"].expected()["status"].tolist():
        bits |= s
    assert bits == 1 | 2 | 8 | 64 | 128
    assert {"herohist-bins1", "herohist-table-form-observer-2"} <= names
    for c in CASES:
        w = c.expected()
        assert (w["hist"].sum(axis=-1) + w["void"] == w["completions"]).all(), c.name           # the invariant, in the expected values too


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_kernel_as_512_lane_workgroups_vs_spec(equity_sim, case):
    exe, work = equity_sim
    bad, sec, log = EC.run_case(exe, case, work, timeout=300)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: herohist done" in log and "LDS bytes" in log
