"""The re-solving kernels' real bodies -- k_rs_prep / k_ts_prep, k_trees_prep, k_resolve_prep and k_resolve_river_solve /
k_resolve_turn_solve, the text of pokerl_amd/csrc/pk_river_solver.hip and pk_turn_solver.hip -- run on the CPU as workgroups of 8 x 64
lanes (tools/host_sim/equity_sim.cpp -DPK_ES_ONLY=18 / 19 on wg_shim.h: every collective a checked rendezvous, LDS refilled with garbage
before every workgroup, PK_IDX on every LDS and work-space subscript, every array -- reach, given, at, at_card and the node outputs too --
an allocation of exactly its size, work arrays and outputs pre-filled).  No GPU.  Every case runs at a grid of 1, so that ONE workgroup
takes the spots in turn and stale node outputs, stale given values or stale LDS of the spot before would show.  Every output is compared
byte for byte with tests/resolve_spec.py: nothing expected comes from a kernel.  What the definition says is not read holds ones in every
case.  The same cases, and the P = 48 fixture, under ASan + UBSan and TSan: tools/host_sim/sanitize_equity.sh --only res-."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "host_sim"))

import equity_cases as EC        # noqa: E402
import resolve_spec as RZ        # noqa: E402

RIVER = [c for c in EC.river_resolve_cases() if c.quick]
TURN = [c for c in EC.turn_resolve_cases() if c.quick]


def build(tmp_path_factory, only, tag):
    if not shutil.which("g++"):
        pytest.fail("g++ not found: the CPU build of the kernel bodies needs it")
    out = tmp_path_factory.mktemp("equity_sim_" + tag)
    exe = str(out / ("equity_sim_" + tag))
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-DPK_HOST_SIM", "-I", os.path.join(ROOT, "tools", "host_sim", "stub"),
                        "-include", os.path.join(ROOT, "tools", "host_sim", "wg_shim.h"), "-DPK_ES_ONLY=%d" % only,
                        os.path.join(ROOT, "tools", "host_sim", "equity_sim.cpp"), "-o", exe], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe, str(out)


@pytest.fixture(scope="module")
def river_sim(tmp_path_factory):
    return build(tmp_path_factory, 18, "rres")


@pytest.fixture(scope="module")
def turn_sim(tmp_path_factory):
    return build(tmp_path_factory, 19, "tres")


def field(case, key):
    return np.asarray(case.arrays[key][1])


@pytest.mark.parametrize("cases, family, prefix, limit", [(RIVER, "riverresolve", "rres-", RZ.RIVER_LIM), (TURN, "turnresolve", "tres-", RZ.TURN_LIM)])
def test_the_cases_cover_what_a_resolve_can_get_wrong(cases, family, prefix, limit):
    by = {c.name: c for c in cases}
    assert all(c.family == family and c.name.startswith(prefix) and int(field(c, "grid")[0]) == 1 for c in cases) and len(cases) >= 8
    others = {c.name for c in EC.all_cases()} | {c.name for c in EC.river_lock_cases()} | {c.name for c in EC.turn_lock_cases()}
    assert not others & set(by)                                               # not part of all_cases(), no name taken twice
    bad = by[prefix + ("refused-bad-at-between" if family == "riverresolve" else "refused-bad-at-bad-card-between")]
    st = bad.expected()["status"].tolist()
    refused = [i for i, s in enumerate(st) if s]
    assert st[0] == 0 and st[-1] == 0 and 32 in st and any(s not in (0, 32) for s in st) and (field(bad, "reach")[refused] == 0xFFFFFFFF).all()
    assert all(not bad.expected()[k][refused].any() for k in ("node_reach", "node_value", "node_br", "value"))
    if family == "turnresolve":
        assert st.count(RZ.BAD_CARD) == 2                                     # no card at all, and a card of the board
        cards = by[prefix + "river-at-first-and-last-card"]
        assert cards.expected()["node_value"][:2].any(axis=(1, 2)).all() and len(set(field(cards, "at_card")[:2].tolist())) == 2
    else:
        seq = by[prefix + "at-after-no-given-and-back"]                       # given node, none, given node, ... in one workgroup
        has = [RZ.GIVEN in field(seq, "kind")[int(k)].tolist() for k in field(seq, "tree_of")]
        assert has == [False, True, False, True, False]
        beyond = field(by[prefix + "given-beyond-the-clamp"], "given").view(np.int64)
        assert (beyond > RZ.GIVEN_LIM).any() and (beyond < -RZ.GIVEN_LIM).any() and (beyond == np.iinfo(np.int64).min).any()
    ends = by[prefix + "at-root-leaf-last"]
    at, n = field(ends, "at"), int(field(ends, "n")[0])
    assert at[0] == 0 and at[2] == n - 1 and int(field(ends, "kind")[0][at[1]]) in (2, 3, 4)
    over = field(by[prefix + "reach-above-the-limit"], "reach")
    assert (over == limit + 1).any() and ((over > limit) & (over != 0xFFFFFFFF)).any()
    big = by[prefix + "large-after-small"]
    n, of = field(big, "n"), field(big, "tree_of")
    assert int(n[of[1]]) > int(n[of[0]])
    assert by[prefix + "ranges-no-reach-no-at"].arrays["reach"][1] is None and by[prefix + "ranges-no-reach-no-at"].arrays["at"][1] is None
    assert int(field(by[prefix + "iters0-all-locked"], "iters")[0]) == 0


@pytest.mark.parametrize("case", RIVER, ids=[c.name for c in RIVER])
def test_river_kernel_as_512_lane_workgroups_vs_spec(river_sim, case):
    exe, work = river_sim
    bad, sec, log = EC.run_case(exe, case, work, timeout=300)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: riverresolve done" in log and "LDS bytes" in log


@pytest.mark.parametrize("case", TURN, ids=[c.name for c in TURN])
def test_turn_kernel_as_512_lane_workgroups_vs_spec(turn_sim, case):
    exe, work = turn_sim
    bad, sec, log = EC.run_case(exe, case, work, timeout=300)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: turnresolve done" in log and "LDS bytes" in log
