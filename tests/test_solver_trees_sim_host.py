"""The tree-per-spot solver kernels' real bodies -- k_rs_prep / k_ts_prep, k_trees_prep and k_trees_river_solve / k_trees_turn_solve, the text
of pokerl_amd/csrc/pk_river_solver.hip and pk_turn_solver.hip -- run on the CPU as workgroups of 8 x 64 lanes (tools/host_sim/equity_sim.cpp
-DPK_ES_ONLY=14 / 15 on wg_shim.h: every collective a checked rendezvous, LDS refilled with garbage before every workgroup, PK_IDX on every
LDS and work-space subscript, every array -- the packed trees too -- an allocation of exactly its size, work arrays and outputs pre-filled).
No GPU.  Every case runs at a grid of 1, so that ONE workgroup takes the spots in turn and a stale tree, stale regrets or stale LDS of the
spot before would show.  Every output is compared byte for byte with the numpy specs run one spot at a time with that spot's tree
(tests/solver_trees_util.py): nothing expected comes from a kernel.  The same cases under ASan + UBSan and TSan:
tools/host_sim/sanitize_equity.sh --only trees."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "host_sim"))

import equity_cases as EC        # noqa: E402

RIVER = [c for c in EC.river_trees_cases() if c.quick]
TURN = [c for c in EC.turn_trees_cases() if c.quick]
BAD_TREE = 32


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
    return build(tmp_path_factory, 14, "rtrees")


@pytest.fixture(scope="module")
def turn_sim(tmp_path_factory):
    return build(tmp_path_factory, 15, "ttrees")


def field(case, key):
    return np.asarray(case.arrays[key][1])


@pytest.mark.parametrize("cases, family, prefix, key, own", [(RIVER, "rivertrees", "rtrees-", "strategy", 4), (TURN, "turntrees", "ttrees-", "river_strategy", 2)])
def test_the_cases_cover_what_a_tree_per_spot_can_get_wrong(cases, family, prefix, key, own):
    by = {c.name: c for c in cases}
    assert all(c.family == family and c.name.startswith(prefix) and int(field(c, "grid")[0]) == 1 for c in cases) and len(cases) >= 6
    others = {c.name for c in EC.all_cases()} | {c.name for c in EC.river_cases()} | {c.name for c in EC.turn_cases()}
    assert not others & set(by)                                               # not part of all_cases(), no name taken twice
    mixed = by[prefix + "big-after-small-and-back"]
    n, of = field(mixed, "n"), field(mixed, "tree_of")
    steps = [int(n[b]) - int(n[a]) for a, b in zip(of[:-1], of[1:])]
    assert max(steps) > 0 and min(steps) < 0                                  # a larger tree after a smaller one, and the reverse
    bad = by[prefix + "refused-and-bad-tree-between"]
    st, of, K = bad.expected()["status"].tolist(), field(bad, "tree_of").tolist(), int(field(bad, "ntrees")[0])
    assert st[0] == 0 and st[1] not in (0, BAD_TREE) and of[2] == K and st[2] == BAD_TREE and st[3] == 0 and of[4] == 0xFFFFFFFF and st[4] == BAD_TREE
    assert len(st) == 6 and st[5] == 0                                        # a valid spot follows the refused ones
    rep = by[prefix + "one-tree-repeated"]
    assert int(field(rep, "ntrees")[0]) == 1 and not field(rep, "tree_of").any() and len(field(rep, "tree_of")) == 3
    stride = next(c for c in cases if "unreferenced" in c.name)
    used = set(field(stride, "tree_of").tolist())
    n = field(stride, "n")
    assert int(np.argmax(n)) not in used                                      # the largest tree is named by no spot, and still sets the strides
    want = stride.expected()[key]                                             # `own`: the most rows of a tree that a spot names
    assert want.shape[1] > own and not want[:, own:].any() and want[:, own - 1].any()


@pytest.mark.parametrize("case", RIVER, ids=[c.name for c in RIVER])
def test_river_kernel_as_512_lane_workgroups_vs_spec(river_sim, case):
    exe, work = river_sim
    bad, sec, log = EC.run_case(exe, case, work, timeout=300)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: rivertrees done" in log and "LDS bytes" in log


@pytest.mark.parametrize("case", TURN, ids=[c.name for c in TURN])
def test_turn_kernel_as_512_lane_workgroups_vs_spec(turn_sim, case):
    exe, work = turn_sim
    bad, sec, log = EC.run_case(exe, case, work, timeout=300)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: turntrees done" in log and "LDS bytes" in log
