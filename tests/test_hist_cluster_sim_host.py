"""The histogram clustering's real kernel bodies -- k_cl_quant, k_cl_pack, k_cl_assign<P>, k_cl_update<LDS>, k_cl_finalise, k_cl_seed_dist<P>,
k_cl_seed_pick, the text of pokerl_amd/csrc/pk_hist_cluster.hip -- run on the CPU as workgroups of 4 waves x 64 lanes
(tools/host_sim/equity_sim.cpp -DPK_ES_ONLY=8 on wg_shim.h: every collective a checked rendezvous, LDS refilled with garbage before every
workgroup, PK_IDX on every LDS subscript, every array an allocation of exactly its size, work arrays and outputs pre-filled), queued in the
order of pk::cl_seed_launch / cl_assign_launch / cl_cluster_launch.  No GPU.  Every output is compared with tests/hist_cluster_spec.py by
exact equality (tools/host_sim/equity_cases.py cluster_cases(): nothing expected comes from a kernel).  The same cases under ASan + UBSan and
TSan: tools/host_sim/sanitize_equity.sh --only cluster."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "host_sim"))

import equity_cases as EC        # noqa: E402
import hist_cluster_spec as CS   # noqa: E402

CASES = [c for c in EC.cluster_cases() if c.quick]


@pytest.fixture(scope="module")
def equity_sim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ not found: the CPU build of the kernel bodies needs it")
    out = tmp_path_factory.mktemp("equity_sim_cluster")
    exe = str(out / "equity_sim_cluster")
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-DPK_HOST_SIM", "-I", os.path.join(ROOT, "tools", "host_sim", "stub"),
                        "-include", os.path.join(ROOT, "tools", "host_sim", "wg_shim.h"), "-DPK_ES_ONLY=8",
                        os.path.join(ROOT, "tools", "host_sim", "equity_sim.cpp"), "-o", exe], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe, str(out)


def test_the_cases_cover_what_the_kernels_can_get_wrong():
    names = {c.name for c in CASES}
    assert all(c.family == "cluster" for c in CASES) and len(CASES) >= 12
    assert not {c.name for c in EC.all_cases()} & {c.name for c in EC.cluster_cases()}
    assert {"cluster-assign-b%d" % b for b in (1, 2, 7, 10, 32)} <= names and {"cluster-iterate-b7", "cluster-iterate-b32"} <= names
    assert {"cluster-iterate-global-sums", "cluster-ties-assign", "cluster-ties-iterate", "cluster-seed-K33-chunk256", "cluster-seed-identical-rows"} <= names
    for b in (1, 2, 7, 10, 32):                                      # a grid of 1 over more rows than a workgroup has lanes; an empty wave
        c = next(c for c in CASES if c.name == "cluster-assign-b%d" % b)
        assert int(c.arrays["grid"][1][0]) == 1 and int(c.arrays["n"][1][0]) > 256
        want = c.expected()
        assert (want["label"][64:128] == CS.NONE).all() and len(set(want["label"].tolist())) >= (4 if b >= 7 else 2)   # (one bin: every row is one point)
    assert {"cluster-assign-n%d-K%d" % (n, K) for n in (1, 63) for K in (2, 3, 70)} <= names    # more centroids than rows: assign takes any K
    assert any(int(c.arrays["skew"][1][0]) % 8 for c in CASES)       # an array that is not 16-byte aligned
    ties = next(c for c in CASES if c.name == "cluster-ties-assign").expected()
    assert set(ties["label"].tolist()) == {0, 1, CS.NONE}            # centroid 2 equals centroid 1 and never wins; the midway rows go to the smaller index
    it = next(c for c in CASES if c.name == "cluster-ties-iterate").expected()
    assert it["centroids_out"][2].tolist() == [0, 0, 0, 65535] and it["changed"][1] > 0   # empty in the first iteration: kept; it wins rows once centroid 1 has moved
    same = next(c for c in CASES if c.name == "cluster-seed-identical-rows").expected()["centroids"]
    assert (same == same[0]).all() and same[0, -1] == 65535          # W = 0 from the second round on
    glob = next(c for c in CASES if c.name == "cluster-iterate-global-sums")
    assert int(glob.arrays["lds"][1][0]) == 0 and glob.expected()["changed"][1] > 0


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_kernels_as_4_wave_workgroups_vs_spec(equity_sim, case):
    exe, work = equity_sim
    bad, sec, log = EC.run_case(exe, case, work, timeout=300)
    print("%s: %.2f s in the driver" % (case.name, sec))
    assert not bad, (bad, log[-3000:])
    assert "equity_sim: cluster done" in log and "LDS bytes" in log
