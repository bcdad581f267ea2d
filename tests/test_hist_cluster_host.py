"""CPU tests of the histogram clustering (no GPU): the properties of the numpy restatement tests/hist_cluster_spec.py (the last bin, monotone
centroids, the derived bound against histogram_emd, the fixed point), the seeding draw against oracle/rng_spec.py on a hand-computed case and
its W = 0 rule, the tie rule on constructed ties, the six entry points in the header, the binding and the library, the new kernels in the
built library's code objects, and the argument checks that happen before any device call.  Every comparison is exact unless it says so."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import hist_cluster_spec as CS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import rng_spec as R  # noqa: E402

ENTRY_POINTS = ("pk_hist_cluster_seed_d", "pk_hist_cluster_assign_d", "pk_hist_cluster_d", "pk_hist_cluster_seed", "pk_hist_cluster_assign",
                "pk_hist_cluster")


@pytest.fixture(scope="module")
def lib():
    from pokerl_amd import _lib, build
    build.build_lib()
    return _lib


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(0x434C5330)
    hist = CS.latent_rows(rng, 3001, 10)
    q, empty = CS.quant(hist)
    return hist, q, empty


def test_quantised_cdf_ends_in_65535_and_empty_rows_are_zero(data):
    hist, q, empty = data
    assert q.dtype == np.uint16 and 100 < empty.sum() < 600
    assert (q[~empty, -1] == 65535).all() and not q[empty].any() and (np.diff(q.astype(np.int64), axis=1) >= 0).all()
    # the largest product of the definition needs 38 bits: the device divides in 64
    big = np.full((1, 32), 65535, np.uint16)
    assert 65535 * int(big.sum()) > 2 ** 36 and CS.quant(big)[0][0].tolist() == [65535 * (b + 1) // 32 for b in range(32)]
    one = np.zeros((1, 5), np.uint16)
    one[0, 3] = 1
    assert CS.quant(one)[0][0].tolist() == [0, 0, 0, 65535, 65535]


def test_seed_centroids_are_rows_and_the_distance_is_the_emd_within_the_derived_bound(data):
    from pokerl_amd import judger as J
    hist, q, empty = data
    C, rows = CS.seed(q, empty, 12, R.DEFAULT_SEED, 3)
    assert len(set(rows)) == 12 and not empty[rows].any() and np.array_equal(C, q[rows])
    d = CS.distances(q[~empty], C)
    emd = J.histogram_emd(hist[~empty][:, None, :], hist[rows][None, :, :])
    assert np.abs(d / 65535.0 - emd).max() < 10 / 65535.0            # |d / 65535 - histogram_emd| < nbins / 65535: each floor is off by less than 1
    assert np.abs(d / 65535.0 - emd).max() > 0                       # (and the quantisation is there to be seen)


def test_centroids_stay_cdfs_and_a_fixed_point_stays_fixed(data):
    hist, q, empty = data
    C0, _ = CS.seed(q, empty, 8, 5)
    r = CS.iterate(q, empty, C0, 40)
    C = r["centroids"]
    assert (C[:, -1] == 65535).all() and (np.diff(C.astype(np.int64), axis=1) >= 0).all()
    assert r["changed"][0] == (~empty).sum() and (r["labels"][empty] == CS.NONE).all() and not r["dist"][empty].any()
    assert int(r["dist"].sum(dtype=np.uint64)) == int(r["inertia"][-1])
    still = np.flatnonzero(r["changed"] == 0)
    assert still.size, r["changed"]                                  # this data settles within 40 iterations
    t = int(still[0])
    assert not r["changed"][t:].any() and len(set(r["inertia"][t:].tolist())) == 1
    again = CS.iterate(q, empty, C, 1)                               # one more iteration from the result: nothing moves
    assert again["changed"][0] == (~empty).sum()                     # (a call's first iteration counts every non-empty row)
    assert np.array_equal(again["centroids"], C) and np.array_equal(again["labels"], r["labels"]) and np.array_equal(again["dist"], r["dist"])
    short = CS.iterate(q, empty, C0, t + 1)                          # stopping at the fixed point gives the same result
    assert np.array_equal(short["centroids"], C) and np.array_equal(short["labels"], r["labels"])


def test_seeding_draw_on_three_rows_by_hand():
    hist = np.array([[1, 0], [0, 0], [0, 1], [1, 1]], np.uint16)     # q: (65535, 65535), empty, (0, 65535), (32767, 65535)
    q, empty = CS.quant(hist)
    assert q.tolist() == [[65535, 65535], [0, 0], [0, 65535], [32767, 65535]] and empty.tolist() == [False, True, False, False]
    live = [0, 2, 3]
    seen = set()
    for nonce in range(12):
        key = R.seed_key(R.DEFAULT_SEED)
        x0, x1 = ((w[0] | (w[1] << 32)) for w in (R.philox4x32_10((j, 0, 0x434C5330, nonce), key) for j in range(2)))
        first = live[(x0 * 3) >> 64]                                 # round 0: weight 1 per non-empty row, the empty one has no share
        d = {0: {2: 65535, 3: 32768}, 2: {0: 65535, 3: 32767}, 3: {0: 32768, 2: 32767}}[first]
        others = sorted(d)
        r = (x1 * (d[others[0]] + d[others[1]])) >> 64
        second = others[0] if r < d[others[0]] else others[1]        # the smallest i whose inclusive prefix sum exceeds r
        third = [i for i in live if i not in (first, second)][0]     # one row is left with a weight: whatever r is, it is chosen
        C, rows = CS.seed(q, empty, 3, R.DEFAULT_SEED, nonce)
        assert rows == [first, second, third] and np.array_equal(C, q[rows]), nonce
        assert CS.draw(R.DEFAULT_SEED, nonce, 0, 3) == (x0 * 3) >> 64
        seen.add(tuple(rows))
    assert len(seen) >= 3                                            # the nonce moves the draw
    assert CS.pick([0, 5, 0, 2], 0) == 1 and CS.pick([0, 5, 0, 2], 4) == 1 and CS.pick([0, 5, 0, 2], 5) == 3 and CS.pick([3], 2) == 0


def test_seeding_with_no_weight_left_takes_the_lowest_non_empty_row():
    hist = np.zeros((9, 4), np.uint16)
    hist[2:] = [1, 2, 0, 1]
    hist[5] = 0
    q, empty = CS.quant(hist)
    C, rows = CS.seed(q, empty, 4, 99, 1)
    assert rows[0] in (2, 3, 4, 6, 7, 8) and rows[1:] == [2, 2, 2] and (C == q[2]).all()
    r = CS.iterate(q, empty, C, 2)                                   # identical centroids: cluster 0 takes every row, the others stay empty and keep theirs
    assert set(r["labels"][~empty].tolist()) == {0} and np.array_equal(r["centroids"], C) and not r["dist"].any()
    with pytest.raises(ValueError):
        CS.seed(*CS.quant(np.zeros((3, 4), np.uint16)), 1, 0)


def test_ties_go_to_the_smallest_centroid():
    q = np.array([[32767, 65535], [32768, 65535], [10, 65535], [10, 65535]], np.uint16)
    empty = np.zeros(4, bool)
    C = np.array([[65535, 65535], [0, 65535], [0, 65535], [65534, 65535]], np.uint16)
    label, dist = CS.assign(q, empty, C)
    # 32767 lies 32767 from 0 (centroids 1 and 2 are equal: the smaller index); 32768 lies 32767 from 65535 and 32766 from 65534
    assert label.tolist() == [1, 3, 1, 1] and dist.tolist() == [32767, 32766, 10, 10]
    mid = np.array([[30000, 65535]], np.uint16)
    label, dist = CS.assign(mid, np.zeros(1, bool), np.array([[40000, 65535], [20000, 65535], [40000, 65535]], np.uint16))
    assert label.tolist() == [0] and dist.tolist() == [10000]        # exactly midway: the smaller index
    label, _ = CS.assign(mid, np.zeros(1, bool), np.array([[20000, 65535], [40000, 65535]], np.uint16))
    assert label.tolist() == [0]
    C2, counts = CS.update(q, np.array([1, 0, 1, 1], np.uint16), C)
    assert counts.tolist() == [1, 3, 0, 0] and C2[2].tolist() == C[2].tolist() and C2[3].tolist() == C[3].tolist()   # empty clusters keep their centroid
    assert C2[0].tolist() == [32768, 65535] and C2[1].tolist() == [(32767 + 10 + 10 + 1) // 3, 65535]               # floor((S + floor(n / 2)) / n)


def test_header_declares_and_binding_lists_the_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "pokerl_hip.h")).read()
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in lib.SYMBOLS and hasattr(L, name), name
        assert getattr(lib.lib(), name).argtypes is not None, name
    assert re.search(r"#define PK_CL_MAX_K 4096\b", header) and re.search(r"#define PK_CL_NONE 0xFFFFu", header)
    assert (lib.CL_MAX_K, lib.CL_NONE, lib.CL_MAX_ITERS) == (CS.MAX_K, CS.NONE, CS.MAX_ITERS) == (4096, 0xFFFF, 1024)
    assert "0x434C5330" in header and "smallest i whose inclusive prefix sum of w exceeds r" in header
    assert lib.lib().pk_abi_version() == 6


def test_cluster_kernels_exist_without_scratch(lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = {k: d for k, d in kernel_meta.kernels(lib.LIB_PATH).items() if k.startswith("k_cl_")}
    want = ["k_cl_assign<%d>" % p for p in range(1, 17)] + ["k_cl_seed_dist<%d>" % p for p in range(1, 17)]
    want += ["k_cl_quant", "k_cl_pack", "k_cl_finalise", "k_cl_seed_pick", "k_cl_update<true>", "k_cl_update<false>"]
    assert sorted(ks) == sorted(want), sorted(ks)
    assert all(d["private_segment"] == 0 and d["vgpr_spill"] == 0 and d["sgpr_spill"] == 0 for d in ks.values()), ks
    assert all(ks["k_cl_assign<%d>" % p]["vgprs"] + ks["k_cl_assign<%d>" % p]["agprs"] <= 64 for p in range(1, 17))   # eight waves per SIMD
    assert ks["k_cl_update<true>"]["lds"] == 4096 * 12 and ks["k_cl_quant"]["lds"] == 16384


def test_argument_errors_are_refused_before_any_device_call(lib):
    L = lib.lib()
    one = np.ones(64, np.uint16)
    p = lib.ptr(one)
    bad = lib.PK_E_INVALID_ARG
    for nbins in (0, 33, -1):
        assert L.pk_hist_cluster_seed_d(0, 2, nbins, p, 1, 1, 0, p, None) == bad and b"nbins" in L.pk_last_error(None)
        assert L.pk_hist_cluster_assign_d(0, 2, nbins, p, 1, p, p, None, None) == bad
        assert L.pk_hist_cluster_d(0, 2, nbins, p, 1, p, 1, p, None, None, None, None) == bad
        assert L.pk_hist_cluster_seed(0, 2, nbins, p, 1, 1, 0, p) == bad
        assert L.pk_hist_cluster_assign(0, 2, nbins, p, 1, p, p, None) == bad
        assert L.pk_hist_cluster(0, 2, nbins, p, 1, p, 1, p, None, None, None) == bad
    for K in (0, 4097, -1, 3):                                       # (3 > n = 2: seeding and clustering take their centroids from rows)
        assert L.pk_hist_cluster_seed_d(0, 2, 4, p, K, 1, 0, p, None) == bad and b"K" in L.pk_last_error(None), K
        assert L.pk_hist_cluster_d(0, 2, 4, p, K, p, 1, p, None, None, None, None) == bad, K
        assert L.pk_hist_cluster_seed(0, 2, 4, p, K, 1, 0, p) == bad, K
        assert L.pk_hist_cluster(0, 2, 4, p, K, p, 1, p, None, None, None) == bad, K
    for K in (0, 4097, -1):
        assert L.pk_hist_cluster_assign(0, 2, 4, p, K, p, p, None) == bad and L.pk_hist_cluster_assign_d(0, 2, 4, p, K, p, p, None, None) == bad, K
    lab = np.zeros(2, np.uint16)                                     # assign labels any number of rows with any K: K > n is no argument error
    assert L.pk_hist_cluster_assign(0, 2, 4, p, 3, p, lib.ptr(lab), None) != bad
    assert L.pk_hist_cluster_assign(0, 1, 4, p, 16, p, lib.ptr(lab), None) != bad
    for n in (0, 2 ** 31):
        assert L.pk_hist_cluster_seed_d(0, n, 4, p, 1, 1, 0, p, None) == bad and b"pk_hist_cluster_seed_d" in L.pk_last_error(None)
        assert L.pk_hist_cluster_d(0, n, 4, p, 1, p, 1, p, None, None, None, None) == bad
    for iters in (0, 1025, -1):
        assert L.pk_hist_cluster_d(0, 2, 4, p, 1, p, iters, p, None, None, None, None) == bad and b"iters" in L.pk_last_error(None)
        assert L.pk_hist_cluster(0, 2, 4, p, 1, p, iters, p, None, None, None) == bad
    assert L.pk_hist_cluster_seed(0, 2, 4, None, 1, 1, 0, p) == bad and L.pk_hist_cluster_assign_d(0, 2, 4, p, 1, p, None, None, None) == bad
    zeros = np.zeros(64, np.uint16)                                  # the host forms see the rows: K non-empty ones are needed
    assert L.pk_hist_cluster_seed(0, 4, 4, lib.ptr(zeros), 1, 1, 0, p) == bad and b"non-empty" in L.pk_last_error(None)
    half = zeros.copy()
    half[:4] = 1
    assert L.pk_hist_cluster(0, 4, 4, lib.ptr(half), 2, p, 1, p, None, None, None) == bad and b"non-empty" in L.pk_last_error(None)
    assert (one == 1).all()                                          # nothing was written


def test_python_helpers_validate_before_any_device_call(lib):
    import pokerl_amd as P
    from pokerl_amd import judger as J
    for name in ("HistogramClusters", "cluster_histograms", "assign_histograms", "seed_histogram_centroids", "cluster_histograms_d", "assign_histograms_d"):
        assert getattr(P, name) is getattr(J, name) and name in P.__all__, name
    assert hasattr(P.StrengthHistogram, "cluster") and J.CL_NONE == 0xFFFF
    hist = np.ones((6, 4), np.uint16)
    for k in (0, 4097, -1, 2.5, "3", None, True, 7):                 # (7 > the six non-empty rows)
        with pytest.raises(ValueError, match="k"):
            J.cluster_histograms(hist, k)
        with pytest.raises(ValueError, match="k"):
            J.seed_histogram_centroids(hist, k)
    for iters in (0, 1025, 2.0, None):
        with pytest.raises(ValueError, match="iters"):
            J.cluster_histograms(hist, 2, iters=iters)
    with pytest.raises(ValueError, match="nonce"):
        J.cluster_histograms(hist, 2, nonce=2 ** 32)
    with pytest.raises(ValueError, match="seed"):
        J.seed_histogram_centroids(hist, 2, seed=-1)
    for bad in (np.ones(4, np.uint16), np.ones((3, 33), np.uint16), np.ones((3, 4)), np.full((3, 4), 65536), np.full((3, 4), -1), np.ones((0, 4), np.uint16)):
        with pytest.raises(ValueError, match="hist"):
            J.cluster_histograms(bad, 1)
        with pytest.raises(ValueError, match="hist"):
            J.assign_histograms(bad, np.ones((1, 4), np.uint16))
    zero = np.zeros((5, 4), np.uint16)
    with pytest.raises(ValueError, match="non-empty"):
        J.cluster_histograms(zero, 1)
    for init in (np.ones((3, 4), np.uint16), np.ones((2, 5), np.uint16), np.ones((2, 4)), np.full((2, 4), 70000)):
        with pytest.raises(ValueError, match="init"):
            J.cluster_histograms(hist, 2, init=init)
    with pytest.raises(ValueError, match="centroids"):
        J.assign_histograms(hist, np.ones((2, 5), np.uint16))
    with pytest.raises(ValueError, match="centroids"):
        J.assign_histograms(hist, np.ones((4097, 4), np.uint16))
    for bins in (0, 33, None):
        with pytest.raises(ValueError, match="bins"):
            J.cluster_histograms_d(4, bins, 0, 1, 0, 1, 0)
        with pytest.raises(ValueError, match="bins"):
            J.assign_histograms_d(4, bins, 0, 1, 0, 0)
    with pytest.raises(ValueError, match="iters"):
        J.cluster_histograms_d(4, 4, 0, 1, 0, 0, 0)
    r = J.HistogramClusters(np.full((3, 4), 65535, np.uint16), np.zeros((2, 5), np.uint16), np.full((2, 5), 65535, np.uint32), np.array([9, 7], np.uint64),
                            np.array([10], np.uint32))
    assert (r.k, r.bins) == (3, 4) and r.emd.dtype == np.float64 and (r.emd == 1.0).all() and "k=3" in repr(r)
