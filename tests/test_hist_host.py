"""CPU tests of the strength histograms (no GPU): the numpy restatement of the definition against the fixture computed by the reference's own
eval_hand / compare_rankings, the row-sum invariant, the river decomposition (a spot's histogram = the sum over its completions of the
one-hot bins of the range-vs-range rows of the completed river boards), the bin rule at its edges, the status bits, the new entry points in
the header and the binding, the new kernels in the built library's code objects, and the Python helpers.  Every comparison is exact."""
import json
import math
import os
import re
import sys

import numpy as np
import pytest

import hist_spec as HS
import rvr_spec as VS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pk_equity_hist_d", "pk_equity_hist", "pk_table_equity_hist_d", "pk_table_equity_hist")
H = HS.HOLDINGS
CASES = ("ones", "random", "dying")


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "hist_ref.json")) as f:
        ref = json.load(f)
    assert ref["holdings"] == H and len(ref["weights"]) == H
    return ref


@pytest.fixture(scope="module")
def lib():
    from pokerl_amd import _lib, build
    build.build_lib()
    return _lib


def test_fixture_covers_what_it_must():
    ref = fixture()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "hist_ref.json")) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "rvr_ref.json"))
    assert ref["bins"] == [1, 2, 7, 32]
    w = ref["weights"]
    assert 0 in w and 65535 in w and max(w) <= 65535 and min(w) >= 0
    shape = [(len(s["board"]), s["pool"]) for s in ref["spots"]]
    assert (5, 4) in shape and (4, 5) in shape and (3, 6) in shape                        # the smallest pools: P = k + 4
    assert (5, 10) in shape and (4, 9) in shape and (3, 10) in shape
    for s in ref["spots"]:
        k = 5 - len(s["board"])
        assert len(s["h"]) == math.comb(s["pool"], 2) and s["completions"] == math.comb(s["pool"] - 2, k)
        assert sorted(s["cases"]) == sorted(CASES)
        assert max(s["cases"]["dying"]["void"]) > 0 and not any(s["cases"]["ones"]["void"])   # a range that dies; one that cannot
        for case in CASES:
            for b in ref["bins"]:                                                             # the row-sum invariant, in the fixture itself
                hist, void, valid = HS.fixture_expected(s, case, b)
                assert (hist.sum(axis=1, dtype=np.int64)[valid] + void[valid] == s["completions"]).all()
                assert not hist[~valid].any() and not void[~valid].any()


def test_spec_equals_reference_fixture():
    ref = fixture()
    bins = tuple(ref["bins"])
    for i, s in enumerate(ref["spots"]):
        nb = len(s["board"])
        weights = np.stack([np.ones(H, np.int64) if c == "ones" else HS.fixture_weights(ref, s, c).astype(np.int64) for c in CASES])
        got = HS.spot_hist(s["board"] + [0] * (5 - nb), nb, s["dead"], weights, bins)
        assert got["status"] == 0 and got["completions"] == s["completions"], i
        for r, case in enumerate(CASES):
            for b in bins:
                hist, void, valid = HS.fixture_expected(s, case, b)
                assert np.array_equal(got["valid"], valid), i
                assert np.array_equal(got["hist"][b][r], hist), (i, case, b)
                assert np.array_equal(got["void"][r], void), (i, case)
        alone = HS.spot_hist(s["board"] + [0] * (5 - nb), nb, s["dead"], None, 7)          # (the one-range, one-bins form)
        assert np.array_equal(alone["hist"], got["hist"][7][0]) and np.array_equal(alone["void"], got["void"][0]), i


def random_weights(rng):
    w = rng.integers(0, 65536, H).astype(np.uint16)
    w[rng.integers(0, H, 400)] = 0
    w[rng.integers(0, H, 100)] = 65535
    return w


@pytest.mark.parametrize("nb,pool", [(3, 6), (3, 9), (4, 5), (4, 12), (5, 4), (5, 20)])
def test_row_sum_invariant_and_river_decomposition_of_the_spec(nb, pool):
    """The identity that pins the definition: for a completion c the river spot (board + c, the same dead, the same weights) has row h =
    (below, equal, den) in the range-vs-range spec for every h disjoint from c; the histogram is the sum of the one-hot bins of those rows."""
    rng = np.random.default_rng(0x48495354 + 10 * nb + pool)
    board, nboard, dead = VS.random_boards(rng, 1, nb, pool)
    sparse = np.zeros(H, np.int64)
    sparse[rng.integers(0, H, 120)] = rng.integers(1, 65536, 120)                         # a range that dies on some completions
    ranges = np.stack([random_weights(rng).astype(np.int64), np.ones(H, np.int64), sparse])
    bins = (1, 2, 7, 10, 32)
    got = HS.spot_hist(board[0], nb, dead[0], ranges, bins)
    assert got["status"] == 0 and got["completions"] == math.comb(pool - 2, 5 - nb) and got["valid"].sum() == math.comb(pool, 2)
    v = got["valid"]
    for b in bins:
        total = got["hist"][b].sum(axis=2, dtype=np.int64) + got["void"]
        assert (total[:, v] == got["completions"]).all() and not total[:, ~v].any(), b
    assert not got["void"][1].any()                                                       # all ones: den > 0 by count
    rivers, live = HS.river_boards(board[0], nb, dead[0])
    assert len(rivers) == math.comb(pool, 5 - nb) and (live.sum(axis=0)[v] == got["completions"]).all()
    rows = [VS.spot_rvr(rv, 5, dead[0], ranges) for rv in rivers]
    assert all(r["status"] == 0 for r in rows)
    for r in range(3):
        win, tie, tot = (np.stack([x[key][r] for x in rows]) for key in ("win", "tie", "tot"))
        for b in bins:
            hist, void = HS.one_hot_sum(win, tie, tot, live, b)
            assert np.array_equal(hist, got["hist"][b][r]) and np.array_equal(void, got["void"][r]), (r, b)


def test_bin_rule_at_its_edges():
    for n in (1, 2, 7, 10, 32):
        for j in range(n + 1):                                                            # strength exactly j / n -> bin j; strength 1 -> the last bin
            want = min(j, n - 1)
            assert HS.bin_of(j, 0, n, n) == want                                          # below / den = j / n
            if 2 * j <= n:
                assert HS.bin_of(0, 2 * j, n, n) == want                                  # ties only: (equal / 2) / den = j / n
            assert HS.bin_of(j * 65535, 0, n * 65535, n) == want
            if 0 < j:
                assert HS.bin_of(2 * j - 1, 1, 2 * n, n) == j - 1                         # a hair under j / n: (4 j - 1) / (4 n)
        assert HS.bin_of(0, 0, 5, n) == 0 and HS.bin_of(5, 0, 5, n) == n - 1 and HS.bin_of(0, 5, 5, n) == min(n - 1, n // 2)
        assert HS.bin_of(0, 0, 0, n) is None                                              # den = 0: void
    # the largest product there is: every weight 65 535, 990 villains, 32 bins -- below the 2^32 the device computes in
    top = 65535 * 990
    assert 32 * 2 * top == 4152297600 < 2 ** 32
    assert HS.bin_of(top, 0, top, 32) == 31 and HS.bin_of(0, top, top, 32) == 16 and HS.bin_of(top - 1, 0, top, 32) == 31
    assert HS.bin_of(top - 65535, 65535, top, 32) == 31 and HS.bin_of(top // 32, 0, top, 32) == 0 and HS.bin_of(-(-top // 32), 0, top, 32) == 1
    # ... and in uint32 arithmetic, as the device does it, every one of these gives the same bin
    for below, equal in ((top, 0), (0, top), (top - 1, 0), (top - 65535, 65535), (top // 32, 0), (-(-top // 32), 0)):
        num = np.uint32(32) * (np.uint32(2) * np.uint32(below) + np.uint32(equal))
        assert int(num) == 32 * (2 * below + equal)
        assert min(31, int(num // (np.uint32(2) * np.uint32(top)))) == HS.bin_of(below, equal, top, 32)
    with pytest.raises(AssertionError):
        HS.bin_of(1, 0, 1, 33)
    with pytest.raises(AssertionError):
        HS.bin_of(1, 0, 1, 0)


def test_a_river_spot_is_one_count_per_valid_holding():
    rng = np.random.default_rng(5)
    board, nboard, dead = VS.random_boards(rng, 1, 5, 12)
    valid = HS.spot_hist(board[0], 5, dead[0], None, 1)["valid"]
    w = np.zeros(H, np.int64)
    first = VS.PAIR_A[np.flatnonzero(valid)[0]]
    w[valid & ((VS.PAIR_A == first) | (VS.PAIR_B == first))] = 7                          # the holdings {first pool card, x}: whoever holds that card meets no weight
    got = HS.spot_hist(board[0], 5, dead[0], w, 10)
    assert got["completions"] == 1 and got["valid"].sum() == 66
    total = got["hist"].sum(axis=1, dtype=np.int64) + got["void"]
    assert (total[got["valid"]] == 1).all() and not total[~got["valid"]].any() and got["void"].any() and got["hist"].any()


def test_status_bits_are_those_of_range_vs_range(lib):
    board = [0x20, 0x21, 0x22, 0x23, 0x24]
    spots = [(board, 5, 0), (board, 2, 0), (board, 0, 0), (board, 6, 0), (board, 255, 0), ([0x20, 0x21, 0xFF, 0x23, 0x24], 4, 0),
             ([0x20, 0x4F, 0x22, 0x23, 0x24], 4, 0), (board, 5, 1 << 52), ([0x20, 0x20, 0x22, 0x23, 0x24], 3, 0), (board, 5, 1 << VS.canon_index(0x21))]
    for nb in (5, 4, 3):
        k = 5 - nb
        free = [c for c in range(52) if c not in {VS.canon_index(x) for x in board[:nb]}]
        spots += [(board, nb, sum(1 << c for c in free[k + 4:])), (board, nb, sum(1 << c for c in free[k + 3:]))]
    seen = set()
    for b, nb, dead in spots:
        got = HS.spot_hist(b, nb, dead, None, 4)                                          # (no full-pool turn or flop is enumerated here)
        want = VS.check_spot(b, nb, dead)[0]
        seen.add(want)
        assert got["status"] == want, (b, nb, dead)
        if want:
            assert got["completions"] == 0 and not got["hist"].any() and not got["void"].any() and not got["valid"].any()
        else:
            assert got["completions"] > 0 and got["valid"].sum() >= 6
    assert seen == {0, VS.BAD_CARD, VS.DUP_CARD, VS.BAD_NBOARD, VS.PREFLOP, VS.SMALL_POOL}
    assert HS.MAX_BINS == lib.EQ_HIST_MAX_BINS == 32
    for nb in (5, 4, 3):                                                                  # P = k + 4: one villain per hero and completion
        k = 5 - nb
        free = [c for c in range(52) if c not in {VS.canon_index(x) for x in board[:nb]}]
        got = HS.spot_hist(board, nb, sum(1 << c for c in free[k + 4:]), None, 2)
        assert got["completions"] == math.comb(k + 2, k) and got["valid"].sum() == math.comb(k + 4, 2)


def test_header_declares_and_binding_lists_the_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "pokerl_hip.h")).read()
    import ctypes
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in lib.SYMBOLS and hasattr(L, name), name
    assert re.search(r"#define PK_EQ_HIST_MAX_BINS 32\b", header)
    assert "completions u32 [m] = C(P - 2, k)" in header and "NOT the `boards` = C(P - 4, k) of range vs range" in header
    assert "INVARIANT: for a valid h, sum over b of hist[h][b] + void[h] = completions" in header
    assert lib.lib().pk_abi_version() == 6


def test_hist_kernels_exist_without_scratch_and_k_rvr_is_as_it_was(lib):
    """`.private_segment_fixed_size` == 0 and no spilled VGPR for the new kernels; the group segment of k_hist holds the 32 KB table and the
    sort, and lets two workgroups share a CU: at most 65 536 bytes; at most 128 registers: four waves per SIMD.  k_rvr, whose stages k_hist
    copies, still has the figures of the commit that added it."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(lib.LIB_PATH)
    hist = {k: d for k, d in ks.items() if k.startswith("k_hist")}
    assert sorted(hist) == ["k_hist", "k_hist_counts"], sorted(hist)
    assert all(d["private_segment"] == 0 and d["vgpr_spill"] == 0 for d in hist.values()), hist
    assert 32768 < hist["k_hist"]["lds"] <= 65536, hist["k_hist"]["lds"]
    assert hist["k_hist"]["vgprs"] + hist["k_hist"]["agprs"] <= 128                        # four waves per SIMD
    assert (ks["k_rvr"]["vgprs"], ks["k_rvr"]["agprs"], ks["k_rvr"]["lds"], ks["k_rvr"]["private_segment"], ks["k_rvr"]["vgpr_spill"]) == (110, 0, 63152, 0, 0)
    assert sorted(k for k in ks if k.startswith("k_rvr")) == ["k_rvr", "k_rvr_prep<false>", "k_rvr_prep<true>"]   # one preparation kernel for both families


def test_null_arguments_and_bad_nbins_are_refused_without_a_device(lib):
    L = lib.lib()
    assert L.pk_table_equity_hist_d(None, None, 4, None, 0, 10, None, None, None, None) == lib.PK_E_INVALID_ARG
    assert L.pk_table_equity_hist(None, None, 4, None, 0, 10, None, None, None, None) == lib.PK_E_INVALID_ARG
    one = np.zeros(64, np.uint8)
    assert L.pk_equity_hist(0, 1, None, lib.ptr(one), None, None, 0, 10, None, None, None, None) == lib.PK_E_INVALID_ARG
    assert b"pk_equity_hist" in L.pk_last_error(None)
    assert L.pk_equity_hist_d(0, 1, lib.ptr(one), None, None, None, 0, 10, None, None, None, None, None) == lib.PK_E_INVALID_ARG
    assert b"pk_equity_hist_d" in L.pk_last_error(None)
    assert L.pk_equity_hist_d(0, 2 ** 31, lib.ptr(one), lib.ptr(one), None, None, 0, 10, None, None, None, None, None) == lib.PK_E_INVALID_ARG
    for nbins in (0, 33, -1, 65536):
        assert L.pk_equity_hist(0, 1, lib.ptr(one), lib.ptr(one), None, None, 0, nbins, None, None, None, None) == lib.PK_E_INVALID_ARG, nbins
        assert b"pk_equity_hist" in L.pk_last_error(None) and b"nbins" in L.pk_last_error(None)
        assert L.pk_equity_hist_d(0, 1, lib.ptr(one), lib.ptr(one), None, None, 0, nbins, None, None, None, None, None) == lib.PK_E_INVALID_ARG, nbins
        assert b"pk_equity_hist_d" in L.pk_last_error(None) and b"nbins" in L.pk_last_error(None)
        assert L.pk_equity_hist(0, 0, None, None, None, None, 0, nbins, None, None, None, None) == lib.PK_E_INVALID_ARG, nbins   # (even with no spot)
    assert L.pk_equity_hist_d(64, 1, lib.ptr(one), lib.ptr(one), None, None, 0, 10, None, None, None, None, None) != lib.PK_OK


def test_python_helpers_validate_before_any_device_call(lib):
    import pokerl_amd as P
    from pokerl_amd import judger as J
    assert P.strength_histogram is J.strength_histogram and P.StrengthHistogram is J.StrengthHistogram and P.histogram_emd is J.histogram_emd
    assert P.strength_histogram_batch is J.strength_histogram_batch and P.strength_histogram_d is J.strength_histogram_d
    assert all(hasattr(P.VecGame, n) for n in ("equity_hist", "equity_hist_d")) and hasattr(P.Game, "equity_hist")
    with pytest.raises(ValueError, match="fewer than three board cards"):
        J.strength_histogram(["2S", "3S"])                                               # pre-flop
    with pytest.raises(ValueError):
        J.strength_histogram(["2S"] * 6)
    with pytest.raises(ValueError):
        J.strength_histogram(["AS", 0x4F, "2S"])                                         # not a card
    with pytest.raises(ValueError):
        J.strength_histogram(["2S", "3S", "4S"], weights=np.ones(1325, np.uint16))
    with pytest.raises(ValueError):
        J.strength_histogram(["2S", "3S", "4S"], weights=np.full(1326, 65536))
    with pytest.raises(ValueError):
        J.strength_histogram(["2S", "3S", "4S"], weights=np.ones((1, 1326), np.uint16))
    for bins in (0, 33, -1, 2.5, "10", None, True):
        with pytest.raises(ValueError, match="bins"):
            J.strength_histogram(["2S", "3S", "4S"], bins=bins)
        with pytest.raises(ValueError, match="bins"):
            J.strength_histogram_batch(np.zeros((3, 5), np.uint8), np.zeros(3), bins=bins)
        with pytest.raises(ValueError, match="bins"):
            J.strength_histogram_d(1, 0, 0, bins=bins)
    with pytest.raises(ValueError):
        J.strength_histogram_batch(np.zeros((3, 4), np.uint8), np.zeros(3))
    with pytest.raises(ValueError):
        J.strength_histogram_batch(np.zeros((3, 5), np.uint8), np.zeros(2))
    with pytest.raises(ValueError):
        J.strength_histogram_batch(np.zeros((3, 5), np.uint8), np.zeros(3), dead=np.zeros(2, np.uint64))
    with pytest.raises(ValueError):
        J.strength_histogram_batch(np.zeros((3, 5), np.uint8), np.zeros(3), weights=np.ones((2, 1326), np.uint16))


def test_pdf_cdf_and_emd_on_hand_made_arrays():
    from pokerl_amd import judger as J
    hist = np.zeros((2, H, 4), np.uint16)
    hist[0, 0], hist[0, 1], hist[0, 2] = [1, 1, 0, 2], [0, 0, 0, 8], [4, 0, 0, 0]         # holding 3 on: nothing counted
    void = np.zeros((2, H), np.uint16)
    void[0, 3] = 4
    r = J.StrengthHistogram(hist, void, np.array([4, 0], np.uint32), np.array([0, VS.PREFLOP], np.uint8))
    assert r.bins == 4 and r.pdf.dtype == np.float64 and r.pdf.shape == (2, H, 4)
    assert r.pdf[0, 0].tolist() == [0.25, 0.25, 0.0, 0.5] and r.pdf[0, 1].tolist() == [0, 0, 0, 1] and np.isnan(r.pdf[0, 3:]).all() and np.isnan(r.pdf[1]).all()
    assert r.cdf[0, 0].tolist() == [0.25, 0.5, 0.5, 1.0] and r.cdf[0, 2].tolist() == [1, 1, 1, 1] and np.isnan(r.cdf[0, 3]).all()
    one = r[0]
    assert one.hist.shape == (H, 4) and one.completions == 4 and one.status == 0 and one.void[3] == 4 and one.pdf[0, 3] == 0.5 and r[1].status == VS.PREFLOP
    # the earth mover's distance in bin units: all the mass moved from bin 0 to bin 3 is 3; the L1 distance of the CDFs
    assert J.histogram_emd(hist[0, 2], hist[0, 1]) == 3.0 and J.histogram_emd(hist[0, 1], hist[0, 2]) == 3.0
    assert J.histogram_emd(hist[0, 0], hist[0, 0]) == 0.0
    assert J.histogram_emd(hist[0, 0], hist[0, 1]) == 0.25 + 0.5 + 0.5 and J.histogram_emd(hist[0, 0], hist[0, 2]) == 0.75 + 0.5 + 0.5
    assert J.histogram_emd([1, 1], [2, 2]) == 0.0 and J.histogram_emd([0.5, 0.5], [0, 1]) == 0.5   # each normalised by its own sum
    d = J.histogram_emd(hist[0, :4], hist[0, 1])                                          # broadcast: [4, bins] against [bins]
    assert d.shape == (4,) and d[:3].tolist() == [1.25, 0.0, 3.0] and math.isnan(d[3])
    assert J.histogram_emd(r.pdf[0, 0], r.hist[0, 2]) == 1.75                             # a pdf against counts
    with pytest.raises(ValueError):
        J.histogram_emd([1, 2, 3], [1, 2])
