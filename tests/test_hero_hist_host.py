"""CPU tests of the hero strength histogram (no GPU): the numpy restatement of the definition (hero_hist_spec) against row h of the
strength-histogram spec for every valid h and against every row of the reference's fixture, the status rule against range equity's, the new
entry points in the header and the binding, the new kernel in the built library's code objects, and the argument validation of the C entry
points and of the Python helpers."""
import json
import os
import re
import sys

import numpy as np
import pytest

import equity_range_spec as RS
import hero_hist_spec as HH
import hist_spec as HS
import rvr_spec as VS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pk_equity_hist_hero_d", "pk_equity_hist_hero", "pk_table_equity_hist_hero_d", "pk_table_equity_hist_hero")
BINS = (1, 2, 7, 10, 32)
H = HH.HOLDINGS


@pytest.fixture(scope="module")
def lib():
    from pokerl_amd import _lib, build
    build.build_lib()
    return _lib


def ranges(rng):
    """random (a third zero) / 65 535 / ones / zero, as one [4, 1326] array."""
    w = rng.integers(0, 200, H)
    w[rng.random(H) < 0.33] = 0
    return np.stack([w, np.full(H, 65535), np.ones(H, np.int64), np.zeros(H, np.int64)]).astype(np.int64)


def hero_of(h):
    return [RS.CANON[RS.PAIR_A[h]], RS.CANON[RS.PAIR_B[h]]]


def rows_equal_public_form(board, nb, dead, w, where):
    """spot_hero_hist(hero = h, the same board / dead / weights) == row h of hist_spec.spot_hist, for EVERY valid h."""
    pub = HS.spot_hist(board, nb, dead, w, BINS)
    assert pub["status"] == 0 and pub["valid"].any(), where
    for h in np.flatnonzero(pub["valid"]):
        got = HH.spot_hero_hist(hero_of(h), board, nb, dead, w, BINS)
        assert got["status"] == 0 and got["completions"] == pub["completions"], (where, h)
        assert np.array_equal(got["void"], pub["void"][:, h]), (where, h)
        for b in BINS:
            assert np.array_equal(got["hist"][b], pub["hist"][b][:, h]), (where, h, b)
            assert (got["hist"][b].sum(axis=-1) + got["void"] == got["completions"]).all(), (where, h, b)   # the invariant
    return int(pub["valid"].sum())


@pytest.mark.parametrize("nb,pool", [(3, 6), (3, 7), (3, 12), (4, 5), (4, 12), (5, 4), (5, 12)])
def test_spec_equals_the_public_form_row_for_every_valid_holding(nb, pool):
    rng = np.random.default_rng(1000 * nb + pool)
    board, nboard, dead = VS.random_boards(rng, 1, nb, pool=pool)
    n = rows_equal_public_form([int(x) for x in board[0]], nb, int(dead[0]), ranges(rng), (nb, pool))
    assert n == pool * (pool - 1) // 2


def test_spec_equals_every_row_of_the_reference_fixture():
    with open(os.path.join(ROOT, "tests", "golden", "hist_ref.json")) as f:
        ref = json.load(f)
    assert ref["holdings"] == H
    rows = 0
    for s in ref["spots"]:
        nb = len(s["board"])
        board = s["board"] + [0] * (5 - nb)
        for case in s["cases"]:
            w = HS.fixture_weights(ref, s, case)
            want = {b: HS.fixture_expected(s, case, b) for b in ref["bins"]}
            for h in s["h"]:                                         # every h of every spot and every case; the hero's cards leave `dead`
                got = HH.spot_hero_hist(hero_of(h), board, nb, s["dead"], w, tuple(ref["bins"]))
                assert got["status"] == 0 and got["completions"] == s["completions"], (s["name"], case, h)
                for b in ref["bins"]:
                    assert np.array_equal(got["hist"][b], want[b][0][h]) and got["void"] == want[b][1][h], (s["name"], case, h, b)
                rows += 1
    assert rows == 3 * sum(len(s["h"]) for s in ref["spots"]) >= 500


def test_status_bits_equal_range_equity_on_bad_spots(lib):
    hero, board = [0x00, 0x01], [0x20, 0x21, 0x22, 0x23, 0x24]
    used = {RS.canon_index(c) for c in hero + board}
    free = [k for k in range(52) if k not in used]
    mask = lambda left: sum(1 << k for k in free[left:])
    spots = [(hero, board, 5, 0), (hero, board, 3, 0), (hero, board, 0, 0), (hero, board, 2, 0), (hero, board, 6, 0), (hero, board, 255, 0),
             ([0x00, 0xFF], board, 5, 0), ([0x0D, 0x01], board, 5, 0), ([0x4F, 0x01], board, 4, 0), (hero, [0x20, 0x21, 0xFF, 0x23, 0x24], 4, 0),
             (hero, board, 5, 1 << 52), (hero, board, 5, 1 << 63), ([0x00, 0x00], board, 5, 0), ([0x00, 0x20], board, 3, 0),
             (hero, [0x20, 0x20, 0x22, 0x23, 0x24], 3, 0), (hero, board, 5, 1 << RS.canon_index(0x21)), (hero, board, 5, 1 << RS.canon_index(0x01)),
             (hero, board, 5, mask(2)), (hero, board, 5, mask(1)), (hero, board, 4, mask(3)), (hero, board, 4, mask(2)), (hero, board, 3, mask(4)),
             (hero, board, 3, mask(3)), ([0x00, 0x0D], board, 1, 1 << 60)]
    seen = 0
    for i, (he, bo, nb, dead) in enumerate(spots):
        got = HH.spot_hero_hist(he, bo, nb, dead, None, 7)
        want = RS.spot_range(he, bo, nb, dead)
        assert got["status"] == want["status"], i
        seen |= got["status"]
        if got["status"]:
            assert got["completions"] == 0 and not got["hist"].any() and got["void"] == 0, i
        else:
            assert got["hist"].sum() + got["void"] == got["completions"] > 0, i
    assert seen == RS.BAD_CARD | RS.DUP_CARD | RS.BAD_NBOARD | RS.PREFLOP | RS.SMALL_POOL
    assert (RS.PREFLOP, RS.SMALL_POOL) == (lib.EQ_PREFLOP, lib.EQ_SMALL_POOL)


def test_header_declares_and_binding_lists_the_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "pokerl_hip.h")).read()
    import ctypes
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in lib.SYMBOLS and hasattr(L, name), name
    assert "Hero strength histogram" in header
    assert lib.lib().pk_abi_version() == 6
    import pokerl_amd as P
    from pokerl_amd import judger as J
    for name in ("HeroHistogram", "hero_histogram", "hero_histogram_batch", "hero_histogram_d"):
        assert getattr(P, name) is getattr(J, name) and name in P.__all__, name
    for cls, names in ((P.VecGame, ("equity_hist_hero", "equity_hist_hero_d", "bucket")), (P.Game, ("equity_hist_hero", "bucket"))):
        for name in names:
            assert callable(getattr(cls, name)), name


def test_hero_kernel_exists_without_scratch_within_its_occupancy(lib):
    """`.private_segment_fixed_size` == 0 and no spill for the new kernels; k_hero_hist declares __launch_bounds__(512, 6) -- three 512-thread
    workgroups per CU --, so its LDS (the 32 KB table, the hero's words, two counters per completion, the weights) is at most 163 840 / 3 =
    54 613 bytes and a lane has at most 512 / 6 -> 80 registers."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(lib.LIB_PATH)
    hh = {k: d for k, d in ks.items() if k.startswith("k_hero_hist")}
    assert sorted(hh) == ["k_hero_hist", "k_hero_hist_counts"], sorted(hh)
    assert all(d["private_segment"] == 0 and d["vgpr_spill"] == 0 for d in hh.values()), hh
    k = hh["k_hero_hist"]
    assert 32768 + 3 * 4 * 1081 + 2 * 1326 <= k["lds"] <= 54613, k["lds"]
    unified = (k["vgprs"] + 3) // 4 * 4 + max(k["agprs"], 0)         # one register file: the accumulation registers start at a multiple of 4
    assert 0 < unified <= 80, k
    src = open(os.path.join(ROOT, "pokerl_amd", "csrc", "pk_equity_hist_hero.hip")).read()
    assert re.search(r"__launch_bounds__\(HH_BLOCK, 6\)\s+k_hero_hist\(", src)
    # the kernels of the families this one borrows from are still there
    assert "k_eqr" in ks and "k_hist" in ks and "k_eqr_prep<true>" in ks


def test_bad_arguments_are_refused_without_a_device(lib):
    L = lib.lib()
    one = np.zeros(64, np.uint8)
    cen = np.zeros((2, 10), np.uint16)
    lab = np.zeros(4, np.uint16)
    dist = np.zeros(4, np.uint32)
    p = lib.ptr

    def host(m=1, hero=one, board=one, nboard=one, bins=10, K=0, centroids=None, label=None, dist_=None):
        return L.pk_equity_hist_hero(0, m, p(hero) if hero is not None else None, p(board) if board is not None else None,
                                     p(nboard) if nboard is not None else None, None, None, 0, bins, None, None, None, None, K,
                                     p(centroids) if centroids is not None else None, p(label) if label is not None else None,
                                     p(dist_) if dist_ is not None else None)

    def dev(m=1, hero=one, bins=10, K=0, centroids=None, label=None, dist_=None):
        return L.pk_equity_hist_hero_d(0, m, p(hero) if hero is not None else None, p(one), p(one), None, None, 0, bins, None, None, None, None, K,
                                       p(centroids) if centroids is not None else None, p(label) if label is not None else None,
                                       p(dist_) if dist_ is not None else None, None)

    def refused(rc, *texts):
        assert rc == lib.PK_E_INVALID_ARG, rc
        err = L.pk_last_error(None)
        for t in texts:
            assert t in err, (t, err)

    for call, name in ((host, b"pk_equity_hist_hero"), (dev, b"pk_equity_hist_hero_d")):
        refused(call(hero=None), name, b"NULL input buffer")
        refused(call(m=2 ** 31), name, b"m >= 2^31")
        for bins in (0, 33, -1):
            refused(call(bins=bins), name, b"nbins must be 1 .. PK_EQ_HIST_MAX_BINS (32)")
        for K in (-1, 4097):
            refused(call(K=K, centroids=cen, label=lab), name, b"K must be 0 (no bucket stage) or 1 .. PK_CL_MAX_K (4096)")
        refused(call(K=2, label=lab), name, b"NULL centroids with K > 0")
        refused(call(K=0, label=lab), name, b"label / dist asked for with K = 0")
        refused(call(K=0, dist_=dist), name, b"label / dist asked for with K = 0")
    refused(host(board=None), b"NULL input buffer")
    refused(host(nboard=None), b"NULL input buffer")
    # a device index no device has: refused, whatever the machine (no GPU is needed to say so)
    assert L.pk_equity_hist_hero_d(64, 1, p(one), p(one), p(one), None, None, 0, 10, None, None, None, None, 0, None, None, None, None) != lib.PK_OK
    # the table forms without a handle, whatever the observer (PK_OBSERVER_NONE with a handle: tests/test_hip_hero_hist.py)
    for obs in (0, lib.OBSERVER_NONE, lib.OBSERVER_ACTIVE):
        assert L.pk_table_equity_hist_hero_d(None, None, 4, obs, None, 0, 10, None, None, None, None, 0, None, None, None) == lib.PK_E_INVALID_ARG
        assert L.pk_table_equity_hist_hero(None, None, 4, obs, None, 0, 10, None, None, None, None, 0, None, None, None) == lib.PK_E_INVALID_ARG


def test_python_helpers_validate_before_any_device_call(lib):
    from pokerl_amd import judger as J
    flop = ["2S", "3S", "4S"]
    with pytest.raises(ValueError):
        J.hero_histogram(["AS"], flop)                                           # one hero card
    with pytest.raises(ValueError, match="fewer than three board cards"):
        J.hero_histogram(["AS", "KS"], ["2S", "3S"])                             # pre-flop
    with pytest.raises(ValueError):
        J.hero_histogram(["AS", "KS"], ["2S"] * 6)
    with pytest.raises(ValueError):
        J.hero_histogram(["AS", 0x4F], flop)                                     # not a card
    for bins in (0, 33, 2.0, True):
        with pytest.raises(ValueError, match="bins"):
            J.hero_histogram(["AS", "KS"], flop, bins=bins)
    with pytest.raises(ValueError):
        J.hero_histogram(["AS", "KS"], flop, weights=np.ones(1325, np.uint16))
    with pytest.raises(ValueError):
        J.hero_histogram(["AS", "KS"], flop, weights=np.full(1326, 65536))
    with pytest.raises(ValueError, match="centroids"):
        J.hero_histogram(["AS", "KS"], flop, bins=10, centroids=np.zeros((3, 7), np.uint16))     # bins of the centroids differ
    with pytest.raises(ValueError, match="centroids"):
        J.hero_histogram(["AS", "KS"], flop, bins=4, centroids=np.full((3, 4), 65536))
    with pytest.raises(ValueError, match="centroids"):
        J.hero_histogram(["AS", "KS"], flop, bins=4, centroids=np.zeros((0, 4), np.uint16))
    with pytest.raises(ValueError):
        J.hero_histogram_batch(np.zeros((3, 3), np.uint8), np.zeros((3, 5)), np.zeros(3))
    with pytest.raises(ValueError):
        J.hero_histogram_batch(np.zeros((3, 2), np.uint8), np.zeros((3, 4)), np.zeros(3))
    with pytest.raises(ValueError):
        J.hero_histogram_batch(np.zeros((3, 2), np.uint8), np.zeros((3, 5)), np.zeros(3), dead=np.zeros(2, np.uint64))
    with pytest.raises(ValueError):
        J.hero_histogram_batch(np.zeros((3, 2), np.uint8), np.zeros((3, 5)), np.zeros(3), weights=np.ones((2, 1326), np.uint16))
    for kw in (dict(bins=0), dict(k=-1), dict(k=4097), dict(k=2), dict(k=0, label_d=1), dict(k=0, dist_d=1)):
        with pytest.raises(ValueError):
            J.hero_histogram_d(1, 1, 1, 1, **kw)
    r = J.HeroHistogram(np.array([[1, 3], [0, 0]], np.uint16), np.array([0, 4], np.uint16), np.array([4, 4], np.uint32), np.array([0, 0], np.uint8),
                        np.array([1, 0xFFFF], np.uint16), np.array([65535, 0], np.uint32))
    assert r.bins == 2 and r.pdf[0].tolist() == [0.25, 0.75] and r.cdf[0].tolist() == [0.25, 1.0] and np.isnan(r.pdf[1]).all()
    assert r.emd.tolist() == [1.0, 0.0] and r[0].label == 1 and r[1].label == lib.CL_NONE and r[0].hist.tolist() == [1, 3]
    assert J.HeroHistogram(r.hist, r.void, r.completions, r.status).emd is None
