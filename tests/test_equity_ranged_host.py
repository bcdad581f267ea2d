"""CPU tests of the ranged sampled equity (no GPU): the Python restatement of the definition (tests/equity_ranged_spec.py) against the
exact range aggregates of tests/equity_range_spec.py and against identities of its own; the entry points in the header, the binding and the
library; argument validation in the C ABI and in the Python helpers; the sampling kernels' code objects (no scratch, no spilled VGPR, LDS per
size class)."""
import os
import re
import sys

import numpy as np
import pytest

import equity_range_spec as RS
import equity_ranged_spec as WS
import equity_spec as ES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pk_equity_ranged_d", "pk_equity_ranged", "pk_table_equity_ranged_d", "pk_table_equity_ranged")
U = WS.UNIFORM


@pytest.fixture(scope="module")
def lib():
    from pokerl_amd import _lib, build
    build.build_lib()
    return _lib


def turn_spot():
    """Hero AS AD against one hidden hand on KS 7D 7C 2H (section 3.2's fixed spot): (holes, board, nb, live)."""
    from pokerl_amd.cards import card_value as cv
    holes = np.array([[cv("AS"), cv("AD")], [ES.UNKNOWN, ES.UNKNOWN]], np.uint8)
    return holes, [cv("KS"), cv("7D"), cv("7C"), cv("2H"), 0], 4, 0b11


def turn_range():
    """The fixed range of the convergence test: numpy's default_rng(20241), about 60 % zeros, weights 0 .. 49."""
    rng = np.random.default_rng(20241)
    w = rng.integers(0, 50, WS.HOLDINGS)
    w[rng.random(WS.HOLDINGS) < 0.6] = 0
    return w.astype(np.uint16)


def test_spec_converges_to_the_exact_range_aggregates_on_the_turn_spot():
    """S = 16 384 attempts of the turn spot under turn_range() against equity_range_spec.aggregate: |win / accepted - agg0 / agg2| and the tie
    analogue each <= 5 sqrt(p (1 - p) / accepted) -- five binomial standard deviations over the accepted attempts, derived; seed and nonce
    fixed, so the outcome is deterministic.  Measured with this range: accepted 12 637 of 16 384; win 0.896336 against 0.897918 exact, deviation
    1.6e-3 (bound 1.35e-2); tie 0.002849 against 0.002886, deviation 3.8e-5 (bound 2.4e-3)."""
    holes, board, nb, live = turn_spot()
    w = turn_range()
    assert 0.55 < (w == 0).mean() < 0.65 and w.max() <= 49
    agg = RS.aggregate(RS.spot_range(holes[0], board, nb), w)
    s = 16384
    got = WS.spot_equity(holes, board, nb, live, s, w, [U, 0], seed=WS.DEFAULT_SEED, nonce=0, ident=0)
    acc = got["accepted"]
    assert got["status"] == 0 and 0 < acc < s
    for name, count, exact in (("win", got["win"][0], agg[0]), ("tie", got["tie"][0], agg[1])):
        p = exact / agg[2]
        dev, bound = abs(count / acc - p), 5 * np.sqrt(p * (1 - p) / acc)
        print("turn spot, %s: accepted %d, exact %.6f, sampled %.6f, deviation %.3g, bound %.3g" % (name, acc, p, count / acc, dev, bound))
        assert dev <= bound, (name, dev, bound)
    assert int(got["share"].astype(object).sum()) == ES.SHARE_UNIT * acc
    # the acceptance itself: the weight on holdings clear of the six dead cards over the whole weight, within five standard deviations
    valid = RS.spot_range(holes[0], board, nb)["valid"]
    q = w[valid].astype(np.int64).sum() / w.astype(np.int64).sum()
    assert abs(acc / s - q) <= 5 * np.sqrt(q * (1 - q) / s)


def test_spec_identities():
    rng = np.random.default_rng(4)
    # a one-holding range on the river: every attempt is accepted and ends the same way -> win = accepted * indicator
    holes, board, nboard, live = ES.random_spots(rng, 3, 4, nb=5, unknown=False)
    for i in range(4):
        exact = ES.spot_equity(holes[i], [int(x) for x in board[i]], 5, 7)
        w = np.zeros((2, WS.HOLDINGS), np.uint16)
        w[0, WS.holding_index(*holes[i, 1])] = 9
        w[1, WS.holding_index(*holes[i, 2])] = 1
        hid = holes[i].copy()
        hid[1:] = ES.UNKNOWN
        got = WS.spot_equity(hid, [int(x) for x in board[i]], 5, 7, 37, w, [U, 0, 1], ident=i)
        assert got["accepted"] == 37 and got["status"] == 0
        for k in ("win", "tie", "share"):
            assert (got[k].astype(np.uint64) == 37 * exact[k].astype(np.uint64)).all(), (i, k)
        # ... and where the one holding is a dead card's: nothing is accepted, status 0
        w[1] = 0
        w[1, WS.holding_index(holes[i, 0, 0], holes[i, 2, 1])] = 5
        dead = WS.spot_equity(hid, [int(x) for x in board[i]], 5, 7, 37, w, [U, 0, 1], ident=i)
        assert dead["accepted"] == 0 and dead["status"] == 0 and not dead["win"].any() and not dead["share"].any()
    # an all-zero range: accepted 0 with status 0
    holes, board, nb, live = turn_spot()
    zero = WS.spot_equity(holes, board, nb, live, 64, np.zeros(WS.HOLDINGS, np.uint16), [U, 0])
    assert zero["accepted"] == 0 and zero["status"] == 0 and not zero["win"].any() and not zero["tie"].any() and not zero["share"].any()
    # nonces: two streams whose counts add (the attempts are independent of each other, so each half is a valid sample of its own)
    w = turn_range()
    a, b = (WS.spot_equity(holes, board, nb, live, 500, w, [U, 0], nonce=x) for x in (1, 2))
    assert (a["win"] != b["win"]).any() and a["accepted"] != 0 and b["accepted"] != 0
    total_share = int(a["share"].astype(object).sum()) + int(b["share"].astype(object).sum())
    assert total_share == ES.SHARE_UNIT * (a["accepted"] + b["accepted"])
    # a prefix of the stream: S = 300 is the first 300 attempts of S = 500
    hands, _, took = WS.attempts(holes, board, nb, live, w, [U, 0], WS.R.seed_key(WS.DEFAULT_SEED), 0, 1, 500)
    first = WS.spot_equity(holes, board, nb, live, 300, w, [U, 0], nonce=1)
    assert first["accepted"] == int((took < 300).sum())
    # the uniform row is the row of ones
    ones = WS.spot_equity(holes, board, nb, live, 200, np.ones(WS.HOLDINGS, np.uint16), [U, 0], nonce=3)
    unif = WS.spot_equity(holes, board, nb, live, 200, None, None, nonce=3)
    assert all((np.asarray(ones[k]) == np.asarray(unif[k])).all() for k in WS.KEYS)


def test_spec_statuses():
    holes = np.array([[0x00, 0x01], [ES.UNKNOWN, ES.UNKNOWN], [0x12, ES.UNKNOWN]], np.uint8)
    board = [0x20, 0x21, 0x22, 0x23, 0x24]
    w = np.ones((2, WS.HOLDINGS), np.uint16)

    def status(h, lv, ro, r=w):
        return WS.spot_equity(np.array(h, np.uint8), board, 5, lv, 8, r, ro)["status"]

    assert status(holes, 0b011, [0, 1, 0]) == 0
    assert status(holes, 0b111, [0, 1, 0]) == ES.BAD_CARD                      # seat 2 is live and shows one card
    assert status(holes, 0b011, [0, 2, 0]) == ES.BAD_CARD                      # row 2 of 2 at the hidden seat
    assert status(holes, 0b011, [2, 1, 7]) == 0                                # ... at a shown seat and at a seat that is not live: not read
    assert status(holes, 0b011, [0, U, 0]) == 0
    assert status(holes, 0b011, None, None) == 0
    assert status(holes, 0b011, [0, 0, 0], None) == ES.BAD_CARD                # R = 0: no row at all
    assert status(holes, 0, [0, 1, 0]) == ES.NO_LIVE


def test_header_declares_and_binding_lists_the_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "pokerl_hip.h")).read()
    import ctypes
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in lib.SYMBOLS and hasattr(L, name), name
    assert lib.lib().pk_abi_version() == 6
    assert "0x45515730" in header and WS.STREAM_EQW == int.from_bytes(b"EQW0", "big")
    assert re.search(r"#define PK_EQW_MAX_RANGES 16\b", header) and lib.EQW_MAX_RANGES == WS.MAX_RANGES == 16
    assert re.search(r"#define PK_EQW_UNIFORM 0xFFFFu", header) and lib.EQW_UNIFORM == WS.UNIFORM == 0xFFFF


def test_bad_arguments_are_refused_without_a_device(lib):
    L = lib.lib()
    one = np.zeros(64, np.uint8)
    p = lib.ptr(one)

    def explicit(n, m, samples, ranges=0, weights=None, holes=p):
        a = L.pk_equity_ranged(0, n, m, holes, p, p, p, None, samples, 1, 0, weights, ranges, None, None, None, None, None, None)
        b = L.pk_equity_ranged_d(0, n, m, holes, p, p, p, None, samples, 1, 0, weights, ranges, None, None, None, None, None, None, None)
        return a, b

    bad = (lib.PK_E_INVALID_ARG, lib.PK_E_INVALID_ARG)
    for n in (1, 17, -3):
        assert explicit(n, 1, 64) == bad
    assert b"pk_equity_ranged_d" in L.pk_last_error(None)
    for samples in (0, 2 ** 24 + 1, 2 ** 32 - 1):
        assert explicit(6, 1, samples) == bad
        assert b"samples" in L.pk_last_error(None)
    for ranges in (17, 2 ** 32 - 1):
        assert explicit(6, 1, 64, ranges, p) == bad
        assert b"num_ranges" in L.pk_last_error(None)
    assert explicit(6, 1, 64, 4, None) == bad                                   # rows without weights
    assert explicit(6, 1, 64, 0, None, None) == bad
    assert b"NULL" in L.pk_last_error(None)
    assert explicit(2, 2 ** 14, 2 ** 24) == bad
    assert b"32 bits" in L.pk_last_error(None)
    for observer in (lib.OBSERVER_NONE, 0, lib.OBSERVER_ACTIVE):
        assert L.pk_table_equity_ranged_d(None, None, 4, observer, 64, 0, None, 0, None, 0, None, None, None, None, None) == lib.PK_E_INVALID_ARG
        assert L.pk_table_equity_ranged(None, None, 4, observer, 64, 0, None, 0, None, 0, None, None, None, None, None) == lib.PK_E_INVALID_ARG


def test_python_helpers_validate_before_any_device_call(lib):
    from pokerl_amd import judger as J
    import pokerl_amd
    assert pokerl_amd.RangedEquity is J.RangedEquity and pokerl_amd.ranged_equity is J.ranged_equity
    assert pokerl_amd.ranged_equity_batch is J.ranged_equity_batch and pokerl_amd.ranged_equity_d is J.ranged_equity_d
    hu = [["AS", "KS"], None]
    w = np.ones(1326, np.uint16)
    for bad in (dict(samples=0), dict(samples=2 ** 24 + 1), dict(nonce=-1), dict(nonce=2 ** 32), dict(board=["2S"] * 6), dict(live=0b100),
                dict(ranges=np.ones(1325)), dict(ranges=np.ones((17, 1326))), dict(ranges=w, range_of=[0, 0, 0]), dict(ranges=w, range_of=[0, 70000])):
        with pytest.raises(ValueError):
            J.ranged_equity(hu, **bad)
    with pytest.raises(ValueError):
        J.ranged_equity([["AS", "KS"], ["QD", None]])                       # half a holding
    with pytest.raises(ValueError):
        J.ranged_equity_d(6, 3, 1, 1, 1, 1, samples=64, num_ranges=17)
    with pytest.raises(ValueError):
        J.ranged_equity_d(17, 3, 1, 1, 1, 1, samples=64)
    from pokerl_amd.game import VecGame
    from pokerl_amd.single import Game
    fake = VecGame.__new__(VecGame)                                         # no handle: validation must come before any call
    fake.num_players, fake.num_tables = 6, 4
    for bad in (dict(observer=6), dict(observer=None), dict(observer=lib.OBSERVER_NONE), dict(samples=0), dict(nonce=2 ** 32),
                dict(ranges=np.ones((17, 1326))), dict(ranges=w, range_of=np.zeros((3, 6)))):
        with pytest.raises(ValueError):
            fake.equity_ranged(**bad)
    for bad in (dict(observer=6), dict(observer=lib.OBSERVER_NONE), dict(samples=0), dict(num_ranges=17)):
        with pytest.raises(ValueError):
            fake.equity_ranged_d(**bad)
    assert hasattr(Game, "equity_ranged")
    e = J.RangedEquity(np.array([[3, 0]], np.uint32), np.array([[1, 1]], np.uint32), np.array([[3 * 720720 + 360360, 360360]], np.uint64),
                       np.array([4], np.uint32), np.array([0], np.uint8), 8)
    assert e.equity.tolist() == [[0.875, 0.125]] and e[0].equity.tolist() == [0.875, 0.125] and e.acceptance.tolist() == [0.5]
    none = J.RangedEquity(np.zeros((1, 2), np.uint32), np.zeros((1, 2), np.uint32), np.zeros((1, 2), np.uint64), np.array([0], np.uint32),
                          np.array([0], np.uint8), 8)
    assert np.isnan(none.equity).all() and none.acceptance.tolist() == [0.0]


# LDS of k_eqw<N, RC>: the 32 KB evaluator table, RC rows of 1326 u32 cumulative sums, the 1326 x u16 holding -> cards table, 32 share words
LDS_WANT = {0: 32768 + 4 + 2652 + 128, 8: 32768 + 8 * 5304 + 2652 + 128, 16: 32768 + 16 * 5304 + 2652 + 128}
CU_LDS = 160 * 1024


def test_ranged_kernels_have_no_scratch_no_vgpr_spill_and_fit_the_lds_budget(lib):
    """Every k_eqw<N, RC>: `.private_segment_fixed_size` 0 and `.vgpr_spill_count` 0; LDS exactly what the size class stages (an unused class
    0 row array is one word), so that R = 0 fits four workgroups per CU, R <= 8 (R <= 4 with it) two, R <= 16 one."""
    from pokerl_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(lib.LIB_PATH)
    eqw = {k: d for k, d in ks.items() if k.startswith("k_eqw")}
    names = ["k_eqw_cdf", "k_eqw_prep<true>", "k_eqw_prep<false>"] + ["k_eqw<%d, %d>" % (n, rc) for n in build.SEATS for rc in LDS_WANT]
    assert sorted(eqw) == sorted(names), sorted(eqw)
    assert build.SEATS == list(range(2, 17))
    assert all(d["private_segment"] == 0 and d["vgpr_spill"] == 0 for d in eqw.values()), {k: d for k, d in eqw.items() if d["private_segment"] or d["vgpr_spill"]}
    for n in build.SEATS:
        for rc, want in LDS_WANT.items():
            got = eqw["k_eqw<%d, %d>" % (n, rc)]["lds"]                       # (each of the four arrays may be padded to 16 bytes)
            assert want <= got <= want + 4 * 16, (n, rc, got)
    assert 4 * (LDS_WANT[0] + 64) <= CU_LDS and 2 * (LDS_WANT[8] + 64) <= CU_LDS and LDS_WANT[16] + 64 <= CU_LDS
    assert LDS_WANT[16] <= 16 * 5304 + 32768 + 4096                          # the issue's budget: the rows and the table, and little else
    print({rc: (LDS_WANT[rc], max(eqw["k_eqw<%d, %d>" % (n, rc)]["vgprs"] for n in build.SEATS)) for rc in LDS_WANT})
