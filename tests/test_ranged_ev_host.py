"""CPU tests of the ranged showdown EV (no GPU): identities of the numpy restatement (tests/ranged_ev_spec.py) against the two restatements it
is made of (equity_ranged_spec, ev_spec), its convergence to exact values within five derived standard deviations, its statuses; the entry
points in the header, the binding and the library; argument validation in the C ABI and in the Python helpers; the kernels' code objects (no
scratch, no spilled VGPR, LDS per size class)."""
import os
import re
import sys

import numpy as np
import pytest

import equity_range_spec as RS
import equity_ranged_spec as WS
import equity_spec as ES
import ev_spec as EV
import ranged_ev_spec as XS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pk_ev_ranged_d", "pk_ev_ranged", "pk_table_ev_ranged_d", "pk_table_ev_ranged")
U = WS.UNIFORM


@pytest.fixture(scope="module")
def lib():
    from pokerl_amd import _lib, build
    build.build_lib()
    return _lib


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def level_sums(r, where):
    """sum_p share[i][p] == 720720 * accepted for every level with amount > 0."""
    for i in range(len(r["amount"])):
        if r["amount"][i] > 0:
            assert int(r["share"][i].astype(object).sum()) == ES.SHARE_UNIT * int(r["accepted"]), (where, i)
        else:
            assert not r["share"][i].any(), (where, i)


def test_equal_bets_give_one_level_whose_share_is_the_ranged_equity():
    """Six seats, 8 random spots, S = 200, the four random_ranges rows mixed with 0xFFFF: with equal bets there is one level, and share[0] and
    accepted equal equity_ranged_spec.spot_equity's."""
    rng = np.random.default_rng(61)
    n, s = 6, 200
    four = WS.random_ranges(np.random.default_rng(1))
    holes, board, nboard, live = WS.random_spots(rng, n, 8)
    ro = rng.choice(np.array([0, 1, 2, 3, U], np.uint16), (8, n))
    some = 0
    for i in range(8):
        args = (holes[i], [int(x) for x in board[i]], int(nboard[i]), int(live[i]))
        got = XS.spot_ev(*args, np.full(n, 25.0), s, four, ro[i], nonce=2, ident=i)
        want = WS.spot_equity(*args, s, four, ro[i], nonce=2, ident=i)
        assert got["status"] == want["status"] == 0
        assert got["accepted"] == want["accepted"]
        assert (got["level_seat"] != XS.NO_LEVEL).sum() == 1 and got["amount"][0] == 150.0
        assert np.array_equal(got["share"][0], want["share"].astype(np.uint64)), i
        assert not got["share"][1:].any()
        level_sums(got, i)
        some += got["accepted"] > 0
    assert some >= 1                                                   # (the zero and one-holding rows accept little: not a vacuous identity)


def test_nothing_hidden_on_a_complete_board_is_the_shown_hands_ev():
    """Every attempt is the same showdown: share == S * ev_spec.spot_ev's share.  With integer bets ev is bit-equal to ev_spec.spot_ev's: both
    quotients (amount * S * share1) / (720720 * S) and (amount * share1) / 720720 are correctly rounded from the same real number as long as the
    products are exact, i.e. stay below 2^53 -- here amount <= 400, S * share1 <= 57 * 720720: below 2^35."""
    rng = np.random.default_rng(62)
    n, s = 5, 57
    holes, board, nboard, live = ES.random_spots(rng, n, 6, nb=5, unknown=False)
    for i in range(6):
        bets = XS.bet_patterns(n, live[i], i + 1).round()
        args = (holes[i], [int(x) for x in board[i]], 5, int(live[i]))
        got = XS.spot_ev(*args, bets, s, None, None, ident=i)
        want = EV.spot_ev(*args, bets)
        assert got["status"] == want["status"] == 0 and got["accepted"] == s and want["boards"] == 1
        assert float(np.max(want["amount"])) * s * ES.SHARE_UNIT < 2.0 ** 53
        assert np.array_equal(got["share"], s * want["share"])
        assert np.array_equal(got["level_seat"], want["level_seat"]) and np.array_equal(bits(got["amount"]), bits(want["amount"]))
        assert np.array_equal(bits(got["ev"]), bits(want["ev"])), (i, got["ev"], want["ev"])
        level_sums(got, i)


def test_one_holding_ranges_on_the_river_and_a_dead_holding():
    rng = np.random.default_rng(63)
    holes, board, nboard, live = ES.random_spots(rng, 3, 4, nb=5, unknown=False)
    bets = np.array([20.0, 10.0, 30.0])
    for i in range(4):
        bd = [int(x) for x in board[i]]
        want = EV.spot_ev(holes[i], bd, 5, 7, bets)
        w = np.zeros((2, WS.HOLDINGS), np.uint16)
        w[0, WS.holding_index(*holes[i, 1])] = 9
        w[1, WS.holding_index(*holes[i, 2])] = 1
        hid = holes[i].copy()
        hid[1:] = ES.UNKNOWN
        got = XS.spot_ev(hid, bd, 5, 7, bets, 37, w, [U, 0, 1], ident=i)
        assert got["accepted"] == 37 and got["status"] == 0
        assert np.array_equal(got["share"], 37 * want["share"]) and np.array_equal(bits(got["ev"]), bits(want["ev"]))
        # the one holding is a dead card's: nothing is accepted, status 0, ev all +0.0; the levels are still reported
        w[1] = 0
        w[1, WS.holding_index(holes[i, 0, 0], holes[i, 2, 1])] = 5
        dead = XS.spot_ev(hid, bd, 5, 7, bets, 37, w, [U, 0, 1], ident=i)
        assert dead["accepted"] == 0 and dead["status"] == 0 and not dead["share"].any()
        assert np.array_equal(bits(dead["ev"]), np.zeros(3, np.uint64))
        assert np.array_equal(dead["level_seat"], want["level_seat"])


def test_nonces_add_prefixes_and_merged():
    from pokerl_amd import judger as J
    holes, board, nb, live = XS.turn_spot()
    w = XS.turn_range()
    bets = np.array([10.0, 30.0])
    a, b = (XS.spot_ev(holes, board, nb, live, bets, 500, w, [U, 0], nonce=x) for x in (1, 2))
    assert a["accepted"] and b["accepted"] and (a["share"] != b["share"]).any()
    total = XS.merged(a, b, bets)
    level_sums(total, "sum")
    assert total["accepted"] == a["accepted"] + b["accepted"]
    want_ev = EV.ev_formula(a["amount"], total["share"], int(total["accepted"]), bets)
    assert np.array_equal(bits(total["ev"]), bits(want_ev))
    ra, rb = (J.RangedEV(x["ev"], x["share"], x["level_seat"], x["amount"], np.uint32(x["accepted"]), np.uint8(0), bets, 500) for x in (a, b))
    m = ra.merged(rb)
    assert np.array_equal(m.share, total["share"]) and int(m.accepted) == int(total["accepted"]) and m.samples == 1000
    assert np.array_equal(bits(m.ev), bits(want_ev))
    # a prefix of the stream: S = 300 is the first 300 attempts of S = 500
    _, _, took = WS.attempts(holes, board, nb, live, w, [U, 0], WS.R.seed_key(WS.DEFAULT_SEED), 0, 1, 500)
    first = XS.spot_ev(holes, board, nb, live, bets, 300, w, [U, 0], nonce=1)
    assert first["accepted"] == int((took < 300).sum()) and (first["share"] <= a["share"]).all()
    level_sums(first, "prefix")


def five_sigma(dev, bound, where):
    print(where, "deviation", np.asarray(dev).tolist(), "bound", np.asarray(bound).tolist())
    assert (np.asarray(dev) <= np.asarray(bound)).all(), (where, dev, bound)


def test_spec_converges_heads_up_on_the_turn():
    """Section 3.6's fixed turn spot under turn_range(), bets [10, 30], S = 16 384.  Exact hero EV = 2 b0 (agg0 + agg1 / 2) / agg2 - b0 from
    equity_range_spec.aggregate; the per-attempt fraction f of the 2 b0 level is in {0, 1/2, 1}, so Var f <= p (1 - p) with p = E f, and the
    bound is 5 * 2 b0 * sqrt(p (1 - p) / accepted).  Seed and nonce fixed: deterministic."""
    holes, board, nb, live = XS.turn_spot()
    w = XS.turn_range()
    agg = RS.aggregate(RS.spot_range(holes[0], board, nb), w)
    b0 = 10.0
    got = XS.spot_ev(holes, board, nb, live, [b0, 30.0], 16384, w, [U, 0])
    acc = got["accepted"]
    assert got["status"] == 0 and 0 < acc < 16384
    assert got["level_seat"].tolist() == [0, 1] and got["amount"].tolist() == [20.0, 20.0]
    p = (agg[0] + agg[1] / 2) / agg[2]
    exact = 2 * b0 * p - b0
    print("accepted", acc, "exact", exact, "sampled", got["ev"][0])
    five_sigma(abs(got["ev"][0] - exact), 5 * 2 * b0 * np.sqrt(p * (1 - p) / acc), "turn spot, hero EV:")
    assert abs(got["ev"].sum()) < 1e-9                                 # the pot is paid out in full


def test_spec_converges_three_seats_on_two_levels():
    """Hero shown on a complete board, two hidden seats with 40-holding ranges, bets [20, 10, 30]: two compared levels and a last stand,
    S = 4 096.  Exact mean and variance of each seat's per-attempt payout by host enumeration (ranged_ev_spec.three_seat_exact); the bound
    is 5 sqrt(var / accepted) per seat."""
    holes, board, nb, live, w, ro = XS.three_seat_spot()
    mean, var, pairs = XS.three_seat_exact()
    assert (mean > 0).all(), mean                                       # every seat's exact payout is non-zero
    got = XS.spot_ev(holes, board, nb, live, XS.THREE_BETS, 4096, w, ro)
    acc = got["accepted"]
    assert got["status"] == 0 and 0 < acc < 4096
    assert got["level_seat"].tolist() == [1, 0, 2] and got["amount"].tolist() == [30.0, 20.0, 10.0]
    payout = got["ev"] + np.array(XS.THREE_BETS)
    print("pairs", pairs, "accepted", acc, "exact", mean.tolist(), "sampled", payout.tolist())
    five_sigma(np.abs(payout - mean), 5 * np.sqrt(var / acc), "three seats, payouts:")


def test_spec_statuses():
    holes = np.array([[0x00, 0x01], [ES.UNKNOWN, ES.UNKNOWN], [0x12, ES.UNKNOWN]], np.uint8)
    board = [0x20, 0x21, 0x22, 0x23, 0x24]
    w = np.ones((2, WS.HOLDINGS), np.uint16)

    def run(lv, ro, r=w, bets=(5.0, 5.0, 5.0)):
        return XS.spot_ev(holes, board, 5, lv, np.array(bets), 8, r, ro)

    assert run(0b011, [0, 1, 0])["status"] == 0
    assert run(0b111, [0, 1, 0])["status"] == ES.BAD_CARD                      # seat 2 is live and shows one card
    assert run(0b011, [0, 2, 0])["status"] == ES.BAD_CARD                      # row 2 of 2 at the hidden seat
    assert run(0b011, [2, 1, 7])["status"] == 0                                # ... at a shown seat and at a seat that is not live: not read
    assert run(0b011, [0, 0, 0], None)["status"] == ES.BAD_CARD                # R = 0: no row at all
    assert run(0, [0, 1, 0])["status"] == ES.NO_LIVE
    for bad in (-1.0, float("nan"), float("inf")):
        r = run(0b011, [0, 1, 0], bets=(5.0, bad, 5.0))
        assert r["status"] == XS.BAD_BET and r["accepted"] == 0 and not r["share"].any() and (r["level_seat"] == XS.NO_LEVEL).all()
        assert np.array_equal(bits(r["ev"]), np.zeros(3, np.uint64)) and not r["amount"].any()
    assert run(0b111, [0, 1, 0], bets=(5.0, -1.0, 5.0))["status"] == ES.BAD_CARD | XS.BAD_BET
    assert run(0b011, [0, 1, 0], bets=(5.0, -0.0, 5.0))["status"] == 0         # -0.0 is a zero
    none = run(0b011, [0, 1, 0], bets=(0.0, -0.0, 0.0))                        # all bets 0: no level, ev all +0.0
    assert none["status"] == 0 and 0 < none["accepted"] <= 8 and (none["level_seat"] == XS.NO_LEVEL).all() and not none["share"].any()
    assert np.array_equal(bits(none["ev"]), np.zeros(3, np.uint64))


def test_header_declares_and_binding_lists_the_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "pokerl_hip.h")).read()
    import ctypes
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in lib.SYMBOLS and hasattr(L, name), name
    assert lib.lib().pk_abi_version() == 6
    assert "Ranged showdown EV" in header
    for define in ("PK_EQ_BAD_BET", "PK_EQW_MAX_RANGES", "PK_EQW_UNIFORM"):      # reused, not redefined
        assert len(re.findall(r"#define %s\b" % define, header)) == 1, define
    assert lib.EQ_BAD_BET == XS.BAD_BET == 64


def test_bad_arguments_are_refused_without_a_device(lib):
    L = lib.lib()
    one = np.zeros(64, np.uint8)
    p = lib.ptr(one)

    def explicit(n, m, samples, ranges=0, weights=None, bets=p, status=p):
        a = L.pk_ev_ranged(0, n, m, p, p, p, p, bets, None, samples, 1, 0, weights, ranges, None, None, None, None, None, None, status)
        b = L.pk_ev_ranged_d(0, n, m, p, p, p, p, bets, None, samples, 1, 0, weights, ranges, None, None, None, None, None, None, status, None)
        return a, b

    bad = (lib.PK_E_INVALID_ARG, lib.PK_E_INVALID_ARG)
    for n in (1, 17, -3):
        assert explicit(n, 1, 64) == bad
    assert b"pk_ev_ranged_d" in L.pk_last_error(None)
    for samples in (0, 2 ** 24 + 1):
        assert explicit(6, 1, samples) == bad
        assert b"pk_ev_ranged_d" in L.pk_last_error(None) and b"samples" in L.pk_last_error(None)
    assert explicit(6, 1, 64, 17, p) == bad
    assert b"pk_ev_ranged_d" in L.pk_last_error(None) and b"num_ranges" in L.pk_last_error(None)
    assert explicit(6, 1, 64, 4, None) == bad                                   # rows without weights
    assert b"pk_ev_ranged_d" in L.pk_last_error(None) and b"NULL weights" in L.pk_last_error(None)
    assert explicit(6, 1, 64, bets=None) == bad
    assert b"pk_ev_ranged_d" in L.pk_last_error(None) and b"NULL" in L.pk_last_error(None)
    assert explicit(6, 1, 64, status=None) == bad
    assert b"pk_ev_ranged_d" in L.pk_last_error(None) and b"NULL status" in L.pk_last_error(None)
    assert explicit(2, 2 ** 14, 2 ** 24) == bad                                 # one group: 2^14 * 2^18 tasks
    assert b"pk_ev_ranged_d" in L.pk_last_error(None) and b"32 bits" in L.pk_last_error(None)
    assert explicit(16, 2 ** 11, 2 ** 24) == bad                                # eight groups: 2^11 * 2^18 * 8
    assert b"32 bits" in L.pk_last_error(None)
    for observer in (lib.OBSERVER_NONE, 0, lib.OBSERVER_ACTIVE):
        assert L.pk_table_ev_ranged_d(None, None, 4, observer, 64, 0, None, 0, None, 0, None, None, None, None, None, p) == lib.PK_E_INVALID_ARG
        assert L.pk_table_ev_ranged(None, None, 4, observer, 64, 0, None, 0, None, 0, None, None, None, None, None, p) == lib.PK_E_INVALID_ARG


def test_python_helpers_validate_before_any_device_call(lib):
    from pokerl_amd import judger as J
    import pokerl_amd
    for name in ("RangedEV", "ranged_ev", "ranged_ev_batch", "ranged_ev_d"):
        assert getattr(pokerl_amd, name) is getattr(J, name) and name in pokerl_amd.__all__, name
    hu = [["AS", "KS"], None]
    w = np.ones(1326, np.uint16)
    ok = dict(bets=[10, 30])
    for bad in (dict(samples=0), dict(samples=2 ** 24 + 1), dict(nonce=-1), dict(nonce=2 ** 32), dict(board=["2S"] * 6), dict(live=0b100),
                dict(ranges=np.ones(1325)), dict(ranges=np.ones((17, 1326))), dict(ranges=w, range_of=[0, 0, 0]), dict(ranges=w, range_of=[0, 70000]),
                dict(bets=None), dict(bets=[10]), dict(bets=[10, 20, 30]), dict(bets=[10, -1]), dict(bets=[10, float("nan")]),
                dict(bets=[float("inf"), 1]), dict(bets=7)):
        with pytest.raises(ValueError):
            J.ranged_ev(hu, **dict(ok, **bad))
    with pytest.raises(ValueError):
        J.ranged_ev([["AS", "KS"], ["QD", None]], **ok)                     # half a holding
    with pytest.raises(ValueError):
        J.ranged_ev_batch(np.zeros((2, 3, 2), np.uint8), np.zeros((2, 5), np.uint8), np.zeros(2, np.uint8), np.ones(2, np.uint16), np.zeros((2, 2)))
    with pytest.raises(ValueError):
        J.ranged_ev_batch(np.zeros((2, 3, 2), np.uint8), np.zeros((2, 5), np.uint8), np.zeros(2, np.uint8), np.ones(2, np.uint16), None)
    with pytest.raises(ValueError):
        J.ranged_ev_d(6, 3, 1, 1, 1, 1, 1, samples=64, status_d=1, num_ranges=17)
    with pytest.raises(ValueError):
        J.ranged_ev_d(17, 3, 1, 1, 1, 1, 1, samples=64, status_d=1)
    with pytest.raises(ValueError):
        J.ranged_ev_d(6, 3, 1, 1, 1, 1, 1, samples=64, status_d=None)
    from pokerl_amd.game import VecGame
    from pokerl_amd.single import Game
    fake = VecGame.__new__(VecGame)                                         # no handle: validation must come before any call
    fake.num_players, fake.num_tables = 6, 4
    for bad in (dict(observer=6), dict(observer=None), dict(observer=lib.OBSERVER_NONE), dict(samples=0), dict(nonce=2 ** 32),
                dict(ranges=np.ones((17, 1326))), dict(ranges=w, range_of=np.zeros((3, 6)))):
        with pytest.raises(ValueError):
            fake.ev_ranged(**bad)
    for bad in (dict(observer=6), dict(observer=lib.OBSERVER_NONE), dict(samples=0), dict(num_ranges=17), dict(status_d=None)):
        with pytest.raises(ValueError):
            fake.ev_ranged_d(**dict(dict(status_d=1), **bad))
    assert hasattr(Game, "ev_ranged")
    # RangedEV's own arithmetic: payout, levels, acceptance, indexing
    e = J.RangedEV(np.array([[5.0, -5.0]]), np.array([[[3 * 720720, 720720], [0, 4 * 720720]]], np.uint64), np.array([[0, 1]], np.uint8),
                   np.array([[20.0, 20.0]]), np.array([4], np.uint32), np.array([0], np.uint8), np.array([[10.0, 30.0]]), 8)
    assert e.payout.tolist() == [[15.0, 25.0]] and e[0].payout.tolist() == [15.0, 25.0] and e.acceptance.tolist() == [0.5]
    assert e.levels == [[(0, 20.0), (1, 20.0)]] and e[0].levels == [(0, 20.0), (1, 20.0)]
    assert np.array_equal(J.ranged_ev_formula(e.amount[0], e.share[0], 4, e.bets[0]), e.ev[0])
    assert np.array_equal(bits(J.ranged_ev_formula(e.amount[0], e.share[0], 0, e.bets[0])), np.zeros(2, np.uint64))


CU_LDS = 160 * 1024


def eqw_lds_bytes(rc):
    """pk::eqw_lds_bytes: the evaluator table, RC cumulative rows, the holding table, 32 share words."""
    return 32768 + rc * 5304 + 2652 + 128


SCRATCH_ALLOWED = {}     # kernel name -> reason, for N = 9 .. 16 only; empty: none needs it


def test_kernels_have_no_scratch_no_vgpr_spill_and_fit_the_lds_classes(lib):
    from pokerl_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(lib.LIB_PATH)
    evw = {k: d for k, d in ks.items() if k.startswith("k_evw")}
    names = (["k_evw_finish"] + ["k_evw_prep<%d, %s>" % (n, t) for n in build.SEATS for t in ("true", "false")]
             + ["k_evw<%d, %d>" % (n, rc) for n in build.SEATS for rc in (0, 8, 16)])
    assert sorted(evw) == sorted(names), sorted(set(evw) ^ set(names))
    for k, d in evw.items():
        n = int(re.search(r"<(\d+)", k).group(1)) if "<" in k else 0
        if k in SCRATCH_ALLOWED:
            assert n >= 9, k
            continue
        assert d["private_segment"] == 0 and d["vgpr_spill"] == 0, (k, d)
    for n in build.SEATS:
        for rc in (0, 8, 16):
            assert evw["k_evw<%d, %d>" % (n, rc)]["lds"] <= eqw_lds_bytes(rc) + 64, (n, rc)
    assert 4 * (eqw_lds_bytes(0) + 64) <= CU_LDS and 2 * (eqw_lds_bytes(8) + 64) <= CU_LDS and eqw_lds_bytes(16) + 64 <= CU_LDS
    assert "pk_ev_ranged.hip" in build.SOURCES and any(h.endswith("pk_ev_ranged.hpp") for h in build.HEADERS)
