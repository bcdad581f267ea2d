"""CPU tests of the sampled showdown equity (no GPU): the entry points in the header and the binding, the new kernels in the built library's
code objects, argument validation in the C ABI and in the Python helpers, and the Python restatement of the definition
(tests/equity_sampled_spec.py) checked against itself and against the exact enumeration of tests/equity_spec.py."""
import math
import os
import re
import sys

import numpy as np
import pytest

import equity_sampled_spec as SS
import equity_spec as ES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pk_equity_sampled_d", "pk_equity_sampled", "pk_table_equity_sampled_d", "pk_table_equity_sampled")


@pytest.fixture(scope="module")
def lib():
    from pokerl_amd import _lib, build
    build.build_lib()
    return _lib


def turn_spot():
    """Hero AS AD against one hidden hand on KS 7D 7C 2H: (holes, board, nb, live)."""
    from pokerl_amd.cards import card_value as cv
    holes = np.array([[cv("AS"), cv("AD")], [ES.UNKNOWN, ES.UNKNOWN]], np.uint8)
    return holes, [cv("KS"), cv("7D"), cv("7C"), cv("2H"), 0], 4, 0b11


def turn_spot_exact():
    """Exact win probabilities [2] of turn_spot: every one of the C(46, 2) = 1 035 opponent hands, each with the same 44 rivers."""
    holes, board, nb, live = turn_spot()
    dead = {int(holes[0, 0]), int(holes[0, 1])} | set(board[:4])
    pool = [c for c in ES.CANON if c not in dead]
    win, boards = np.zeros(2, np.int64), 0
    for i in range(len(pool)):
        for j in range(i + 1, len(pool)):
            r = ES.spot_equity(np.array([holes[0], [pool[i], pool[j]]], np.uint8), board, nb, live)
            assert r["status"] == 0 and r["boards"] == 44
            win += r["win"]
            boards += r["boards"]
    assert boards == 1035 * 44
    return win / boards


def test_header_declares_and_binding_lists_the_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "pokerl_hip.h")).read()
    import ctypes
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in lib.SYMBOLS and hasattr(L, name), name
    assert lib.lib().pk_abi_version() == 6
    assert lib.EQS_SAMPLES_MAX == SS.SAMPLES_MAX == 1 << 24
    assert "0x45515330" in header and SS.STREAM_EQS == int.from_bytes(b"EQS0", "big")


def test_sampled_kernels_exist_without_scratch(lib):
    """`.private_segment_fixed_size` == 0 for the preparation kernels and for the sampling kernel of every seat count, and the sampling
    kernel's LDS (the 32 KB table and little else) lets four workgroups share a CU."""
    from pokerl_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(lib.LIB_PATH)
    names = ["k_eqs_prep<true>", "k_eqs_prep<false>"] + ["k_eqs<%d>" % n for n in build.SEATS]
    eqs = {k: d for k, d in ks.items() if k.startswith("k_eqs")}
    assert sorted(eqs) == sorted(names), sorted(eqs)
    assert build.SEATS == list(range(2, 17))
    assert all(d["private_segment"] == 0 for d in eqs.values()), {k: d["private_segment"] for k, d in eqs.items()}
    assert all(32768 < eqs["k_eqs<%d>" % n]["lds"] <= 40960 for n in build.SEATS)


def test_bad_arguments_are_refused_without_a_device(lib):
    L = lib.lib()
    one = np.zeros(64, np.uint8)
    p = lib.ptr(one)

    def explicit(n, m, samples, holes=p):
        a = L.pk_equity_sampled(0, n, m, holes, p, p, p, None, samples, 1, 0, None, None, None, None, None)
        b = L.pk_equity_sampled_d(0, n, m, holes, p, p, p, None, samples, 1, 0, None, None, None, None, None, None)
        return a, b

    for n in (1, 17, -3):
        assert explicit(n, 1, 64) == (lib.PK_E_INVALID_ARG, lib.PK_E_INVALID_ARG)
    assert b"pk_equity_sampled_d" in L.pk_last_error(None)
    for samples in (0, 2 ** 24 + 1, 2 ** 32 - 1):
        assert explicit(6, 1, samples) == (lib.PK_E_INVALID_ARG, lib.PK_E_INVALID_ARG)
        assert b"pk_equity_sampled_d" in L.pk_last_error(None) and b"samples" in L.pk_last_error(None)
    assert explicit(6, 1, 64, None) == (lib.PK_E_INVALID_ARG, lib.PK_E_INVALID_ARG)
    assert b"NULL" in L.pk_last_error(None)
    # m * ceil(samples / 64) must fit 32 bits: 2^14 * 2^18 = 2^32 does not, one spot less does
    assert explicit(2, 2 ** 14, 2 ** 24) == (lib.PK_E_INVALID_ARG, lib.PK_E_INVALID_ARG)
    assert b"32 bits" in L.pk_last_error(None)
    assert explicit(2, 2 ** 31, 1) == (lib.PK_E_INVALID_ARG, lib.PK_E_INVALID_ARG)
    assert L.pk_equity_sampled_d(64, 2, 1, p, p, p, p, None, 64, 1, 0, None, None, None, None, None, None) != lib.PK_OK
    for observer in (16, 0, lib.OBSERVER_ACTIVE, -3):
        assert L.pk_table_equity_sampled_d(None, None, 4, observer, 64, 0, None, None, None, None, None) == lib.PK_E_INVALID_ARG
        assert L.pk_table_equity_sampled(None, None, 4, observer, 64, 0, None, None, None, None, None) == lib.PK_E_INVALID_ARG


def test_python_helpers_validate_before_any_device_call(lib):
    from pokerl_amd import judger as J
    import pokerl_amd
    assert pokerl_amd.SampledEquity is J.SampledEquity and pokerl_amd.sampled_equity is J.sampled_equity
    assert pokerl_amd.sampled_equity_batch is J.sampled_equity_batch
    hu = [["AS", "KS"], None]
    for bad in (dict(samples=0), dict(samples=2 ** 24 + 1), dict(nonce=-1), dict(nonce=2 ** 32), dict(board=["2S"] * 6), dict(live=[0, 2]),
                dict(live=0b100)):
        with pytest.raises(ValueError):
            J.sampled_equity(hu, **bad)
    with pytest.raises(ValueError):
        J.sampled_equity([["AS", "KS"]])                                    # one seat
    with pytest.raises(ValueError):
        J.sampled_equity([["AS", "KS"], ["QD"]])                            # one hole card
    with pytest.raises(ValueError):
        J.sampled_equity([["AS", "KS"], [0x4F, None]])                      # not a card
    z5, z = np.zeros((3, 5)), np.zeros(3)
    with pytest.raises(ValueError):
        J.sampled_equity_batch(np.zeros((3, 6, 3), np.uint8), z5, z, z)
    with pytest.raises(ValueError):
        J.sampled_equity_batch(np.zeros((3, 17, 2), np.uint8), z5, z, z)
    with pytest.raises(ValueError):
        J.sampled_equity_batch(np.zeros((3, 6, 2), np.uint8), np.zeros((3, 4)), z, z)
    with pytest.raises(ValueError):
        J.sampled_equity_batch(np.zeros((3, 6, 2), np.uint8), z5, z, z, ids=np.zeros(4))
    with pytest.raises(ValueError):
        J.sampled_equity_batch(np.zeros((3, 6, 2), np.uint8), z5, z, z, samples=0)
    with pytest.raises(ValueError):
        J.sampled_equity_d(6, 3, 1, 1, 1, 1, samples=2 ** 24 + 1)
    with pytest.raises(ValueError):
        J.sampled_equity_d(17, 3, 1, 1, 1, 1, samples=64)
    from pokerl_amd.game import VecGame
    from pokerl_amd.single import Game
    fake = VecGame.__new__(VecGame)                                         # no handle: validation must come before any call
    fake.num_players, fake.num_tables = 6, 4
    for bad in (dict(observer=6), dict(observer=-3), dict(samples=0), dict(samples=2 ** 24 + 1), dict(nonce=2 ** 32)):
        with pytest.raises(ValueError):
            fake.equity_sampled(**bad)
        with pytest.raises(ValueError):
            fake.equity_sampled_d(**bad)
    assert hasattr(Game, "equity_sampled")
    e = J.SampledEquity(np.array([[3, 0]], np.uint32), np.array([[1, 1]], np.uint32), np.array([[3 * 720720 + 360360, 360360]], np.uint64),
                        np.array([4], np.uint32), np.array([0], np.uint8))
    assert e.equity.tolist() == [[0.875, 0.125]] and e[0].equity.tolist() == [0.875, 0.125]
    assert np.allclose(e.stderr, [[0.0, math.sqrt(0.25 * 0.75 / 4)]])
    refused = J.SampledEquity(np.zeros((1, 2), np.uint32), np.zeros((1, 2), np.uint32), np.zeros((1, 2), np.uint64), np.array([0], np.uint32),
                              np.array([2], np.uint8))
    assert not refused.equity.any() and not refused.stderr.any()


@pytest.mark.parametrize("n", [2, 6, 16])
def test_spec_draws_are_distinct_and_never_a_known_card(n):
    rng = np.random.default_rng(40 + n)
    holes, board, nboard, live = SS.random_spots(rng, n, 20)
    live[0] = (1 << n) - 1
    holes[0] = ES.UNKNOWN                                                   # all live, all hidden: D = 5 - nb + 2N
    nboard[0] = 0
    key = SS.R.seed_key(SS.DEFAULT_SEED)
    total = 0
    for i in range(20):
        status, dead, lv, hidden = SS.check_spot(holes[i], board[i], int(nboard[i]), int(live[i]))
        assert status == 0
        hands, _ = SS.sample_cards(holes[i], [int(x) for x in board[i]], int(nboard[i]), int(live[i]), key, 1000 + i, 5, 100)
        total += 100
        nb = int(nboard[i])
        for s in range(100):
            cards = [int(c) for c in hands[s, 0, :5]] + [int(c) for p in range(n) for c in hands[s, p, 5:] if c != ES.UNKNOWN]
            assert len(set(cards)) == len(cards) and all(c in ES.CANON for c in cards)
            drawn = [int(c) for c in hands[s, 0, nb:5]] + [int(hands[s, p, 5 + b]) for p, b in hidden]
            assert not set(drawn) & dead and len(drawn) == 5 - nb + len(hidden)
        assert (hands[:, :, :nb] == board[i][:nb]).all()
        known = holes[i] != ES.UNKNOWN
        assert (hands[:, :, 5:][:, known] == holes[i][known]).all()
    assert total == 2000
    if n == 16:
        assert len(SS.check_spot(holes[0], board[0], 0, int(live[0]))[3]) + 5 == 37


def test_spec_with_everything_known_is_the_exact_count_times_samples():
    rng = np.random.default_rng(3)
    for n in (2, 6, 9):
        holes, board, nboard, live = ES.random_spots(rng, n, 4, nb=5, unknown=False)
        for i in range(4):
            exact = ES.spot_equity(holes[i], [int(x) for x in board[i]], 5, int(live[i]))
            got = SS.spot_equity(holes[i], [int(x) for x in board[i]], 5, int(live[i]), 37, ident=i)
            assert exact["boards"] == 1 and got["samples"] == 37 and got["status"] == 0
            for k in ("win", "tie", "share"):
                assert (got[k].astype(np.uint64) == 37 * exact[k].astype(np.uint64)).all(), (n, i, k)


def test_spec_statuses_are_equity_specs_except_hidden_bytes_at_live_seats():
    holes = np.array([[0x00, 0x01], [0x12, 0x13], [ES.UNKNOWN, ES.UNKNOWN]], np.uint8)
    board = [0x20, 0x21, 0x22, 0x23, 0x24]

    def both(h, b, nb, lv):
        return ES.spot_equity(np.array(h, np.uint8), b, nb, lv)["status"], SS.spot_equity(np.array(h, np.uint8), b, nb, lv, 8)["status"]

    assert both(holes, board, 5, 0b011) == (0, 0)
    assert both(holes, board, 5, 0b111) == (ES.BAD_CARD, 0)                  # hidden cards at a live seat: the one difference
    assert both([[0x00, ES.UNKNOWN], [0x12, 0x13], [0x05, 0x06]], board, 5, 0b111) == (ES.BAD_CARD, 0)   # ... a single byte
    assert both(holes, board, 5, 0) == (ES.NO_LIVE, ES.NO_LIVE)
    assert both(holes, board, 5, 0b111000) == (ES.NO_LIVE, ES.NO_LIVE)
    assert both(holes, board, 6, 0b011) == (ES.BAD_NBOARD, ES.BAD_NBOARD)
    assert both(holes, board, 6, 0b111) == (ES.BAD_NBOARD | ES.BAD_CARD, ES.BAD_NBOARD)
    assert both(holes, [0x20, 0x20, 0x22, 0x23, 0x24], 5, 0b111) == (ES.DUP_CARD | ES.BAD_CARD, ES.DUP_CARD)
    assert both(holes, [0x20, 0x20, 0x22, 0x23, 0x24], 1, 0b011) == (0, 0)
    assert both(holes, [0x2D, 0x21, 0x22, 0x23, 0x24], 5, 0b111) == (ES.BAD_CARD, ES.BAD_CARD)
    assert both(holes, [ES.UNKNOWN, 0x21, 0x22, 0x23, 0x24], 5, 0b111) == (ES.BAD_CARD, ES.BAD_CARD)     # 0xFF in the board stays refused
    assert both([[0x00, 0x01], [0x4F, 0x13], [ES.UNKNOWN, ES.UNKNOWN]], board, 5, 0b101) == (ES.BAD_CARD, ES.BAD_CARD)
    assert both([[0x00, 0x00], [0x12, 0x13], [ES.UNKNOWN, 0x05]], board, 5, 0b100) == (ES.DUP_CARD | ES.BAD_CARD, ES.DUP_CARD)
    r = SS.spot_equity(holes, [0x00, 0x21, 0x22, 0x23, 0x24], 5, 0b111, 8)
    assert r["status"] == ES.DUP_CARD and r["samples"] == 0 and not r["win"].any() and not r["share"].any()
    rng = np.random.default_rng(8)
    for n in (2, 6, 16):                                                     # and on random spots with nothing hidden: the same word
        h, b, nb, lv = ES.random_spots(rng, n, 30)
        for i in range(30):
            assert SS.check_spot(h[i], b[i], int(nb[i]), int(lv[i]))[0] == ES.check_spot(h[i], b[i], int(nb[i]), int(lv[i]))[0]


def test_spec_table_spots_hide_what_the_observer_cannot_see():
    rng = np.random.default_rng(2)
    t, n = 50, 6
    deck = np.array([[ES.CANON[c] for c in rng.permutation(52)[:5 + 2 * n]] for _ in range(t)], np.uint8)
    ps = rng.integers(0, 5, (t, n))
    turn, active = rng.integers(0, 5, t), rng.integers(0, n, t)
    plain = ES.table_spots(deck, ps, turn)
    for a, b in zip(SS.table_spots(deck, ps, turn, active, SS.OBSERVER_NONE), plain):
        assert (a == b).all()
    for observer in (SS.OBSERVER_ACTIVE, 3):
        holes, board, nboard, live = SS.table_spots(deck, ps, turn, active, observer)
        assert (board == plain[1]).all() and (nboard == plain[2]).all() and (live == plain[3]).all()
        for i in range(t):
            who = int(active[i]) if observer == SS.OBSERVER_ACTIVE else 3
            assert (holes[i, who] == plain[0][i, who]).all() and (np.delete(holes[i], who, axis=0) == ES.UNKNOWN).all()


def test_spec_converges_to_the_exact_turn_equity():
    """S = 16 384 samples of the turn spot against the exact mixture over the 1 035 opponent hands: |win / S - p| <= 5 sqrt(p (1 - p) / S)
    per seat -- five binomial standard deviations, derived; seed and nonce are fixed, so the outcome is deterministic."""
    p = turn_spot_exact()
    holes, board, nb, live = turn_spot()
    s = 16384
    got = SS.spot_equity(holes, board, nb, live, s, seed=SS.DEFAULT_SEED, nonce=0, ident=0)
    assert got["status"] == 0 and got["samples"] == s
    dev = np.abs(got["win"] / s - p)
    bound = 5 * np.sqrt(p * (1 - p) / s)
    print("turn spot: exact", p, "sampled", got["win"] / s, "deviation", dev, "bound", bound)
    assert (dev <= bound).all(), (dev, bound)
    assert int(got["share"].astype(object).sum()) == ES.SHARE_UNIT * s
