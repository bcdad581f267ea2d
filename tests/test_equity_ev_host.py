"""CPU tests of the showdown EV (no GPU): the numpy restatement of the definition (tests/ev_spec.py) against the fixture the reference's own
Game.end_hand wrote (tests/golden/ev_ref.json), the new entry points in the header and the binding, the new kernels in the built library's
code objects, and the argument validation of the Python helpers."""
import json
import os
import re
import sys

import numpy as np
import pytest

import equity_spec as ES
import ev_spec as EV
import ev_witness as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ev_ref.json")
ENTRY_POINTS = ("pk_equity_ev_d", "pk_equity_ev", "pk_table_equity_ev_d", "pk_table_equity_ev")
# kernel -> (private-segment bytes, reason): kernels of this family at 9 .. 16 seats that may use scratch.  None does.
EV_SCRATCH_ALLOWED = {}


def fixture_spots():
    with open(FIXTURE) as f:
        ref = json.load(f)
    assert ref["share_unit"] == EV.SHARE_UNIT
    return ref["spots"]


def spot_inputs(s):
    board = s["board"] + [0] * (5 - len(s["board"]))
    return np.array(s["holes"], np.uint8), board, len(s["board"]), s["live"], np.array(s["bets"], np.float64)


@pytest.fixture(scope="module")
def lib():
    from pokerl_amd import _lib, build
    build.build_lib()
    return _lib


def test_fixture_is_data_only_and_small():
    assert os.path.getsize(FIXTURE) <= 1 << 20
    with open(FIXTURE) as f:
        ref = json.load(f)
    assert set(ref) == {"share_unit", "bets_from", "end_hand_calls", "spots"} and 2000 <= ref["end_hand_calls"] <= 10000

    def plain(x):      # numbers, hex-float strings and containers of them: nothing a program could read as code
        if isinstance(x, dict):
            return all(isinstance(k, str) and plain(v) for k, v in x.items())
        if isinstance(x, list):
            return all(plain(v) for v in x)
        return isinstance(x, (int, float)) or (isinstance(x, str) and re.fullmatch(r"-?0x[01]\.[0-9a-f]+p[+-]\d+", x) is not None)
    assert plain(ref)
    spots = ref["spots"]
    assert {s["n"] for s in spots} == set(range(2, 10)) and {len(s["board"]) for s in spots} == {3, 4, 5}
    assert sum(s["boards"] for s in spots) == ref["end_hand_calls"]
    for s in spots:
        assert set(s["bets"]) <= set(ref["bets_from"]) and (("payoffs" in s) == (len(s["board"]) == 5)) and (("mean" in s) != ("payoffs" in s))
    many = [s for s in spots if len({b for p, b in enumerate(s["bets"]) if (s["live"] >> p) & 1}) > 1]
    assert len(many) >= 30


def test_spec_equals_reference_fixture():
    for i, s in enumerate(fixture_spots()):
        got = EV.spot_ev(*spot_inputs(s))
        assert got["status"] == 0 and got["boards"] == s["boards"], i
        EV.check_against_reference(got["ev"], s, i)
        lv = EV.levels(np.array(s["bets"]), s["live"])
        assert float(np.sum(got["amount"])) == float(np.sum(np.array(s["bets"]))) or not lv     # (integer money: the levels pay the pot out)
        for j, (seat, amount, remain, last) in enumerate(lv):
            if amount > 0:
                assert int(np.sum(got["share"][j])) == EV.SHARE_UNIT * s["boards"], (i, j)


def test_line_148_spot_needs_its_own_comparison_per_level():
    """Fixture spot 0: three live seats of one rank class, the lowest bettor first with the lowest kicker.  W_1 is not W_0 restricted to
    remain_1: the first hand of the best rank class fixes best_kicker, and that hand is gone at level 1."""
    s = fixture_spots()[0]
    holes, board, nb, live, bets = spot_inputs(s)
    assert nb == 5 and live == 0b111 and np.argmin(bets) == 0
    lv = EV.levels(bets, live)
    assert [x[0] for x in lv][0] == 0 and lv[1][2] == 0b110
    rank, kick = EV.spot_rankings(holes, board, nb, live, ES.check_spot(holes, board, nb, live)[1])
    assert len(set(int(r) for r in rank[:, 0])) == 1 and kick[0, 0] < kick[2, 0] < kick[1, 0]
    w0, w1 = int(EV.level_winners(rank, kick, lv[0][2])[0]), int(EV.level_winners(rank, kick, lv[1][2])[0])
    assert w1 != (w0 & lv[1][2]) and w0 == 0b100 and w1 == 0b010


def test_spec_levels():
    assert EV.levels([10, 10, 10], 0b111) == [(0, 30.0, 0b111, False)]                        # equal bets: one level carries all the money
    assert [(s, a) for s, a, _, _ in EV.levels([30, 10, 20], 0b111)] == [(1, 30.0), (2, 20.0), (0, 10.0)]
    assert EV.levels([30, 10, 20], 0b111)[2][3]                                               # the top bettor's excess: the last stand
    assert EV.levels([0, 10, 10], 0b111) == [(0, 0.0, 0b111, False), (1, 20.0, 0b110, False)]   # a live seat with bet 0: a level of amount 0
    assert EV.levels([10, 50, 10], 0b101) == [(0, 30.0, 0b101, False), (2, 40.0, 0b100, True)]   # dead money: to the last seat in (stable) order
    assert EV.levels([5, 7, 9], 0b010) == [(1, 21.0, 0b010, True)]                            # one live seat
    assert EV.levels([0, 0, 0], 0b111) == [] and EV.levels([0, 0], 0b01) == []
    r = EV.spot_ev(np.array([[0x00, 0x01], [0x12, 0x13]], np.uint8), [0x20, 0x21, 0x22, 0x23, 0x24], 5, 0b11, [1.0, -1.0])
    assert r["status"] == EV.BAD_BET and r["boards"] == 0 and not r["ev"].any() and (r["level_seat"] == EV.NO_LEVEL).all()
    for bad in (float("nan"), float("inf")):
        assert EV.spot_ev(np.array([[0x00, 0x01], [0x12, 0x13]], np.uint8), [0x20, 0x21, 0x22, 0x23, 0x24], 5, 0b11, [1.0, bad])["status"] == EV.BAD_BET


@pytest.mark.parametrize("shape", sorted(W.WITNESS))
def test_the_oracle_game_pays_what_the_spec_expects(shape):
    """The game itself as witness, on the CPU: the C oracle's tables at the start of the river's betting round, the spec's ev of the table
    form's spot, then the hand played out by seats that check -- the payoffs end_hand pays equal that ev bit for bit.  The seeds are the ones the
    GPU test uses: at least one such table has a side pot (three live seats, two distinct live bet levels)."""
    from oracle import loader as O
    tables, n = shape
    seed, steps = W.WITNESS[shape]
    b = O.OracleGame(tables, n, start_credits=W.ladder_stacks(n), seed=seed)
    snap = W.deep_steps(b, steps)
    holes, board, nboard, live, bets = W.spots_of(snap)
    ll = W.live_levels(live, bets)
    assert any(a >= 3 and c >= 2 for a, c in ll)
    cand = W.river_candidates(snap)
    assert any(ll[t][0] >= 3 and ll[t][1] >= 2 for t in cand), [ll[t] for t in cand]
    want = {t: EV.spot_ev(holes[t], [int(x) for x in board[t]], int(nboard[t]), int(live[t]), bets[t]) for t in cand}
    assert all(w["status"] == 0 and w["boards"] == 1 for w in want.values())
    paid = W.play_out_passively(b, cand)
    for t in cand:
        assert np.array_equal(paid[t].view(np.uint64), want[t]["ev"].view(np.uint64)), (t, paid[t], want[t]["ev"], bets[t])


def test_header_declares_and_binding_lists_the_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "pokerl_hip.h")).read()
    import ctypes
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in lib.SYMBOLS and hasattr(L, name), name
    declared = set(re.findall(r"\bint (pk_\w*equity_ev\w*)\s*\(", header))
    assert declared == set(ENTRY_POINTS) == {s for s in lib.SYMBOLS if "equity_ev" in s}
    assert re.search(r"#define PK_EQ_BAD_BET %du\b" % EV.BAD_BET, header) and lib.EQ_BAD_BET == EV.BAD_BET == lib.EQ_PREFLOP
    assert lib.lib().pk_abi_version() == 6


def test_ev_kernels_exist_without_scratch(lib):
    """`.private_segment_fixed_size` == 0 for every kernel of the family at N <= 8; at 9 .. 16 the same, or the allow-list names the kernel."""
    from pokerl_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(lib.LIB_PATH)
    names = ["k_ev_finish"] + ["k_ev<%d>" % n for n in build.SEATS] + ["k_ev_prep<%d, %s>" % (n, t) for n in build.SEATS for t in ("true", "false")]
    ev = {k: d for k, d in ks.items() if re.match(r"k_ev(_prep|_finish)?(<|$)", k)}
    assert sorted(ev) == sorted(names), sorted(ev)
    for k, d in ev.items():
        m = re.search(r"<(\d+)", k)
        n = int(m.group(1)) if m else 0
        if k in EV_SCRATCH_ALLOWED:
            assert n > 8 and d["private_segment"] == EV_SCRATCH_ALLOWED[k][0] > 0, (k, d)
        else:
            assert d["private_segment"] == 0 and d["vgpr_spill"] == 0, (k, d)
    assert all(32768 < ev["k_ev<%d>" % n]["lds"] <= 40960 for n in build.SEATS)               # four workgroups share a CU, as k_equity


def test_null_arguments_are_refused_without_a_device(lib):
    L = lib.lib()
    one = np.zeros(64, np.uint8)
    p = lib.ptr(one)
    assert L.pk_table_equity_ev_d(None, None, 4, None, None, None, None, None, p) == lib.PK_E_INVALID_ARG
    assert L.pk_table_equity_ev(None, None, 4, None, None, None, None, None, p) == lib.PK_E_INVALID_ARG
    for n in (1, 17, -3):
        assert L.pk_equity_ev(0, n, 1, p, p, p, p, p, None, None, None, None, None, p) == lib.PK_E_INVALID_ARG
        assert L.pk_equity_ev_d(0, n, 1, p, p, p, p, p, None, None, None, None, None, p, None) == lib.PK_E_INVALID_ARG
    assert L.pk_equity_ev(0, 6, 1, p, p, p, p, None, None, None, None, None, None, p) == lib.PK_E_INVALID_ARG        # no bets
    assert L.pk_equity_ev(0, 6, 1, p, p, p, p, p, None, None, None, None, None, None) == lib.PK_E_INVALID_ARG        # no status
    assert b"pk_equity_ev" in L.pk_last_error(None)
    assert L.pk_equity_ev_d(0, 2, 2 ** 31 - 1, p, p, p, p, p, None, None, None, None, None, p, None) == lib.PK_E_INVALID_ARG
    assert b"too many spots" in L.pk_last_error(None)


def test_python_helpers_validate_before_any_device_call(lib):
    from pokerl_amd import judger as J
    import pokerl_amd
    for name in ("ShowdownEV", "showdown_ev", "showdown_ev_batch", "showdown_ev_d"):
        assert getattr(pokerl_amd, name) is getattr(J, name) and name in pokerl_amd.__all__
    assert hasattr(pokerl_amd.VecGame, "equity_ev") and hasattr(pokerl_amd.VecGame, "equity_ev_d") and hasattr(pokerl_amd.Game, "equity_ev")
    two = [["AS", "KS"], ["QD", "QC"]]
    with pytest.raises(ValueError):
        J.showdown_ev(two)                                                  # no bets
    with pytest.raises(ValueError):
        J.showdown_ev(two, bets=[1.0])                                      # one bet for two seats
    with pytest.raises(ValueError):
        J.showdown_ev(two, bets=[1.0, -2.0])
    with pytest.raises(ValueError):
        J.showdown_ev(two, bets=[1.0, float("nan")])
    with pytest.raises(ValueError):
        J.showdown_ev([["AS", "KS"]], bets=[1.0])
    with pytest.raises(ValueError):
        J.showdown_ev(two, board=["2S"] * 6, bets=[1.0, 1.0])
    with pytest.raises(ValueError):
        J.showdown_ev(two, live=[0, 2], bets=[1.0, 1.0])
    with pytest.raises(ValueError):
        J.showdown_ev_batch(np.zeros((3, 6, 2), np.uint8), np.zeros((3, 5)), np.zeros(3), np.zeros(3), np.zeros((3, 5)))
    r = J.ShowdownEV(np.array([[5.0, -5.0]]), np.zeros((1, 2, 2), np.uint64), np.array([[0, 0xFF]], np.uint8), np.array([[10.0, 0.0]]),
                     np.array([1], np.uint32), np.array([0], np.uint8), np.array([[5.0, 5.0]]))
    assert r.payout.tolist() == [[10.0, 0.0]] and r[0].payout.tolist() == [10.0, 0.0] and r.levels == [[(0, 10.0)]] and r[0].levels == [(0, 10.0)]
    assert J.ev_status_text(EV.BAD_BET | ES.NO_LIVE) == "no live seat; a bet that is negative, NaN or infinite"
