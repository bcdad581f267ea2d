"""CPU tests of the range equity (no GPU): the numpy restatement of the definition against the fixture computed by the reference's own
eval_hand / compare_rankings and against the two-seat showdown-equity spec, the holding index, the new entry points in the header and the
binding, the new kernels in the built library's code objects, and the argument validation of the Python helpers."""
import json
import os
import re
import sys

import numpy as np
import pytest

import equity_range_spec as RS
import equity_spec as ES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pk_equity_range_d", "pk_equity_range", "pk_table_equity_range_d", "pk_table_equity_range")


def fixture_spots():
    with open(os.path.join(ROOT, "tests", "golden", "equity_range_ref.json")) as f:
        ref = json.load(f)
    assert ref["holdings"] == RS.HOLDINGS
    return ref["spots"]


@pytest.fixture(scope="module")
def lib():
    from pokerl_amd import _lib, build
    build.build_lib()
    return _lib


def test_fixture_covers_what_it_must():
    spots = fixture_spots()
    shape = [(len(s["board"]), s["pool"], bool(s["dead"])) for s in spots]
    assert (5, 45, False) in shape and (4, 46, False) in shape                  # full-pool river and turn
    assert (3, 20, True) in shape and any(nb == 4 and d for nb, _, d in shape)  # flop with a dead mask that leaves 20, turn with a dead mask
    # the royal-flush board: the hero plays the board and never loses (the reference ranks a villain who adds LOW spades a mere flush --
    # judger.py:56-57 -- so not every holding ties, as it would at poker)
    assert any(len(s["board"]) == 5 and len(s["h"]) == 990 and all(w + t == 1 for w, t in zip(s["win"], s["tie"])) and 0 < sum(s["tie"]) < 990 for s in spots)
    # the hero flops the nuts, a royal flush, on a full pool (the same tracker ranks it a mere flush on the boards that bring low spades, so
    # the reference does not let it win EVERY board)
    assert any(s["name"] == "a flop where the hero holds the nuts" and len(s["board"]) == 3 and s["pool"] == 47 and max(s["win"]) == 990 for s in spots)
    for s in spots:
        assert len(s["h"]) == len(s["win"]) == len(s["tie"]) == s["pool"] * (s["pool"] - 1) // 2


def test_spec_equals_reference_fixture():
    for i, s in enumerate(fixture_spots()):
        nb = len(s["board"])
        got = RS.spot_range(s["hero"], s["board"] + [0] * (5 - nb), nb, s["dead"])
        assert got["status"] == 0 and got["boards"] == s["boards"], i
        h = np.array(s["h"])
        valid = np.zeros(RS.HOLDINGS, bool)
        valid[h] = True
        assert np.array_equal(got["valid"], valid), i
        assert got["win"][h].tolist() == s["win"] and got["tie"][h].tolist() == s["tie"], i
        assert not got["win"][~valid].any() and not got["tie"][~valid].any(), i


def test_spec_equals_two_seat_showdown_equity():
    """The counts against a holding are the hero's counts of the two-seat spot with that holding filled in (equity_spec.spot_equity)."""
    rng = np.random.default_rng(0x52414E47)
    checked = 0
    for nb, pool in ((5, None), (4, None), (3, 20), (4, 22), (5, 30)):
        hero, board, nboard, dead = RS.random_spots(rng, 1, nb, pool)
        r = RS.spot_range(hero[0], board[0], nb, dead[0])
        assert r["status"] == 0
        gone = [RS.CANON[k] for k in range(52) if (int(dead[0]) >> k) & 1]
        for h in rng.choice(np.nonzero(r["valid"])[0], 3, replace=False):
            villain = [RS.CANON[RS.PAIR_A[h]], RS.CANON[RS.PAIR_B[h]]]
            # the dead cards leave the two-seat spot's pool as further seats that hold them and do not show down
            extra = gone + [ES.UNKNOWN] * (len(gone) % 2)
            holes = np.array([list(hero[0]), villain] + [extra[j:j + 2] for j in range(0, len(extra), 2)], np.uint8)
            if holes.shape[0] > 16:
                continue
            e = ES.spot_equity(holes, [int(x) for x in board[0]], nb, 0b11)
            assert e["status"] == 0 and e["boards"] == r["boards"]
            assert (int(e["win"][0]), int(e["tie"][0])) == (int(r["win"][h]), int(r["tie"][h]))
            checked += 1
    assert checked >= 12


def test_spec_status_bits(lib):
    assert (RS.BAD_CARD, RS.DUP_CARD, RS.BAD_NBOARD, RS.IN_FLIGHT, RS.BAD_TABLE, RS.PREFLOP, RS.SMALL_POOL, RS.HOLDINGS) == \
        (lib.EQ_BAD_CARD, lib.EQ_DUP_CARD, lib.EQ_BAD_NBOARD, lib.EQ_IN_FLIGHT, lib.EQ_BAD_TABLE, lib.EQ_PREFLOP, lib.EQ_SMALL_POOL, lib.EQ_HOLDINGS)
    hero, board = [0x00, 0x01], [0x20, 0x21, 0x22, 0x23, 0x24]
    st = lambda *a: RS.spot_range(*a)["status"]
    assert st(hero, board, 5) == 0 and st(hero, board, 3) == 0
    assert [st(hero, board, nb) for nb in (0, 1, 2)] == [RS.PREFLOP] * 3
    assert st(hero, board, 6) == RS.BAD_NBOARD
    assert st([0x00, 0xFF], board, 5) == RS.BAD_CARD and st(hero, [0x20, 0x21, 0xFF, 0x23, 0x24], 4) == RS.BAD_CARD
    assert st(hero, [0x20, 0x21, 0xFF, 0x23, 0x24], 2) == RS.PREFLOP           # (only the first nb board cards count)
    assert st([0x0D, 0x01], board, 5) == RS.BAD_CARD and st(hero, board, 5, 1 << 52) == RS.BAD_CARD
    assert st([0x00, 0x00], board, 5) == RS.DUP_CARD and st(hero, [0x20, 0x01, 0x22, 0x23, 0x24], 3) == RS.DUP_CARD
    assert st(hero, board, 5, 1 << RS.canon_index(0x21)) == RS.DUP_CARD        # a board card that is also dead
    assert st(hero, board, 3, 1 << RS.canon_index(0x24)) == 0                  # (... but not one the spot does not use)
    used = {RS.canon_index(c) for c in hero + board}
    free = [k for k in range(52) if k not in used]
    mask = lambda left: sum(1 << k for k in free[left:])
    assert st(hero, board, 5, mask(2)) == 0 and st(hero, board, 5, mask(1)) == RS.SMALL_POOL
    r = RS.spot_range(hero, board, 5, mask(2))
    assert r["boards"] == 1 and r["valid"].sum() == 1
    r = RS.spot_range(hero, board, 5, mask(1))
    assert r["boards"] == 0 and not r["win"].any() and not r["valid"].any()


def test_holding_index_is_a_bijection(lib):
    import pokerl_amd as P
    assert P.HOLDINGS.shape == (RS.HOLDINGS, 2) and P.HOLDINGS.dtype == np.uint8
    seen = set()
    for k0 in range(52):
        for k1 in range(52):
            if k0 == k1:
                continue
            h = P.holding_index(RS.CANON[k0], RS.CANON[k1])
            assert h == RS.holding_index(k0, k1) and 0 <= h < RS.HOLDINGS
            assert sorted(P.HOLDINGS[h].tolist()) == sorted([RS.CANON[k0], RS.CANON[k1]])
            seen.add(h)
    assert seen == set(range(RS.HOLDINGS))
    assert P.HOLDINGS[:, 0].tolist() == [RS.CANON[a] for a in RS.PAIR_A] and P.HOLDINGS[:, 1].tolist() == [RS.CANON[b] for b in RS.PAIR_B]
    assert P.holding_index("AS", "KS") == P.holding_index("KS", "AS")
    with pytest.raises(ValueError):
        P.holding_index("AS", "AS")


def test_header_declares_and_binding_lists_the_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "pokerl_hip.h")).read()
    import ctypes
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in lib.SYMBOLS and hasattr(L, name), name
    assert re.search(r"#define PK_EQ_HOLDINGS 1326\b", header)
    assert re.search(r"#define PK_EQ_PREFLOP 64u\b", header) and re.search(r"#define PK_EQ_SMALL_POOL 128u\b", header)
    assert lib.lib().pk_abi_version() == 6


def test_range_kernels_exist_without_scratch(lib):
    """`.private_segment_fixed_size` == 0 for the new kernels, and the enumeration kernel's LDS (the 32 KB table, the hero's words, two
    counters per holding) lets three workgroups share a CU: at most 163 840 / 3 = 54 613 bytes."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(lib.LIB_PATH)
    eqr = {k: d for k, d in ks.items() if k.startswith("k_eqr")}
    assert sorted(eqr) == ["k_eqr", "k_eqr_prep<false>", "k_eqr_prep<true>"], sorted(eqr)
    assert all(d["private_segment"] == 0 and d["vgpr_spill"] == 0 for d in eqr.values()), eqr
    assert 32768 + 4 * 1081 + 8 * 1326 <= eqr["k_eqr"]["lds"] <= 54613, eqr["k_eqr"]["lds"]


def test_null_arguments_are_refused_without_a_device(lib):
    L = lib.lib()
    assert L.pk_table_equity_range_d(None, None, 4, 0, None, 0, None, None, None, None, None) == lib.PK_E_INVALID_ARG
    assert L.pk_table_equity_range(None, None, 4, 0, None, 0, None, None, None, None, None) == lib.PK_E_INVALID_ARG
    one = np.zeros(64, np.uint8)
    assert L.pk_equity_range(0, 1, None, lib.ptr(one), lib.ptr(one), None, None, 0, None, None, None, None, None) == lib.PK_E_INVALID_ARG
    assert b"pk_equity_range" in L.pk_last_error(None)
    assert L.pk_equity_range_d(0, 1, lib.ptr(one), None, lib.ptr(one), None, None, 0, None, None, None, None, None, None) == lib.PK_E_INVALID_ARG
    assert L.pk_equity_range_d(0, 2 ** 31, lib.ptr(one), lib.ptr(one), lib.ptr(one), None, None, 0, None, None, None, None, None, None) == lib.PK_E_INVALID_ARG
    assert L.pk_equity_range_d(64, 1, lib.ptr(one), lib.ptr(one), lib.ptr(one), None, None, 0, None, None, None, None, None, None) != lib.PK_OK


def test_python_helpers_validate_before_any_device_call(lib):
    from pokerl_amd import judger as J
    with pytest.raises(ValueError):
        J.range_equity(["AS"], ["2S", "3S", "4S"])                               # one hero card
    with pytest.raises(ValueError):
        J.range_equity(["AS", "KS"], ["2S", "3S"])                               # pre-flop
    with pytest.raises(ValueError):
        J.range_equity(["AS", "KS"], ["2S"] * 6)
    with pytest.raises(ValueError):
        J.range_equity(["AS", 0x4F], ["2S", "3S", "4S"])                         # not a card
    with pytest.raises(ValueError):
        J.range_equity(["AS", "KS"], ["2S", "3S", "4S"], weights=np.ones(1325, np.uint16))
    with pytest.raises(ValueError):
        J.range_equity(["AS", "KS"], ["2S", "3S", "4S"], weights=np.full(1326, 65536))
    with pytest.raises(ValueError):
        J.range_equity_batch(np.zeros((3, 3), np.uint8), np.zeros((3, 5)), np.zeros(3))
    with pytest.raises(ValueError):
        J.range_equity_batch(np.zeros((3, 2), np.uint8), np.zeros((3, 5)), np.zeros(3), weights=np.ones((2, 1326), np.uint16))
    assert J.dead_mask(["AS", "2S"]) == (1 << 0) | (1 << 4)
    r = J.RangeEquity(np.array([[2, 0]], np.uint32), np.array([[0, 2]], np.uint32), np.array([2], np.uint32), np.array([0], np.uint8),
                      np.array([[2, 2, 4]], np.uint64))
    assert r.equity.tolist() == [[1.0, 0.5]] and r.strength.tolist() == [0.75] and r[0].strength == 0.75
    assert J.equity_status_text(RS.PREFLOP).startswith("fewer than three board cards")
    v = J.valid_holdings(np.array([[0x00, 0x01]], np.uint8), np.array([[0x20, 0x21, 0x22, 0x23, 0x24]], np.uint8), np.array([3]), np.array([1 << 51], np.uint64))
    assert np.array_equal(v[0], RS.spot_range([0x00, 0x01], [0x20, 0x21, 0x22, 0x23, 0x24], 3, 1 << 51)["valid"])
