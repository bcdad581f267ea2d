"""CPU tests of range vs range (no GPU): the numpy restatement of the definition against the fixture computed by the reference's own
eval_hand / compare_rankings and against the range-equity spec row by row, the two-seat order claim of DESIGN.md section 3.4, the status
bits, the new entry points in the header and the binding, the new kernels in the built library's code objects, and the Python helpers."""
import json
import math
import os
import re
import sys

import numpy as np
import pytest

import equity_range_spec as RS
import equity_spec as ES
import rvr_spec as VS
from oracle import loader as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pk_equity_rvr_d", "pk_equity_rvr", "pk_table_equity_rvr_d", "pk_table_equity_rvr")
H = VS.HOLDINGS


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "rvr_ref.json")) as f:
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
    w = ref["weights"]
    assert 0 in w and 65535 in w and max(w) <= 65535 and min(w) >= 0
    shape = [(len(s["board"]), s["pool"]) for s in ref["spots"]]
    assert shape.count((5, 47)) == 3 and (4, 14) in shape and (3, 10) in shape            # three full-pool rivers, a dead-mask turn and flop
    assert (5, 4) in shape and (4, 5) in shape and (3, 6) in shape                        # the smallest pools: P = k + 4
    royal = [s for s in ref["spots"] if "royal" in s["name"]][0]
    assert max(royal["tie"]) > 500                                                        # large groups of equal keys
    for s in ref["spots"]:
        n = s["pool"] * (s["pool"] - 1) // 2
        assert all(len(s[key]) == n for key in ("h", "win", "tie", "tot", "win_w", "tie_w", "tot_w"))
        assert s["boards"] == math.comb(s["pool"] - 4, 5 - len(s["board"]))
        assert all(a + b <= c for a, b, c in zip(s["win"], s["tie"], s["tot"]))


def test_spec_equals_reference_fixture():
    ref = fixture()
    weights = np.array([np.ones(H, np.int64), ref["weights"]])
    for i, s in enumerate(ref["spots"]):
        nb = len(s["board"])
        got = VS.spot_rvr(s["board"] + [0] * (5 - nb), nb, s["dead"], weights)
        assert got["status"] == 0 and got["boards"] == s["boards"], i
        h = np.array(s["h"])
        valid = np.zeros(H, bool)
        valid[h] = True
        assert np.array_equal(got["valid"], valid), i
        for r, suffix in ((0, ""), (1, "_w")):
            for key in ("win", "tie", "tot"):
                assert got[key][r][h].tolist() == s[key + suffix], (i, key + suffix)
                assert not got[key][r][~valid].any(), (i, key + suffix)
        alone = VS.spot_rvr(s["board"] + [0] * (5 - nb), nb, s["dead"])                   # (the one-range form)
        assert all(np.array_equal(alone[key], got[key][0]) for key in ("win", "tie", "tot")), i


@pytest.mark.parametrize("nb,pool", [(5, 47), (4, 12), (3, 9)])
def test_spec_row_is_the_range_equity_of_that_hero(nb, pool):
    """The identity that pins the definition: row h = agg[3] of the range-equity spot hero = h, same board, dead and weights."""
    rng = np.random.default_rng(0x525652 + nb)
    board, nboard, dead = VS.random_boards(rng, 1, nb, pool)
    w = rng.integers(0, 65536, H)
    w[rng.integers(0, H, 200)] = 0
    r = VS.spot_rvr(board[0], nb, dead[0], w)
    assert r["status"] == 0 and r["valid"].sum() == pool * (pool - 1) // 2
    for h in rng.choice(np.flatnonzero(r["valid"]), 3, replace=False):
        hero = [VS.CANON[VS.PAIR_A[h]], VS.CANON[VS.PAIR_B[h]]]
        one = RS.spot_range(hero, board[0], nb, dead[0])
        assert one["status"] == 0 and one["boards"] == r["boards"]
        assert RS.aggregate(one, w) == [int(r["win"][h]), int(r["tie"][h]), int(r["tot"][h])], h


def test_two_seat_order_claim():
    """with two entries compare_rankings is a strict weak order on the ranking word -- the lower class number wins,
    within a class the larger kickers value wins, equal words tie -- over ALL pairs of the ranking words of one full-pool river board."""
    rng = np.random.default_rng(34)
    board, _, _ = VS.random_boards(rng, 1, 5)
    pool = [k for k in range(52) if VS.CANON[k] not in board[0].tolist()]
    hands = np.array([list(board[0]) + [VS.CANON[a], VS.CANON[b]] for b in pool for a in pool if a < b], np.uint8)
    assert len(hands) == 1081
    rank, kick, _ = O.eval_hands(hands)
    i, j = np.meshgrid(np.arange(1081), np.arange(1081), indexing="ij")
    i, j = i.ravel(), j.ravel()
    got = ES.winners_literal(np.stack([rank[i], rank[j]]), np.stack([kick[i], kick[j]]))
    ri, rj, ki, kj = rank[i].astype(np.int64), rank[j].astype(np.int64), kick[i].astype(np.int64), kick[j].astype(np.int64)
    first = (ri < rj) | ((ri == rj) & (ki > kj))
    same = (ri == rj) & (ki == kj)
    assert np.array_equal(got, np.where(same, 3, np.where(first, 1, 2)))
    assert len(set(rank.tolist())) >= 3 and same.sum() > 1081                             # several classes, and ties beyond the diagonal
    # ... so ONE integer orders them: larger = stronger, equal = tie (the device's sort key; a class number fits 4 bits, kickers 20)
    assert rank.max() <= 15 and kick.max() < 1 << 20
    key = ((15 - rank.astype(np.int64)) << 20) | kick.astype(np.int64)
    assert np.array_equal(got, np.where(key[i] == key[j], 3, np.where(key[i] > key[j], 1, 2)))


def test_spec_status_bits(lib):
    assert (VS.BAD_CARD, VS.DUP_CARD, VS.BAD_NBOARD, VS.IN_FLIGHT, VS.BAD_TABLE, VS.PREFLOP, VS.SMALL_POOL, VS.HOLDINGS) == \
        (lib.EQ_BAD_CARD, lib.EQ_DUP_CARD, lib.EQ_BAD_NBOARD, lib.EQ_IN_FLIGHT, lib.EQ_BAD_TABLE, lib.EQ_PREFLOP, lib.EQ_SMALL_POOL, lib.EQ_HOLDINGS)
    board = [0x20, 0x21, 0x22, 0x23, 0x24]
    st = lambda *a: VS.check_spot(*a)[0]                                                  # (spot_rvr's own check; no full-pool flop is enumerated here)
    assert st(board, 5) == 0 and st(board, 4) == 0 and st(board, 3) == 0
    assert [st(board, nb) for nb in (0, 1, 2)] == [VS.PREFLOP] * 3
    assert st(board, 6) == VS.BAD_NBOARD and st(board, 255) == VS.BAD_NBOARD
    assert st([0x20, 0x21, 0xFF, 0x23, 0x24], 4) == VS.BAD_CARD and st([0x20, 0x4F, 0x22, 0x23, 0x24], 4) == VS.BAD_CARD
    assert st([0x20, 0x21, 0xFF, 0x23, 0x24], 2) == VS.PREFLOP                            # (only the first nb board cards count)
    assert st(board, 5, 1 << 52) == VS.BAD_CARD
    assert st([0x20, 0x20, 0x22, 0x23, 0x24], 3) == VS.DUP_CARD
    assert st(board, 5, 1 << VS.canon_index(0x21)) == VS.DUP_CARD                         # a board card that is also dead
    assert st(board, 3, 1 << VS.canon_index(0x24)) == 0                                   # (... but not one the spot does not use)
    for nb in (5, 4, 3):
        k = 5 - nb
        free = [c for c in range(52) if c not in {VS.canon_index(x) for x in board[:nb]}]
        mask = lambda left: sum(1 << c for c in free[left:])
        assert st(board, nb, mask(k + 4)) == 0 and st(board, nb, mask(k + 3)) == VS.SMALL_POOL
        r = VS.spot_rvr(board, nb, mask(k + 4))
        assert r["boards"] == 1 and r["valid"].sum() == math.comb(k + 4, 2) and (r["tot"][r["valid"]] == math.comb(k + 2, 2)).all()
        r = VS.spot_rvr(board, nb, mask(k + 3))
        assert r["boards"] == 0 and not r["win"].any() and not r["tot"].any() and not r["valid"].any()


def test_header_declares_and_binding_lists_the_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "pokerl_hip.h")).read()
    import ctypes
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in lib.SYMBOLS and hasattr(L, name), name
    assert "IDENTITY: row h of a spot is the agg[3] that pk_equity_range returns for hero = h" in header
    assert lib.lib().pk_abi_version() == 6


def test_rvr_kernels_exist_without_scratch(lib):
    """`.private_segment_fixed_size` == 0 and no spilled VGPR for the new kernels; the group segment of k_rvr holds the 32 KB table and the
    sort, and lets two workgroups share a CU: at most 65 536 bytes."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(lib.LIB_PATH)
    rvr = {k: d for k, d in ks.items() if k.startswith("k_rvr")}
    assert sorted(rvr) == ["k_rvr", "k_rvr_prep<false>", "k_rvr_prep<true>"], sorted(rvr)
    assert all(d["private_segment"] == 0 and d["vgpr_spill"] == 0 for d in rvr.values()), rvr
    assert 32768 < rvr["k_rvr"]["lds"] <= 65536, rvr["k_rvr"]["lds"]
    assert rvr["k_rvr"]["vgprs"] + rvr["k_rvr"]["agprs"] <= 128                           # four waves per SIMD


def test_null_arguments_are_refused_without_a_device(lib):
    L = lib.lib()
    assert L.pk_table_equity_rvr_d(None, None, 4, None, 0, None, None, None, None, None) == lib.PK_E_INVALID_ARG
    assert L.pk_table_equity_rvr(None, None, 4, None, 0, None, None, None, None, None) == lib.PK_E_INVALID_ARG
    one = np.zeros(64, np.uint8)
    assert L.pk_equity_rvr(0, 1, None, lib.ptr(one), None, None, 0, None, None, None, None, None) == lib.PK_E_INVALID_ARG
    assert b"pk_equity_rvr" in L.pk_last_error(None)
    assert L.pk_equity_rvr_d(0, 1, lib.ptr(one), None, None, None, 0, None, None, None, None, None, None) == lib.PK_E_INVALID_ARG
    assert b"pk_equity_rvr_d" in L.pk_last_error(None)
    assert L.pk_equity_rvr_d(0, 2 ** 31, lib.ptr(one), lib.ptr(one), None, None, 0, None, None, None, None, None, None) == lib.PK_E_INVALID_ARG
    assert L.pk_equity_rvr_d(64, 1, lib.ptr(one), lib.ptr(one), None, None, 0, None, None, None, None, None, None) != lib.PK_OK


def test_python_helpers_validate_before_any_device_call(lib):
    import pokerl_amd as P
    from pokerl_amd import judger as J
    assert P.range_vs_range is J.range_vs_range and P.RangeVsRange is J.RangeVsRange
    assert P.range_vs_range_batch is J.range_vs_range_batch and P.range_vs_range_d is J.range_vs_range_d
    with pytest.raises(ValueError, match="fewer than three board cards"):
        J.range_vs_range(["2S", "3S"])                                                   # pre-flop
    with pytest.raises(ValueError):
        J.range_vs_range(["2S"] * 6)
    with pytest.raises(ValueError):
        J.range_vs_range(["AS", 0x4F, "2S"])                                             # not a card
    with pytest.raises(ValueError):
        J.range_vs_range(["2S", "3S", "4S"], weights=np.ones(1325, np.uint16))
    with pytest.raises(ValueError):
        J.range_vs_range(["2S", "3S", "4S"], weights=np.full(1326, 65536))
    with pytest.raises(ValueError):
        J.range_vs_range(["2S", "3S", "4S"], weights=np.ones((1, 1326), np.uint16))
    with pytest.raises(ValueError):
        J.range_vs_range_batch(np.zeros((3, 4), np.uint8), np.zeros(3))
    with pytest.raises(ValueError):
        J.range_vs_range_batch(np.zeros((3, 5), np.uint8), np.zeros(2))
    with pytest.raises(ValueError):
        J.range_vs_range_batch(np.zeros((3, 5), np.uint8), np.zeros(3), dead=np.zeros(2, np.uint64))
    with pytest.raises(ValueError):
        J.range_vs_range_batch(np.zeros((3, 5), np.uint8), np.zeros(3), weights=np.ones((2, 1326), np.uint16))
    dead = sum(1 << k for k in range(12, 51))                                             # leaves P = 10
    v = J.rvr_valid_holdings(np.array([[0x20, 0x21, 0x22, 0x23, 0x24]], np.uint8), np.array([3]), np.array([dead], np.uint64))
    assert v[0].sum() == 45 and np.array_equal(v[0], VS.spot_rvr([0x20, 0x21, 0x22, 0x23, 0x24], 3, dead)["valid"])


def test_strength_and_against_on_hand_made_arrays():
    from pokerl_amd import judger as J
    win, tie, tot = np.zeros((2, H), np.uint64), np.zeros((2, H), np.uint64), np.zeros((2, H), np.uint64)
    win[0, :3], tie[0, :3], tot[0, :3] = [2, 0, 1], [0, 2, 1], [4, 4, 0]                  # holding 2: tot = 0
    r = J.RangeVsRange(win, tie, tot, np.array([2, 0], np.uint32), np.array([0, VS.PREFLOP], np.uint8))
    s = r.strength
    assert s.shape == (2, H) and s[0, :2].tolist() == [0.5, 0.25] and np.isnan(s[0, 2:]).all() and np.isnan(s[1]).all()
    a = r.against()
    assert a.shape == (2,) and a[0] == (2 + 1 + 1 + 0.5) / 8 and math.isnan(a[1])
    u = np.zeros(H, np.int64)
    u[0], u[1] = 3, 1
    assert r.against(u)[0] == (3 * 2 + 1 * 1) / (3 * 4 + 1 * 4) and r[0].against(u) == 7 / 16
    one = r[0]
    assert one.win.shape == (H,) and one.boards == 2 and one.status == 0 and one.strength[0] == 0.5 and math.isnan(one.strength[2])
    assert math.isnan(r[1].against())
    big = J.RangeVsRange(np.full(H, 7 * 10 ** 10, np.uint64), np.zeros(H, np.uint64), np.full(H, 7 * 10 ** 10, np.uint64), 1, 0)
    assert big.against(np.full(H, 65535)) == 1.0                                          # (Python integers: 65 535 * 1 326 * 7e10 > 2^64)
    with pytest.raises(ValueError):
        r.against(np.ones(5))
