"""CPU tests of the showdown equity (no GPU): the numpy restatement of the definition against the fixture computed by the reference's own
eval_hand / compare_rankings, the new entry points in the header and the binding, the new kernels in the built library's code objects, and
the argument validation of the Python helpers."""
import json
import os
import re
import sys

import numpy as np
import pytest

import equity_spec as ES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pk_equity_d", "pk_equity", "pk_table_equity_d", "pk_table_equity")


def fixture_spots():
    with open(os.path.join(ROOT, "tests", "golden", "equity_ref.json")) as f:
        ref = json.load(f)
    assert ref["share_unit"] == ES.SHARE_UNIT
    return ref["spots"]


@pytest.fixture(scope="module")
def lib():
    from pokerl_amd import _lib, build
    build.build_lib()
    return _lib


def test_fixture_covers_what_it_must():
    spots = fixture_spots()
    assert {s["n"] for s in spots} >= {2, 3, 6, 9, 16}
    assert {len(s["board"]) for s in spots} >= {3, 4, 5}
    assert any(ES.UNKNOWN in sum(s["holes"], []) for s in spots)
    assert any(bin(s["live"]).count("1") < s["n"] for s in spots)
    dependent = [s for s in spots if s["line148"]]
    assert len(dependent) >= 3 and all(bin(s["live"]).count("1") >= 3 for s in dependent)


def test_spec_equals_reference_fixture():
    for i, s in enumerate(fixture_spots()):
        board = s["board"] + [0] * (5 - len(s["board"]))
        got = ES.spot_equity(np.array(s["holes"], np.uint8), board, len(s["board"]), s["live"])
        assert got["status"] == 0 and got["boards"] == s["boards"], i
        for k in ("win", "tie", "share"):
            assert [int(x) for x in got[k]] == s[k], (i, k)
        assert sum(s["share"]) == ES.SHARE_UNIT * s["boards"]
        if s["line148"]:          # ... and the marked spots do change when the loop raises best_kicker
            alt = ES.spot_equity(np.array(s["holes"], np.uint8), board, len(s["board"]), s["live"], fixed148=True)
            assert any([int(x) for x in alt[k]] != s[k] for k in ("win", "tie", "share")), i


def test_spec_status_bits(lib):
    """The spec's refusals, under the names and values the binding and the header give them."""
    assert (ES.BAD_CARD, ES.DUP_CARD, ES.NO_LIVE, ES.BAD_NBOARD, ES.IN_FLIGHT, ES.BAD_TABLE, ES.SHARE_UNIT) == \
        (lib.EQ_BAD_CARD, lib.EQ_DUP_CARD, lib.EQ_NO_LIVE, lib.EQ_BAD_NBOARD, lib.EQ_IN_FLIGHT, lib.EQ_BAD_TABLE, lib.EQ_SHARE_UNIT)
    holes = np.array([[0x00, 0x01], [0x12, 0x13], [ES.UNKNOWN, ES.UNKNOWN]], np.uint8)
    board = [0x20, 0x21, 0x22, 0x23, 0x24]
    assert ES.spot_equity(holes, board, 5, 0b011)["status"] == 0
    assert ES.spot_equity(holes, board, 5, 0b111)["status"] == ES.BAD_CARD            # unknown cards at a live seat
    assert ES.spot_equity(holes, board, 5, 0)["status"] == ES.NO_LIVE
    assert ES.spot_equity(holes, board, 6, 0b011)["status"] == ES.BAD_NBOARD
    assert ES.spot_equity(holes, [0x20, 0x20, 0x22, 0x23, 0x24], 5, 0b011)["status"] == ES.DUP_CARD
    assert ES.spot_equity(holes, [0x20, 0x20, 0x22, 0x23, 0x24], 1, 0b011)["status"] == 0     # (only the first nb board cards count)
    assert ES.spot_equity(holes, [0x2D, 0x21, 0x22, 0x23, 0x24], 5, 0b011)["status"] == ES.BAD_CARD
    assert ES.spot_equity(holes, [ES.UNKNOWN, 0x21, 0x22, 0x23, 0x24], 5, 0b011)["status"] == ES.BAD_CARD
    r = ES.spot_equity(holes, [0x00, 0x21, 0x22, 0x23, 0x24], 5, 0b011)
    assert r["status"] == ES.DUP_CARD and r["boards"] == 0 and not r["win"].any() and not r["share"].any()


def test_header_declares_and_binding_lists_the_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "pokerl_hip.h")).read()
    import ctypes
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in lib.SYMBOLS and hasattr(L, name), name
    for name, value in (("PK_EQ_SHARE_UNIT", ES.SHARE_UNIT), ("PK_EQ_BAD_CARD", ES.BAD_CARD), ("PK_EQ_DUP_CARD", ES.DUP_CARD),
                        ("PK_EQ_NO_LIVE", ES.NO_LIVE), ("PK_EQ_BAD_NBOARD", ES.BAD_NBOARD), ("PK_EQ_IN_FLIGHT", ES.IN_FLIGHT),
                        ("PK_EQ_BAD_TABLE", ES.BAD_TABLE)):
        assert re.search(r"#define %s %du\b" % (name, value), header), name
    assert (lib.EQ_SHARE_UNIT, lib.EQ_BAD_CARD, lib.EQ_DUP_CARD, lib.EQ_NO_LIVE, lib.EQ_BAD_NBOARD, lib.EQ_IN_FLIGHT, lib.EQ_BAD_TABLE) == \
        (ES.SHARE_UNIT, ES.BAD_CARD, ES.DUP_CARD, ES.NO_LIVE, ES.BAD_NBOARD, ES.IN_FLIGHT, ES.BAD_TABLE)
    assert lib.lib().pk_abi_version() == 6


def test_equity_kernels_exist_without_scratch(lib):
    """`.private_segment_fixed_size` == 0 for the preparation kernels and for the enumeration kernel of every seat count, and the
    enumeration kernel's LDS (the 32 KB table + the wavefronts' pools) lets four workgroups share a CU (160 KB)."""
    from pokerl_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(lib.LIB_PATH)
    names = ["k_equity_prep<true>", "k_equity_prep<false>"] + ["k_equity<%d>" % n for n in build.SEATS]
    eq = {k: d for k, d in ks.items() if k.startswith("k_equity")}
    assert sorted(eq) == sorted(names), sorted(eq)
    assert all(d["private_segment"] == 0 for d in eq.values()), {k: d["private_segment"] for k, d in eq.items()}
    assert all(32768 < eq["k_equity<%d>" % n]["lds"] <= 40960 for n in build.SEATS)


def test_null_arguments_are_refused_without_a_device(lib):
    L = lib.lib()
    assert L.pk_table_equity_d(None, None, 4, None, None, None, None, None) == lib.PK_E_INVALID_ARG
    assert L.pk_table_equity(None, None, 4, None, None, None, None, None) == lib.PK_E_INVALID_ARG
    one = np.zeros(64, np.uint8)
    for n in (1, 17, -3):
        assert L.pk_equity(0, n, 1, lib.ptr(one), lib.ptr(one), lib.ptr(one), lib.ptr(one), None, None, None, None, None) == lib.PK_E_INVALID_ARG
        assert L.pk_equity_d(0, n, 1, lib.ptr(one), lib.ptr(one), lib.ptr(one), lib.ptr(one), None, None, None, None, None, None) == lib.PK_E_INVALID_ARG
    assert L.pk_equity(0, 6, 1, None, lib.ptr(one), lib.ptr(one), lib.ptr(one), None, None, None, None, None) == lib.PK_E_INVALID_ARG
    assert b"pk_equity" in L.pk_last_error(None)
    # the device counts a call's tasks in 32 bits: a batch whose worst case (33 tasks per spot) does not fit is refused, not wrapped
    for m in (131 * 10 ** 6, 2 ** 31 - 1):
        assert L.pk_equity_d(0, 2, m, lib.ptr(one), lib.ptr(one), lib.ptr(one), lib.ptr(one), None, None, None, None, None, None) == lib.PK_E_INVALID_ARG
        assert b"too many spots" in L.pk_last_error(None)
        assert L.pk_equity(0, 2, m, lib.ptr(one), lib.ptr(one), lib.ptr(one), lib.ptr(one), None, None, None, None, None) == lib.PK_E_INVALID_ARG
    assert L.pk_equity_d(64, 2, 1, lib.ptr(one), lib.ptr(one), lib.ptr(one), lib.ptr(one), None, None, None, None, None, None) != lib.PK_OK


def test_refusals_are_the_recorded_ones(lib):
    """Every bad-argument call of the equity family (34 entry points) recorded in golden/equity_refusals.json, replayed: the return code and
    the pk_last_error(NULL) text, both exactly.  All of them are refused before any device is looked at."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_equity_refusals as MR
    with open(os.path.join(ROOT, "tests", "golden", "equity_refusals.json")) as f:
        ref = json.load(f)
    calls = [(c["fn"], c["args"]) for c in ref["calls"]]
    assert calls == [tuple(c) for c in MR.cases()]                              # (the fixture is what the script would record today)
    assert len({fn for fn, _ in calls}) == 34 and all(c["rc"] == lib.PK_E_INVALID_ARG for c in ref["calls"])
    got = MR.run(lib, calls, ref["mark"])
    for c, (rc, err) in zip(ref["calls"], got):
        assert (rc, err) == (c["rc"], c["error"]), (c["fn"], c["args"])


def test_python_helpers_validate_before_any_device_call(lib):
    from pokerl_amd import judger as J
    with pytest.raises(ValueError):
        J.showdown_equity([["AS", "KS"]])                                   # one seat
    with pytest.raises(ValueError):
        J.showdown_equity([["AS", "KS"], ["QD"]])                           # one hole card
    with pytest.raises(ValueError):
        J.showdown_equity([["AS", "KS"], ["QD", "QC"]], board=["2S"] * 6)   # six board cards
    with pytest.raises(ValueError):
        J.showdown_equity([["AS", "KS"], ["QD", "QC"]], live=[0, 2])        # a live seat that does not exist
    with pytest.raises(ValueError):
        J.showdown_equity([["AS", "KS"], ["QD", "QC"]], live=0b100)
    with pytest.raises(ValueError):
        J.showdown_equity([["AS", "KS"], [0x4F, 0x01]])                     # not a card
    with pytest.raises(ValueError):
        J.showdown_equity_batch(np.zeros((3, 6, 3), np.uint8), np.zeros((3, 5)), np.zeros(3), np.zeros(3))
    with pytest.raises(ValueError):
        J.showdown_equity_batch(np.zeros((3, 17, 2), np.uint8), np.zeros((3, 5)), np.zeros(3), np.zeros(3))
    with pytest.raises(ValueError):
        J.showdown_equity_batch(np.zeros((3, 6, 2), np.uint8), np.zeros((3, 4)), np.zeros(3), np.zeros(3))
    e = J.Equity(np.array([[1, 0]], np.uint32), np.array([[0, 0]], np.uint32), np.array([[720720, 0]], np.uint64), np.array([1], np.uint32),
                 np.array([0], np.uint8))
    assert e.equity.tolist() == [[1.0, 0.0]] and e[0].equity.tolist() == [1.0, 0.0]
    assert J.equity_status_text(ES.DUP_CARD | ES.NO_LIVE) == "a card twice; no live seat"
