"""CPU tests of the pre-flop matchups (no GPU): the numpy restatement of the definition (preflop_spec) against the showdown-equity spec on the
two witness matchups whose suit-isomorphic results differ, the additivity of partial counts, the golden file against its generator's list,
the status rule, the new constants and entry points in the header and the binding, the k_pfm_* kernels in the built library's code objects,
and the argument validation of the C entry points and of the Python helpers."""
import json
import os
import re
import sys

import numpy as np
import pytest

import equity_spec as ES
import preflop_spec as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pk_preflop_count_d", "pk_preflop_count", "pk_preflop_matchups_d", "pk_preflop_matchups", "pk_equity_preflop_d", "pk_equity_preflop",
                "pk_table_equity_preflop_d", "pk_table_equity_preflop", "pk_equity_rvr_preflop_d", "pk_equity_rvr_preflop")
WITNESSES = (([0x04, 0x03], [0x1C, 0x2B], (706238, 11593, 994473)), ([0x34, 0x33], [0x0C, 0x1B], (707259, 11592, 993453)))
H = PS.HOLDINGS


@pytest.fixture(scope="module")
def lib():
    from pokerl_amd import _lib, build
    build.build_lib()
    return _lib


@pytest.mark.parametrize("hero,villain,want", WITNESSES)
def test_pair_counts_over_all_boards_equal_the_showdown_equity_spec(hero, villain, want):
    """Both spots are five-four suited against king-queen off suit (rank nibble 0 is the ace); the evaluator is not invariant under a renaming of suits, so the counts differ."""
    got = PS.pair_counts(PS.holding_of_values(*hero), PS.holding_of_values(*villain))
    e = ES.spot_equity([hero, villain], [0] * 5, 0, 3)
    assert e["status"] == 0 and e["boards"] == PS.PAIR_BOARDS == sum(got)
    assert got == (int(e["win"][0]), int(e["tie"][0]), int(e["win"][1])) == want


def test_counts_add_over_a_split_range_and_agree_with_pair_counts():
    first, n = 1000003, 24
    w, t = PS.counts(first, n)
    w1, t1 = PS.counts(first, 7)
    w2, t2 = PS.counts(first + 7, n - 7)
    assert (w1 + w2 == w).all() and (t1 + t2 == t).all() and w.any() and t.any()
    sh = PS.shared()
    assert not w[sh].any() and not t[sh].any() and (t == t.T).all()
    rng = np.random.default_rng(5)
    for h, o in [(0, 1325), (1325, 0), (54, 55), (7, 7), (0, 1)] + [tuple(int(x) for x in rng.integers(0, H, 2)) for _ in range(40)]:
        assert PS.pair_counts(h, o, first, n) == (int(w[h, o]), int(t[h, o]), int(w[o, h])), (h, o)
    # a board decides every pair of holdings in play that share no card exactly once
    one_w, one_t = PS.counts(first + 3, 1)
    assert 2 * int(one_w.sum()) + int(one_t.sum()) == 1081 * 990
    assert PS.boards(0, 3).tolist() == [[0, 1, 2, 3, 4], [0, 1, 2, 3, 5], [0, 1, 2, 3, 6]] and PS.boards(PS.ALL_BOARDS - 1, 1).tolist() == [[47, 48, 49, 50, 51]]
    assert PS.unrank(first) == [int(x) for x in PS.all_boards()[first]]


def test_golden_file_is_what_its_generator_lists():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_preflop_matchups as G
    with open(os.path.join(ROOT, "tests", "golden", "preflop_matchups.json")) as f:
        gold = json.load(f)
    assert gold["boards"] == PS.PAIR_BOARDS and [g["name"] for g in gold["matchups"]] == [m[0] for m in G.MATCHUPS] and len(G.MATCHUPS) >= 16
    pairs = set()
    for g, (name, a, b) in zip(gold["matchups"], G.MATCHUPS):
        assert g["hero"] == [int(x) for x in a] and g["villain"] == [int(x) for x in b]
        assert (g["h"], g["o"]) == (PS.holding_of_values(*a), PS.holding_of_values(*b)) and g["win"] + g["tie"] + g["lose"] == PS.PAIR_BOARDS
        pairs.add((g["h"], g["o"]))
    for hero, villain, want in WITNESSES:                            # the two witnesses, a pair of adjacent holdings, holdings 0 and 1325
        g = next(x for x in gold["matchups"] if x["hero"] == hero and x["villain"] == villain)
        assert (g["win"], g["tie"], g["lose"]) == want
    assert (0, 1325) in pairs and (1325, 0) in pairs and any(abs(h - o) == 1 for h, o in pairs)
    # one of them recomputed here (the others: about 2 s each, python tests/golden/make_preflop_matchups.py)
    g = gold["matchups"][10]
    assert PS.pair_counts(g["h"], g["o"]) == (g["win"], g["tie"], g["lose"])


def test_status_rule_and_the_readers_spec():
    assert PS.hero_status([0x00, 0x01]) == 0 and PS.hero_status([0x3C, 0x0C]) == 0
    for hero in ([0x4A, 0x01], [0x05, 0xFF], [0x0D, 0x00], [0xFF, 0xFF], [0x40, 0x40]):
        assert PS.hero_status(hero) == PS.BAD_CARD, hero
    assert PS.hero_status([0x21, 0x21]) == PS.DUP_CARD
    rng = np.random.default_rng(1)
    win, tie = rng.integers(0, 1 << 20, (H, H)).astype(np.uint32), rng.integers(0, 1 << 10, (H, H)).astype(np.uint32)
    w = rng.integers(0, 65536, (3, H)).astype(np.uint16)
    rw, rt, tot = PS.rvr(win, tie, w)
    for h in (0, 700, 1325):                                         # row h of range vs range = the hero form's aggregates
        hero = [int(PS.CANON_V[PS.HOLD_A[h]]), int(PS.CANON_V[PS.HOLD_B[h]])]
        for s in range(3):
            r = PS.hero_equity(win, tie, hero, w[s])
            assert r["status"] == 0 and r["boards"] == PS.PAIR_BOARDS and r["agg"].tolist() == [int(rw[s, h]), int(rt[s, h]), int(tot[s, h])]
    ones = PS.hero_equity(win, tie, [0x00, 0x01])
    assert int(ones["agg"][2]) == 1225 * PS.PAIR_BOARDS
    bad = PS.hero_equity(win, tie, [0x00, 0x00])
    assert bad["status"] == PS.DUP_CARD and bad["boards"] == 0 and not bad["win"].any() and not bad["agg"].any()
    assert 65535 * 1225 * PS.PAIR_BOARDS < 2 ** 64


def test_header_declares_and_binding_lists_the_entry_points(lib):
    header = open(os.path.join(ROOT, "include", "pokerl_hip.h")).read()
    import ctypes
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in lib.SYMBOLS and hasattr(L, name), name
    assert "Pre-flop matchups" in header
    for name, value in (("PK_PREFLOP_BOARDS", PS.PAIR_BOARDS), ("PK_PREFLOP_ALL_BOARDS", PS.ALL_BOARDS)):
        assert re.search(r"#define %s %du\b" % (name, value), header), name
    assert (lib.PREFLOP_BOARDS, lib.PREFLOP_ALL_BOARDS, lib.EQ_HOLDINGS) == (PS.PAIR_BOARDS, PS.ALL_BOARDS, H)
    assert (lib.EQ_BAD_CARD, lib.EQ_DUP_CARD) == (PS.BAD_CARD, PS.DUP_CARD)
    assert lib.lib().pk_abi_version() == 6
    import pokerl_amd as P
    from pokerl_amd import judger as J
    for name in ("PreflopMatchups", "preflop_matchups", "preflop_matchups_d", "preflop_counts", "preflop_counts_d", "preflop_equity", "preflop_equity_batch",
                 "preflop_equity_d", "preflop_range_vs_range", "preflop_range_vs_range_batch", "preflop_range_vs_range_d"):
        assert getattr(P, name) is getattr(J, name) and name in P.__all__, name
    for cls, names in ((P.VecGame, ("equity_preflop", "equity_preflop_d")), (P.Game, ("equity_preflop",))):
        for name in names:
            assert callable(getattr(cls, name)), name
    from pokerl_amd import build
    assert "pk_preflop.hip" in build.SOURCES


def test_kernels_exist_without_scratch_within_their_occupancy(lib):
    """`.private_segment_fixed_size` == 0 and no spill for every k_pfm_* kernel.  k_pfm_count declares __launch_bounds__(256, 2): a lane has at
    most 256 registers (128 of them counters); its LDS is the two key strips of 32 boards, 2 x 16 KB, as DESIGN.md section 3.10 states, so
    LDS allows five workgroups per CU.  k_pfm_rank stages the 32 KB evaluator table and nothing else."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(lib.LIB_PATH)
    pf = {k: d for k, d in ks.items() if k.startswith("k_pfm_")}
    assert sorted(pf) == ["k_pfm_count<false>", "k_pfm_count<true>", "k_pfm_hero", "k_pfm_prep<false>", "k_pfm_prep<true>", "k_pfm_rank", "k_pfm_rvr"], sorted(pf)
    assert all(d["private_segment"] == 0 and d["vgpr_spill"] == 0 for d in pf.values()), pf
    for name in ("k_pfm_count<false>", "k_pfm_count<true>"):
        k = pf[name]
        assert k["lds"] == 2 * 32 * 128 * 4 == 32768, k["lds"]
        unified = (k["vgprs"] + 3) // 4 * 4 + max(k["agprs"], 0)
        assert 128 + 16 <= unified <= 256, k
    assert pf["k_pfm_rank"]["lds"] == 32768 and pf["k_pfm_hero"]["lds"] <= 256 and pf["k_pfm_rvr"]["lds"] <= 512
    src = open(os.path.join(ROOT, "pokerl_amd", "csrc", "pk_preflop.hip")).read()
    assert re.search(r"__launch_bounds__\(PFM_COUNT_BLOCK, 2\)\s+k_pfm_count\(", src)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3.10" in design and "k_pfm_count" in design
    # the new kernels match none of the prefixes the other families' tests list their kernels by
    for k in pf:
        assert not re.match(r"k_(rvr|hist|eqr|eqs|eqw|equity|ev|hero_hist|cl_|reset|make_fresh|pick|rollout|step|env_)", k), k
    assert "k_eqr" in ks and "k_rvr" in ks and "k_equity<2>" in ks


def test_bad_arguments_are_refused_without_a_device(lib):
    L = lib.lib()
    p = lib.ptr
    big = np.zeros(8, np.uint8)

    def refused(rc, *texts):
        assert rc == lib.PK_E_INVALID_ARG, rc
        err = L.pk_last_error(None)
        for t in texts:
            assert t in err, (t, err)

    refused(L.pk_preflop_count(0, PS.ALL_BOARDS, 1, 0, None, None), b"pk_preflop_count", b"first + n above PK_PREFLOP_ALL_BOARDS")
    refused(L.pk_preflop_count_d(0, 5, PS.ALL_BOARDS, 0, None, None, None), b"pk_preflop_count_d", b"first + n above")
    refused(L.pk_preflop_count(0, 0xFFFFFFFF, 0xFFFFFFFF, 1, None, None), b"first + n above")          # (the sum is formed in 64 bits)
    refused(L.pk_equity_preflop(0, 1, None, None, 0, None, None, None, None, None), b"pk_equity_preflop", b"NULL input buffer")
    refused(L.pk_equity_preflop_d(0, 1, None, None, 0, None, None, None, None, None, None), b"pk_equity_preflop_d", b"NULL input buffer")
    refused(L.pk_equity_preflop(0, 2 ** 31, p(big), None, 0, None, None, None, None, None), b"m >= 2^31")
    refused(L.pk_equity_rvr_preflop(0, 2 ** 31, None, None, None, None), b"pk_equity_rvr_preflop", b"m >= 2^31")
    refused(L.pk_equity_rvr_preflop_d(0, 2 ** 31, None, None, None, None, None), b"pk_equity_rvr_preflop_d", b"m >= 2^31")
    # a device index no device has: refused, whatever the machine (no GPU is needed to say so)
    assert L.pk_equity_preflop_d(64, 1, p(big), None, 0, None, None, None, None, None, None) != lib.PK_OK
    assert L.pk_preflop_matchups(64, None, None) != lib.PK_OK and L.pk_preflop_count_d(64, 0, 1, 0, None, None, None) != lib.PK_OK
    for obs in (0, lib.OBSERVER_NONE, lib.OBSERVER_ACTIVE):            # the table forms without a handle
        assert L.pk_table_equity_preflop_d(None, None, 4, obs, None, 0, None, None, None, None, None) == lib.PK_E_INVALID_ARG
        assert L.pk_table_equity_preflop(None, None, 4, obs, None, 0, None, None, None, None, None) == lib.PK_E_INVALID_ARG


def test_python_helpers_validate_before_any_device_call(lib):
    from pokerl_amd import judger as J
    with pytest.raises(ValueError):
        J.preflop_equity(["AS"])
    with pytest.raises(ValueError):
        J.preflop_equity(["AS", 0x4F])
    with pytest.raises(ValueError):
        J.preflop_equity(["AS", "KS"], weights=np.ones(1325, np.uint16))
    with pytest.raises(ValueError):
        J.preflop_equity(["AS", "KS"], weights=np.full(H, 65536))
    with pytest.raises(ValueError):
        J.preflop_equity_batch(np.zeros((3, 3), np.uint8))
    with pytest.raises(ValueError):
        J.preflop_equity_batch(np.zeros((3, 2), np.uint8), weights=np.ones((2, H), np.uint16))
    for bad in (np.ones(H, np.uint16), np.ones((2, 1325), np.uint16), np.full((1, H), -1), np.full((1, H), 65536), np.ones((1, H), np.float64)):
        with pytest.raises(ValueError):
            J.preflop_range_vs_range_batch(bad)
    with pytest.raises(ValueError):
        J.preflop_range_vs_range(np.ones((1, H), np.uint16))
    for first, n in ((-1, 1), (0, -1), (PS.ALL_BOARDS, 1), (PS.ALL_BOARDS - 1, 2)):
        with pytest.raises(ValueError):
            J.preflop_counts(first, n)
    w = np.zeros((H, H), np.uint32)
    for win, tie in ((w, None), (w, w.astype(np.uint64)), (w, w[:, ::-1]), (w[:-1], w[:-1])):
        with pytest.raises(ValueError):
            J.preflop_counts(0, 1, win, tie)
    m = J.PreflopMatchups(np.full((H, H), PS.PAIR_BOARDS // 2, np.uint32), np.zeros((H, H), np.uint32))
    e = m.equity
    assert np.isnan(e[0, 0]) and np.isnan(e[0, 1]) and e[0, 1325] == (PS.PAIR_BOARDS // 2) / PS.PAIR_BOARDS and (m.shared == PS.shared()).all()
    v = J.preflop_valid_holdings(np.array([[0x00, 0x10], [0x3C, 0x2C]], np.uint8))
    assert v.shape == (2, H) and v.sum(axis=1).tolist() == [1225, 1225] and not v[0, 0] and v[0, 1325]
