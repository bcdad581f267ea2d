"""CPU pre-flight of tests/test_hip_equity_seat_matrix.py, with the specs alone: at every seat count 2 .. 16 the INPUTS of every family's
case (tests/equity_seat_matrix.py) reach what depends on the seat count -- so that a GPU case cannot pass by comparing nothing.  No spot
is refused; seat N - 1 wins alone, ties, and ties among three or more; the full ladder fills every group of pot levels; from eight seats
on the fractional ladder has a level whose clipped bets add up to other bits in numpy's order than left to right; the all-hidden ranged
spots accept every attempt, the mixed rows still reject and still accept nothing somewhere, and at least half of the spots with a hidden
seat accept something; the sampled draw counts lie on both sides of every word and block edge; the table state stands on three streets
with a folded seat and, from eight seats on, level amounts that round differently left to right.  The comparators reject a one-bit change.  The figures are printed per N (pytest -s shows them).
Measured: 3 s for the module's 86 cases (the specs of all fifteen seat counts of one family: 0.1 - 0.5 s; the oracle's tables and their five specs: 0.7 s)."""
import math

import numpy as np
import pytest

import equity_ranged_spec as WS
import equity_seat_matrix as M
import equity_spec as ES
import ev_spec as EV
from oracle import loader as O

SEATS = M.SEATS


def calls(family, N):
    return list(zip(M.case(family, N), M.want(family, N)))


@pytest.mark.parametrize("family", M.SPOT_FAMILIES)
def test_no_spot_is_refused_and_the_specs_keep_the_invariants(family):
    """Floor 1, and the invariants the device results are held to, on the specs' own outputs; the royal spots by the closed form."""
    for N in SEATS:
        for k, (c, w) in enumerate(calls(family, N)):
            assert not w["status"].any(), (family, N, k, w["status"].tolist())
            assert sorted(i for part in c["parts"].values() for i in part) == list(range(len(c["nboard"]))), (family, N, k)
            M.invariants(family, w, M.where_of(family, N, "spec, call %d" % k))
        if family in ("equity", "ev"):
            M.assert_royal(family, N, M.want(family, N)[0], M.where_of(family, N, "spec"))


@pytest.mark.parametrize("N", SEATS)
def test_equity_reaches_the_top_seat_and_many_way_ties(N):
    """Floor 2, on the spots with two or more live seats other than the royal one (which ties N ways by construction): seat N - 1 wins a
    board alone and ties one, and some board has three or more winners -- a seat whose share is below win + tie / 2 has split a board
    three ways or more (at two seats: a tie).  Boards of 1, P, C(P, 2) and C(P, 3) occur, P the spot's own pool."""
    (c, w), = calls("equity", N)
    spots = c["parts"]["all_live"] + [i for i in c["parts"]["folded"] if bin(int(c["live"][i])).count("1") >= 2]
    win, tie, share = (w[k][spots].astype(object) for k in ("win", "tie", "share"))
    assert win[:, N - 1].any(), "no sole win of seat N - 1"
    assert tie[:, N - 1].any(), "no tie of seat N - 1"
    many = 2 * (share - ES.SHARE_UNIT * win) < ES.SHARE_UNIT * tie
    assert many.any() if N > 2 else tie.any(), "no board with three or more winners"
    ks = set()
    for i in range(len(c["nboard"])):
        pool = 52 - len(ES.check_spot(c["holes"][i], c["board"][i], int(c["nboard"][i]), c["live"][i])[1])
        assert w["boards"][i] == math.comb(pool, 5 - int(c["nboard"][i]))
        ks.add(5 - int(c["nboard"][i]))
    assert ks == {0, 1, 2, 3}
    assert [int(c["live"][i]) for i in c["parts"]["top_alone"]] == [1 << (N - 1)] * 3 and all(c["live"][i] == M.full(N) for i in c["parts"]["all_live"])
    print("equity    N=%2d: boards %s, sole wins / ties of seat N-1 %d / %d, seats in a 3+-way tie %d"
          % (N, w["boards"].tolist(), int(win[:, N - 1].sum()), int(tie[:, N - 1].sum()), int(many.sum())))


@pytest.mark.parametrize("family", ["ranged", "ranged_ev"])
@pytest.mark.parametrize("N", SEATS)
def test_ranged_spots_accept_and_reject(family, N):
    """Floor 3.  (a) accepts every attempt on both spots with H = N hidden seats; a spot of (b) or (c) accepts some and rejects some; a
    spot of (c) accepts nothing; at least half of the spots with a hidden seat accept something."""
    (c1, w1), (c2, w2) = calls(family, N)
    S = M.S_RANGED
    for i in c1["parts"]["a"]:
        assert len(WS.check_spot(c1["holes"][i], c1["board"][i], int(c1["nboard"][i]), c1["live"][i], c1["range_of"][i], 16)[3]) == N
    assert (w1["accepted"][c1["parts"]["a"]] == S).all(), w1["accepted"].tolist()
    assert sorted(c1["range_of"][0].tolist()) == list(range(N)) and c1["range_of"][1].tolist() == c1["range_of"][0].tolist()[::-1]
    assert (c1["range_of"][c1["parts"]["b"]] == M.U).sum(axis=1).tolist() == [1, 1] and (c1["holes"][c1["parts"]["b"], N - 1] != ES.UNKNOWN).all()
    partial = np.concatenate([w1["accepted"][c1["parts"]["b"]], w2["accepted"]])
    assert ((partial > 0) & (partial < S)).any(), partial.tolist()
    assert (w2["accepted"] == 0).any(), w2["accepted"].tolist()
    assert (w1["accepted"][c1["parts"]["d"]] == S).all()
    hidden = [(c, w, i) for c, w in ((c1, w1), (c2, w2)) for i in range(len(c["nboard"]))
              if WS.check_spot(c["holes"][i], c["board"][i], int(c["nboard"][i]), c["live"][i], c["range_of"][i], len(c["weights"]))[3]]
    some = sum(int(w["accepted"][i] > 0) for c, w, i in hidden)
    assert len(hidden) >= 8 and 2 * some >= len(hidden), (some, len(hidden))
    print("%-9s N=%2d: accepted %s + %s; %d of %d spots with a hidden seat accept" % (family, N, w1["accepted"].tolist(), w2["accepted"].tolist(), some, len(hidden)))


@pytest.mark.parametrize("N", SEATS)
def test_ladders_fill_every_group_and_round_in_numpy_order(N):
    """Floor 4.  The full ladder (ev) and the fractional ladder (ev, ranged_ev (a)) yield N level records, records 0 .. N - 2 compared with
    amount > 0 and the last the last stand: every one of the ev_groups_max(N) groups of levels has work, the ragged last one included.
    From eight seats on the fractional ladder has a level whose amount np.sum and a left-to-right loop give different bits."""
    (c, w), = calls("ev", N)
    (cx, wx), _ = calls("ranged_ev", N)
    rows = [(c, w, i, "ev " + name) for name in ("ladder", "frac") for i in c["parts"][name]] + [(cx, wx, i, "ranged_ev (a)") for i in cx["parts"]["a"]]
    assert len(rows) == 6
    for cc, ww, i, name in rows:
        assert (ww["level_seat"][i] != EV.NO_LEVEL).all() and (ww["amount"][i][:N - 1] > 0).all(), (name, i)
        assert sorted(ww["level_seat"][i].tolist()) == list(range(N)), (name, i)
        gmask = M.groups_with_work(ww["level_seat"][i], ww["amount"][i], N)
        assert bin(gmask).count("1") == M.ev_groups_max(N) == -(-(N - 1) // (3 if N <= 8 else 2)), (name, i, bin(gmask))
    assert c["bets"][c["parts"]["ladder"][0]].tolist() == sorted(c["bets"][c["parts"]["ladder"][0]].tolist())          # ascending on the turn,
    assert c["bets"][c["parts"]["ladder"][1]].tolist() == sorted(c["bets"][c["parts"]["ladder"][1]].tolist())[::-1]    # descending on the flop
    plain, dense = M.frac_ladder(N, M.FRAC_PLAIN), M.frac_ladder(N, M.FRAC_DENSE)
    assert [cc["bets"][i].tolist() for cc, _, i, name in rows if "ladder" not in name] == [plain.tolist()] + [dense.tolist()] * 3
    sensitive = {}
    for name, frac in (("plain", plain), ("dense", dense)):
        assert len(set(frac.tolist())) == N
        sensitive[name] = M.order_sensitive_levels(frac, M.full(N))
        if N >= 8:
            assert sensitive[name], "np.sum and the left-to-right sum agree on every level of the %s fractional ladder" % name
        else:
            assert not sensitive[name]
    assert N < 8 or len(sensitive["dense"]) >= 3
    dead = c["parts"]["dead_money"][0]
    live = int(c["live"][dead])
    assert not (live >> (N - 1)) & 1 and c["bets"][dead][N - 1] > max(c["bets"][dead][p] for p in range(N) if (live >> p) & 1)
    assert bin(int(c["live"][c["parts"]["one_live"][0]])).count("1") == 1
    print("ev        N=%2d: %d groups of %d levels; levels of the fractional ladders that round differently left to right: %s; dead-money spot live %s"
          % (N, M.ev_groups_max(N), M.ev_group(N), sensitive, bin(live)))


def test_sampled_draw_counts_lie_on_both_sides_of_every_edge():
    """Floor 5.  The all-hidden pre-flop spot draws D = 2 N + 5 cards: 9 .. 37.  The spec takes a new 64-bit word every 9 draws and a new
    Philox block every 18: over the fifteen seat counts D stands at most one draw below and at most two above each of the edges 9, 18,
    27 and 36, so every word count 1 .. 5 and every block count 1 .. 3 occurs."""
    ds = []
    for N in SEATS:
        (c, w), = calls("sampled", N)
        i, = c["parts"]["all_hidden"]
        ds.append(5 - int(c["nboard"][i]) + len(M.SS.check_spot(c["holes"][i], c["board"][i], int(c["nboard"][i]), c["live"][i])[3]))
        assert ds[-1] == 2 * N + 5 and c["samples"] == 65 and not np.array_equal(c["ids"], np.arange(13))
        kinds = {float((h[(int(lv) >> np.arange(N)) & 1 == 1] == ES.UNKNOWN).mean()) for h, lv in zip(c["holes"][:12], c["live"][:12])}
        assert 0.0 in kinds and 1.0 in kinds and len(kinds) >= 3 - (N == 2) and c["nboard"][:12].tolist() == [0, 1, 2, 3, 4, 5] * 2
    for edge in (9, 18, 27, 36):
        assert any(edge - 1 <= d <= edge for d in ds) and any(edge < d <= edge + 2 for d in ds), edge
    assert {-(-d // 9) for d in ds} == {1, 2, 3, 4, 5} and {-(-d // 18) for d in ds} == {1, 2, 3}
    print("sampled  : draw counts", ds)


@pytest.mark.parametrize("N", SEATS)
def test_the_table_state_on_the_oracle(N):
    """The table recipe on the C oracle: every table reaches its street (flop, turn and river occur), from three seats on some table has a
    folded seat, no table is refused by any of the five specs, the ranged forms accept something somewhere, some table pays two levels, and
    from eight seats on some level's amount differs between np.sum and a left-to-right loop."""
    cfg = M.table_config(N)
    o = O.OracleGame(cfg["tables"], N, cfg["start_credits"], seed=cfg["seed"], table_id_base=cfg["table_id_base"])
    snap = M.table_state(o)
    assert sorted(set(snap["turn"].tolist())) == [1, 2, 3]
    folded = int((snap["states"] == 0).sum())
    assert folded or N == 2, "no folded seat on any table"
    want = M.table_want_of_snapshot(N, snap)
    assert sorted(want) == sorted(M.TABLE_PARTS)
    for name, w in want.items():
        assert not w["status"].any(), (name, w["status"].tolist())
        M.invariants(M.TABLE_PARTS[name], w, M.where_of("table_forms", N, name))
    assert want["equity_ranged"]["accepted"].any() and np.array_equal(want["equity_ranged"]["accepted"], want["ev_ranged"]["accepted"])
    levels = (want["equity_ev"]["level_seat"] != EV.NO_LEVEL).sum(axis=1)
    assert levels.max() >= 2 or N == 2
    live = ES.table_spots(snap["cards"][:, :5 + 2 * N], snap["states"], snap["turn"])[3]
    sensitive = sum(len(M.order_sensitive_levels(b, int(lv))) for b, lv in zip(snap["bets"] + snap["pending"], live))
    assert sensitive or N < 8, "no table has a level whose amount rounds differently left to right"
    print("tables    N=%2d: streets %s, folded seats %d, levels %s (%d order-sensitive), ranged accepted %s"
          % (N, snap["turn"].tolist(), folded, levels.tolist(), sensitive, want["equity_ranged"]["accepted"].tolist()))


@pytest.mark.parametrize("family", M.SPOT_FAMILIES)
def test_the_comparators_reject_one_bit(family):
    """assert_same / assert_same_bytes / invariants fail on a one-bit change of any output of the top seat."""
    N = 13
    w = M.want(family, N)[0]
    for k in M.KEYS[family]:
        other = {key: np.array(v, copy=True) for key, v in w.items()}
        flat = other[k].reshape(-1).view(np.uint8)
        flat[-1] ^= 1
        with pytest.raises(AssertionError):
            M.assert_same(family, other, w, "one bit in " + k)
        with pytest.raises(AssertionError):
            M.assert_same_bytes(family, other, w, "one bit in " + k)
    other = {key: np.array(v, copy=True) for key, v in w.items()}
    other["share"].reshape(-1)[0] += 1
    with pytest.raises(AssertionError):
        M.invariants(family, other, "one unit of share")
    M.assert_same(family, w, w, "itself")
    M.assert_same_bytes(family, w, w, "itself")
