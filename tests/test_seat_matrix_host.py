"""CPU pre-flight of tests/test_hip_seat_matrix.py, with the oracle alone: the oracle half of every (seat count, configuration) ends within
its step budget and below the caps, contains what the configuration is there for, and the comparators of tests/seat_matrix.py reject a
one-bit change -- so a GPU case cannot pass by comparing nothing.  The figures are printed per (N, configuration) (pytest -s shows them)."""
import numpy as np
import pytest

import seat_matrix as M

T_LAST = M.T_MATRIX - 1     # a lane of the ragged wavefront (at 64 tables per wave)
CAP_SHARE = 0.05        # ladder / top_seat: at most this share of the tables may run into PK_TERR_HAND_CAP / _ENV_CAP; default and resumed: none
CROSS_SHARE = 0.75      # resumed: at least this share of the tables deals hand_serial 2^32 in every family's run


def cap_limit(kind, T):
    return 0 if kind in ("default", M.RESUMED) else int(CAP_SHARE * T)


def resumed_runs(N, T):
    """The oracle halves of the resumed families as the drivers of tests/seat_matrix.py run them, at the matrix's step counts: per family
    (snapshot before the first reset -- an env's first reset already plays the opponents in front of seat 0 --, snapshot at the end of the run)."""
    cfg = M.matrix_config(M.RESUMED, N, T)
    start = M.oracle_of(cfg).snapshot()
    *_, last = M.game_step_trace(cfg, M.k_of("game_step", M.RESUMED, N))
    yield "game_step", start, last["o"].snapshot()
    if T > 1:
        *_, last = M.game_step_trace(cfg, M.k_of("game_step_async", M.RESUMED, N))
        yield "game_step_async", start, last["o"].snapshot()
    yield "env_step", start, M.env_want(cfg, 0, M.k_of("env_step", M.RESUMED, N))[3].snapshot()
    if T > 1:
        o = M.oracle_of(cfg)
        o.reset(dealer=cfg["dealer"])
        o.rollout(M.k_of("rollout", M.RESUMED, N), cfg["policy"], True)          # (rollout_then_lockstep goes on for ten lockstep steps)
        yield "rollout", start, o.snapshot()
        o = M.oracle_of(cfg)
        o.reset(dealer=cfg["dealer"])
        o.rollout(M.k_of("rollout_call", M.RESUMED, N) + 7 + 45, 2, True)         # (rollout_call: fused, one step per launch, five deferred calls)
        yield "rollout_call", start, o.snapshot()


@pytest.mark.parametrize("N", M.RESUMED_SEATS)
def test_resumed_runs_cross_both_boundaries(N):
    """The resumed configuration is there for the 64-bit serials: in the oracle half of every family that runs it, every table's
    action-block index step_serial >> 3 starts below 2^32 and ends at or above it, and at least CROSS_SHARE of the tables end two hands, so
    that hand_serial 2^32 - 1 and 2^32 are both dealt (hand_serial ends ABOVE 2^32).  The lone table of the step and env families crosses both."""
    for T in (M.T_MATRIX, 1):
        fig = {}
        for family, snap0, snap1 in resumed_runs(N, T):
            assert (snap0["hand_serial"] == 2 ** 32 - 2).all() and (snap0["step_serial"] >> np.uint64(3) == 2 ** 32 - 1).all(), family
            blocks, hands = M.crossed(snap0, snap1)
            fig[family] = hands
            assert blocks, (family, T, "the action-block index does not cross 2^32 on every table")
            assert hands >= (CROSS_SHARE * T if T > 1 else 1), (family, T, hands, "tables that dealt hand_serial 2^32")
        print("seat matrix resumed  N=%2d T=%3d: tables that dealt hand_serial 2^32: %s" % (N, T, fig))


def test_tpb_rule_edges():
    """pk_create's rule for tables per wave, restated in seat_matrix.tpb_rule (the `spread` cases hold every handle to it): 1 up to 1 024
    tables, doubling with the batch, 64 only above 32 768 -- so no small shape fills a wave by itself."""
    assert [M.tpb_rule(T) for T in (1, 1024, 1025, 32768, 32769)] == [1, 1, 2, 32, 64]
    assert [M.tpb_rule(T) for T in (M.T_MATRIX, M.T_BATCHES, 2048, 2049, 16384, 16385, 1 << 20)] == [1, 1, 2, 4, 16, 32, 64]
    assert M.shape_demand(M.matrix_config("default", 6)) == (1, 1) and M.shape_demand(M.matrix_config("default", 6, shape="full")) == (64, 64)
    assert M.shape_demand(M.matrix_config("default", 6, 1, "part")) == (8, 8)
    assert M.batch_ranges(M.T_BATCHES, 2) == [(0, 128), (128, 197)] and M.batch_ranges(M.T_MATRIX, 8) == [(0, 64), (64, 128), (128, 165)]


@pytest.mark.parametrize("kind,N", [(kind, N) for kind in M.KINDS for N in M.SEATS] + [(M.RESUMED, N) for N in M.RESUMED_SEATS],
                         ids=lambda v: str(v))      # (the resumed configuration has cases at RESUMED_SEATS only)
def test_caps_and_content(kind, N):
    cfg = M.matrix_config(kind, N)
    T = cfg["T"]
    K_GAME, K_ENV = M.k_of("game_step", kind, N), M.k_of("env_step", kind, N)
    # ---- lockstep Game.step: the trace ends (it is a bounded loop over a terminating oracle), caps, side pots
    capped, paid, resets, over_seen = np.zeros(T, bool), 0, 0, 0
    for tr in M.game_step_trace(cfg, K_GAME, before=True):
        assert not (tr["eo"] & 2).any(), (tr["s"], "game.py:473: the bounded twin would stop here and compare nothing further")
        capped |= (tr["eo"] & M.CAPS) != 0
        resets += int(tr["over"].sum())
        over_seen += int(M.oracle_views(tr["pre"])[2].sum())
        paid = max(paid, int(M.seats_paid(tr).max()))
    fig = dict(game_capped=int(capped.sum()), game_resets=resets, seats_paid=paid, game_over_seen=over_seen)
    assert capped.sum() <= cap_limit(kind, T), fig
    assert not any((tr["eo"] & 2).any() for tr in M.game_step_trace(M.matrix_config(kind, N, 1), K_GAME)), "game.py:473 at one table"
    # ---- the same agents' rollout: finished games and showdowns from the counters
    o = M.oracle_of(cfg)
    o.reset(dealer=cfg["dealer"])
    c, err = o.rollout(K_GAME, cfg["policy"], True)
    fig.update(games=int(c[3]), showdowns=int(c[2]))
    if kind in ("default", M.RESUMED):
        assert err == 0 and c[3] >= 1 and c[2] >= 1, fig
    if kind == "ladder":
        assert paid >= min(N, 4), fig                # side pots formed: that many seats RECEIVED different non-zero amounts in one hand
        assert over_seen > 0, fig                    # ... and pot / high_bet / game_over are read on finished games
    # ---- PokerGameEnv.step, one opponent policy and one per seat
    for T_env in (T, M.T_BATCHES, 1):
        ecfg = M.matrix_config(kind, N, T_env)
        st = M.env_want(ecfg, 1 if kind == "ladder" else 0, K_ENV)[4]
        assert st["capped"] <= cap_limit(kind, T_env), (T_env, st["capped"])
        if T_env == T:
            fig.update(env_capped=st["capped"], env_done=st["done"])
            assert st["done"] > 0, fig
    pols, external = M.multi_seats(cfg)
    st = M.multi_want(cfg, pols, M.K_MULTI)[1]
    fig.update(multi_capped=st["capped"])
    assert st["capped"] <= cap_limit(kind, T), fig
    for T1 in (1,):
        c1 = M.matrix_config(kind, N, T1)
        assert M.multi_want(c1, pols, M.K_MULTI)[1]["capped"] == 0 and M.env_want(c1, 0, K_ENV)[4]["capped"] == 0
    if kind == "top_seat":
        assert N - 1 in external and (N == 2 or pols[0] != pols[N - 2])
        y = M.multi_yields(cfg, pols, external, M.K_MULTI)        # (also: the twin replay ends in the oracle's own state)
        fig.update(yields_to_top_seat=y[N - 1])
        assert y[N - 1] >= 1, fig
        ik = M.in_kernel_seats(cfg)
        assert M.env_want(cfg, ik, M.K_MULTI, seat0=0)[4]["capped"] <= cap_limit(kind, T) and (N == 2 or ik[0] != ik[N - 2])
    # ---- call-agent rollout, and the tables the snapshot / equity families start from
    o = M.oracle_of(cfg)
    o.reset(dealer=cfg["dealer"])
    c, err = o.rollout(M.k_of("rollout_call", kind, N), 2, True)
    assert err == 0 and c[0] == T * M.k_of("rollout_call", kind, N) and c[1] > 0, c
    snap = M.played_oracle(cfg, M.K_PLAYED, M.extra_call(kind, N)).snapshot()
    fig.update(past_the_flop=int((snap["turn"] >= 1).sum()))
    assert len(M.equity_tables(snap["turn"])) == M.EQUITY_FIRST, fig
    print("seat matrix %-8s N=%2d: capped share %.3f (game) %.3f (env) %.3f (multi) | %s"
          % (kind, N, fig["game_capped"] / T, fig["env_capped"] / T, fig["multi_capped"] / T, fig))


DEEP_FLOOR = 40         # deep: river hand ends among three or more seats, and hands that pay three or more amounts, in the game_step run


@pytest.mark.parametrize("N", M.SEATS)
def test_deep_caps_and_content(N):
    """The deep configuration (the never-fold caller of rng_spec.py) is there for hands the other agents do not produce: in the oracle
    half of its game_step run at least DEEP_FLOOR hand ends come at the river among three or more live seats (N = 2: at the river), at
    least DEEP_FLOOR hands pay three or more distinct amounts (N >= 3), and one raise after the flop falls per ten tables; no table of
    any family's run -- a lone table included -- meets a cap or game.py:473; the env families deliver finished episodes and hand ends
    with a non-zero reward; the multi-agent runs end below the caps; the rollout, snapshot and equity families start from tables past
    the flop."""
    cfg = M.matrix_config(M.DEEP, N)
    T = cfg["T"]
    assert cfg["base"] + T > 2 ** 32 > cfg["base"] and cfg["dealer"] == N - 1 and len(set(cfg["start"])) == N
    K_GAME = M.k_of("game_step", M.DEEP, N)
    fig = dict(river_3way=0, paid_3=0, max_paid=0, raises_after_flop=0, allin_after_flop=0, game_resets=0, ends_by_street=[0, 0, 0, 0])
    for tr in M.game_step_trace(cfg, K_GAME, before=True):
        assert not tr["eo"].any(), (tr["s"], "a cap, an invalid action or game.py:473 in the game_step run")
        assert not (tr["a"] == 0).any(), "the deep caller folded"
        was, ended = tr["was"], (tr["fo"] & 2) != 0
        live = np.isin(was["states"], (1, 2, 3)).sum(axis=1)                   # seats in the hand: active, called or all-in
        fig["river_3way"] += int((ended & (was["turn"] == 3) & (live >= min(N, 3))).sum())
        for street in range(4):
            fig["ends_by_street"][street] += int((ended & (was["turn"] == street)).sum())
        paid = M.seats_paid(tr)
        fig["paid_3"] += int((paid >= 3).sum()); fig["max_paid"] = max(fig["max_paid"], int(paid.max()))
        fig["raises_after_flop"] += int((np.isin(tr["a"], (3, 4, 5)) & (was["turn"] >= 1)).sum())
        fig["allin_after_flop"] += int(((tr["a"] == 6) & (was["turn"] >= 1)).sum())
        fig["game_resets"] += int(tr["over"].sum())
    assert fig["river_3way"] >= DEEP_FLOOR and (N == 2 or fig["paid_3"] >= DEEP_FLOOR) and 10 * fig["raises_after_flop"] >= T, fig
    assert not any(tr["eo"].any() for tr in M.game_step_trace(M.matrix_config(M.DEEP, N, 1), K_GAME)), "a cap or game.py:473 at one table"
    # ---- PokerGameEnv.step: seat 0 deep against call agents (random agents too up to six seats), 165 / 197 tables and a lone one
    K_ENV = M.k_of("env_step", M.DEEP, N)
    for opp in (2, 0) if N <= 6 else (2,):
        for T_env in (T, M.T_BATCHES, 1):
            want, _, acts, _, st = M.env_want(M.env_config(M.DEEP, N, T_env), opp, K_ENV)
            assert st["capped"] == 0 and not any(e.any() for e in st["step_terr"]), (opp, T_env, st["capped"])
            if T_env == T:
                rewarded = sum(int(((w[2] != 0) & (w[0] != 0)).sum()) for w in want)
                fig["env_done_vs_%d" % opp], fig["env_rewarded_hands_vs_%d" % opp] = st["done"], rewarded
                assert st["done"] > 0 and rewarded > 0 and not any((a == 0).any() for a in acts), fig
    # ---- one agent per seat: every seat the deep caller, and in-kernel call agents among them
    for mixed in (False, True):
        pols, external = M.deep_multi_seats(N, mixed)
        assert all(p in (2, 14) for p in pols) and (mixed or len(external) == N - 1)
        for T1 in (T, 1):
            st = M.multi_want(M.matrix_config(M.DEEP, N, T1), pols, M.K_MULTI)[1]
            assert st["capped"] == 0, (mixed, T1, st["capped"])
    # ---- the tables the rollout_from_deep, snapshot and equity families start from, and the call agents' rollout from there
    o = M.played_oracle(cfg, M.k_of("played", M.DEEP, N))
    snap = o.snapshot()
    fig.update(past_the_flop=int((snap["turn"] >= 1).sum()), allin_or_broke_seats=int(np.isin(snap["states"], (3, M.PS_BROKEN)).any(axis=1).sum()))
    assert len(M.equity_tables(snap["turn"])) == M.EQUITY_FIRST and fig["allin_or_broke_seats"] > 0, fig
    c, err = o.rollout(M.K_ROLLOUT, 2, True)
    fig.update(rollout_hands=int(c[1]), rollout_showdown_evals=int(c[2]))
    assert err == 0 and c[0] == T * M.K_ROLLOUT and c[1] > 0 and c[2] > 0, fig
    print("seat matrix deep     N=%2d: %s" % (N, fig))


def test_the_top_seat_configuration_wraps_the_table_ids():
    cfg = M.matrix_config("top_seat", 16)
    assert cfg["base"] + cfg["T"] > 2 ** 32 > cfg["base"] and cfg["top"] == 15
    assert M.T_MATRIX % 64 == 37 and M.T_MATRIX // 64 == 2 and M.T_BATCHES == 3 * 64 + 5


# ------------------------------------------------------------------ the comparators reject a one-bit change
def _flip_low_bit(x):
    x.view(np.uint64)[...] ^= np.uint64(1)


def test_comparators_reject_one_bit():
    cfg = M.matrix_config("default", 6)
    want, rows, acts, o, _ = M.env_want(cfg, 0, 6)
    k = next(i for i, w in enumerate(want) if w[0].any())
    good = tuple(x.copy() for x in want[k])
    M.assert_delivered(good, want[k], "unchanged")
    t = int(np.argmax(want[k][0] != 0))
    bad = tuple(x.copy() for x in want[k])
    _flip_low_bit(bad[0][t:t + 1])                              # the low mantissa bit of one delivered reward
    assert bad[0][t] != want[k][0][t] and abs(bad[0][t] - want[k][0][t]) < 1e-12
    with pytest.raises(AssertionError, match="reward"):
        M.assert_delivered(bad, want[k], "reward bit")
    bad = tuple(x.copy() for x in want[k])
    bad[3][T_LAST] ^= 1                                         # one terr byte
    with pytest.raises(AssertionError, match="terr"):
        M.assert_delivered(bad, want[k], "terr byte")
    # ... of the [K, T] form the bounded drivers index, too
    W = [np.stack([w[i] for w in want]) for i in range(4)]
    idx, cnt = np.arange(cfg["T"]), np.full(cfg["T"], k)
    got = [x[cnt, idx].copy() for x in W]
    M.assert_delivered(tuple(got), tuple(x[cnt, idx] for x in W), "unchanged, indexed")
    _flip_low_bit(got[0][t:t + 1])
    with pytest.raises(AssertionError, match="reward"):
        M.assert_delivered(tuple(got), tuple(x[cnt, idx] for x in W), "reward bit, indexed")
    # a deep trace: the low mantissa bit of a reward delivered at the end of a hand raised on every street (a fractional amount)
    dcfg = M.env_config(M.DEEP, 9)
    dwant = M.env_want(dcfg, 2, M.k_of("env_step", M.DEEP, 9))[0]
    k, t = next((k, int(np.argmax(w[0] != np.round(w[0])))) for k, w in enumerate(dwant) if (w[0] != np.round(w[0])).any())
    bad = tuple(x.copy() for x in dwant[k])
    M.assert_delivered(bad, dwant[k], "deep, unchanged")
    _flip_low_bit(bad[0][t:t + 1])
    assert dwant[k][2][t] and bad[0][t] != dwant[k][0][t] and abs(bad[0][t] - dwant[k][0][t]) < 1e-12
    with pytest.raises(AssertionError, match="reward"):
        M.assert_delivered(bad, dwant[k], "deep reward bit")
    # observation rows: one element of the dense row, one byte of the packed row
    dense, packed = M.oracle_rows(o.snapshot(), cfg["N"])
    mask = np.ones(cfg["T"], bool)
    assert M.assert_rows(dense.copy(), packed.copy(), dense, packed, mask, "unchanged") == 2 * cfg["T"]
    d = dense.copy()
    _flip_low_bit(d[T_LAST, 17:18])                             # (a stack: its low mantissa bit)
    with pytest.raises(AssertionError, match="dense row"):
        M.assert_rows(d, None, dense, packed, mask, "row element")
    mask_off = mask.copy()
    mask_off[T_LAST] = False
    M.assert_rows(d, None, dense, packed, mask_off, "row element of a table outside the mask")
    p = packed.copy()
    p[T_LAST, 2] ^= 1
    with pytest.raises(AssertionError, match="packed row"):
        M.assert_rows(None, p, dense, packed, mask, "packed byte")
    # flags / terr of Game.step
    tr = next(M.game_step_trace(cfg, 1))
    M.assert_flags(tr["fo"].copy(), tr["eo"].copy(), tr["fo"], tr["eo"], False, "unchanged")
    te = tr["eo"].copy()
    te[T_LAST] ^= 1
    with pytest.raises(AssertionError, match="flags / terr"):
        M.assert_flags(tr["fo"].copy(), te, tr["fo"], tr["eo"], False, "terr byte")


def test_oracle_rows_are_the_host_mirror_s_rows():
    """oracle_rows restates the row layouts: its packed rows unpack (pokerl_amd.unpack_obs) to its dense rows, and a StateView built from a
    dense row reads the oracle's fields."""
    from pokerl_amd.state_view import StateView, packed_dtype, unpack_obs
    for kind, N in (("default", 2), ("ladder", 9), ("top_seat", 16)):
        cfg = M.matrix_config(kind, N)
        snap = M.played_oracle(cfg, 25, 5).snapshot()
        dense, packed = M.oracle_rows(snap, N)
        assert packed.shape[1] == packed_dtype(N).itemsize
        assert unpack_obs(packed, N).tobytes() == dense.tobytes()
        for t in (0, 64, T_LAST):
            sv = StateView(dense[t], N)
            nvis = 0 if snap["turn"][t] == 0 else snap["turn"][t] + 2
            assert sv.player == snap["active"][t] and sv.turn == snap["turn"][t] and sv.minimum_raise_value == snap["min_raise"][t]
            assert [c.value for c in sv.community_cards] == snap["cards"][t, :nvis].tolist()
            assert [c.value for c in sv.player_cards] == snap["cards"][t, 5 + 2 * sv.player:7 + 2 * sv.player].tolist()
            assert sv.credits.tobytes() == snap["credits"][t].tobytes() and sv.pending_bets.tobytes() == snap["pending"][t].tobytes()
