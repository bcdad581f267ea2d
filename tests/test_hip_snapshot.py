"""GPU tests of the table snapshots (pk_save_tables(_d), pk_load_tables(_d), pk_clone_tables_d; VecGame.save / load / clone_tables,
copy.deepcopy and pickle of Game and VecGame): restores against the CPU oracle, subsets, clones within and across handles, overlap, the
redeal against its Python restatement (tests/snapshot_spec.py), refusals that leave the destination untouched, and the example."""
import copy
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import golden_util as GU
import snapshot_spec as SS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


@pytest.fixture(scope="module")
def O():
    from oracle import loader
    loader.lib()
    return loader


def state_of(g):
    """Every getter of a VecGame, keyed like the oracle's snapshot (golden_util.SNAP_FIELDS), plus the deferred-step bookkeeping."""
    onehot, _ = g.get_valid_actions()
    valid = (onehot.astype(np.uint8) << np.arange(7, dtype=np.uint8)).sum(axis=1).astype(np.uint8)
    srank, skick = g.hand_rankings
    return dict(active=g.active_player.astype(np.uint8), turn=g.turn.astype(np.uint8), dealer=g.dealer_idx.astype(np.uint8),
                sb=g.small_blind_idx.astype(np.uint8), bb=g.big_blind_idx.astype(np.uint8), hand=g.hand, states=g.player_states,
                credits=g.credits, bets=g.bets, pending=g.pending_bets, payoffs=g.payoffs, min_raise=g.minimum_raise_value, cards=g.deck,
                srank=srank, skick=skick, valid=valid, hand_serial=g.hand_serial, step_serial=g.step_serial, owed=g.owed)


def assert_same(a, b, where, keys=GU.SNAP_FIELDS, rows_a=None, rows_b=None):
    for k in keys:
        x = np.asarray(a[k]) if rows_a is None else np.asarray(a[k])[rows_a]
        y = np.asarray(b[k]) if rows_b is None else np.asarray(b[k])[rows_b]
        if not GU.bits_equal(x, y):
            y = y.astype(x.dtype)
            bad = np.argwhere(x != y) if x.shape == y.shape else [[-1]]
            raise AssertionError("%s: field %s differs (first at %s)" % (where, k, list(bad[0]) if len(bad) else "?"))


def flags_of(over, hand, turn):
    return over.astype(np.uint8) | (hand.astype(np.uint8) << 1) | (turn.astype(np.uint8) << 2)


def lockstep(g, o, policy, steps, check, where):
    for s in range(steps):
        a = o.pick_actions(policy)
        fo, eo = o.step(a)
        over, hand, turn, terr = g.step(a, strict=False)
        assert np.array_equal(flags_of(over, hand, turn), fo) and np.array_equal(terr, eo), (where, s)
        m = (fo & 1).astype(np.uint8)
        if m.any():
            o.reset(mask=m)
            g.reset(mask=m)
        if check:
            assert_same(o.snapshot(), state_of(g), "%s step %d" % (where, s))


def refused(fn, code=-1):
    from pokerl_amd import PokerlHipError
    with pytest.raises(PokerlHipError) as e:
        fn()
    assert ("error %d:" % code) in str(e.value), str(e.value)


# ------------------------------------------------------------------ 1. restore vs the oracle
@pytest.mark.parametrize("T,N", [(4096, 2), (65536, 6), (1024, 9), (256, 16)])
@pytest.mark.parametrize("policy", [0, 1], ids=["random", "allin"])
@pytest.mark.parametrize("form", ["host", "device"])
def test_restore_continues_like_the_oracle(PK, O, T, N, policy, form):
    from pokerl_amd.hipmem import DeviceBuffer
    g, o = PK.VecGame(T, num_players=N), O.OracleGame(T, N)
    g.reset()
    o.reset()
    lockstep(g, o, policy, 13, False, "before save")
    assert_same(o.snapshot(), state_of(g), "before save")
    buf = None
    if form == "host":
        blob = g.save()
    else:
        buf = DeviceBuffer(PK.snapshot_nbytes(N, T))
        g.save_d(buf)
    # off course: other actions, a masked reset, and an asynchronous rollout that may leave deferred steps behind
    g.step(g.pick_actions(2 if policy != 2 else 0), strict=False)
    g.reset(mask=(np.arange(T) % 3 == 0).astype(np.uint8))
    g.rollout(7, policy=0, counters=False)
    if form == "host":
        g.load(blob)
    else:
        g.load_d(buf)
        buf.free()
    st = state_of(g)
    assert_same(o.snapshot(), st, "right after load")
    assert not st["owed"].any()
    lockstep(g, o, policy, 10 if T >= 65536 else 24, True, "after load")
    g.close()


# ------------------------------------------------------------------ 2. subset save / load
def test_subset_save_load_touches_only_the_named_tables(PK):
    from pokerl_amd.hipmem import DeviceBuffer
    T, N = 4096, 6
    rng = np.random.default_rng(2)
    g = PK.VecGame(T, num_players=N)
    g.reset()
    g.rollout(30)
    idx = rng.choice(T, 500, replace=False).astype(np.int32)
    blob = g.save(idx)
    before = state_of(g)
    idx_d = DeviceBuffer(idx.nbytes).upload(idx)
    blob_d = DeviceBuffer(PK.snapshot_nbytes(N, len(idx)))
    g.save_d(blob_d, idx_d, m=len(idx))
    assert np.array_equal(blob_d.download(np.uint8, blob.size), blob)        # the two forms write the same bytes
    hd = SS.header(blob)
    assert (hd["magic"], hd["version"], hd["n"], hd["m"]) == (SS.MAGIC, SS.VERSION, N, len(idx))
    g.rollout(40)
    rolled = state_of(g)
    dst = rng.permutation(idx).astype(np.int32)             # the records of idx[i] go to dst[i]
    g.load(blob, dst)
    now = state_of(g)
    others = np.setdiff1d(np.arange(T), dst)
    assert_same(rolled, now, "untouched tables", keys=list(rolled), rows_a=others, rows_b=others)
    assert_same(before, now, "loaded tables", keys=list(GU.SNAP_FIELDS), rows_a=idx, rows_b=dst)
    g.rollout(40)
    dst_d = DeviceBuffer(idx.nbytes).upload(dst)
    g.load_d(blob_d, dst_d, m=len(idx))
    assert_same(before, state_of(g), "loaded tables (device form)", keys=list(GU.SNAP_FIELDS), rows_a=idx, rows_b=dst)
    for b in (idx_d, blob_d, dst_d):
        b.free()


# ------------------------------------------------------------------ 3. permuted clone within one handle
def test_permuted_clone_follows_the_source_hand(PK, O):
    from oracle import rng_spec as R
    T, N, seed = 2048, 6, 0x5EED
    rng = np.random.default_rng(3)
    g, o = PK.VecGame(T, num_players=N, seed=seed), O.OracleGame(T, N, seed=seed)
    g.reset()
    o.reset()
    lockstep(g, o, 0, 9, False, "warm")
    src = state_of(g)
    perm = rng.permutation(T).astype(np.int32)             # table t <- table perm[t], every table both a source and a destination
    g.clone_tables(np.arange(T), perm)
    now = state_of(g)
    assert_same(src, now, "right after the clone", keys=list(src), rows_a=perm)
    live = np.ones(T, bool)                                  # clone t still in the hand it was copied in
    hand_prev = now["hand"].copy()
    canon = R.canonical_deck_values()
    checked = 0
    for s in range(40):
        a = o.pick_actions(0)
        fo, eo = o.step(a)
        over, hand, turn, terr = g.step(a[perm], strict=False)
        fg = flags_of(over, hand, turn)
        assert np.array_equal(fg[live], fo[perm][live]) and np.array_equal(terr[live], eo[perm][live]), s
        ended = live & ((fo[perm] & 2) != 0)
        st, so = state_of(g), o.snapshot()
        cont = live & ~ended
        # (a step can roll on through further hands nobody can act in, game.py:607-611: those deal from the destination's own decks)
        ended = ended & (st["hand"] == hand_prev + 1) & (so["hand"][perm] == hand_prev + 1)
        hand_prev = st["hand"].copy()
        assert_same(so, st, "step %d, hand going on" % s, rows_a=perm[cont], rows_b=np.nonzero(cont)[0])
        keys = [k for k in GU.SNAP_FIELDS if k != "cards"]   # the deal of the next hand is the destination's own
        assert_same(so, st, "step %d, hand ended" % s, keys=keys, rows_a=perm[ended], rows_b=np.nonzero(ended)[0])
        for t in np.nonzero(ended & ((fo[perm] & 1) == 0))[0][:40]:
            hs = int(st["hand_serial"][t]) - 1
            deck = [canon[k] for k in R.deck_permutation(seed, int(t), hs, 5 + 2 * N)[:5 + 2 * N]]
            assert st["cards"][t].tolist() == deck, t
            checked += 1
        live &= ~((fo[perm] & 2) != 0)
        m_o, m_g = (fo & 1).astype(np.uint8), (fg & 1).astype(np.uint8)
        if m_o.any():
            o.reset(mask=m_o)
        if m_g.any():
            g.reset(mask=m_g)
        if not live.any():
            break
    assert not live.any() and checked > 100


# ------------------------------------------------------------------ 4. fan-out, across handles, overlap
def test_fan_out_one_to_65535(PK):
    T, N = 65536, 6
    g = PK.VecGame(T, num_players=N)
    g.reset()
    g.rollout(25)
    before = state_of(g)
    g.clone_tables(np.arange(1, T), [0])
    now = state_of(g)
    rows = np.zeros(T, np.int64)
    assert_same(before, now, "fan-out", keys=list(before), rows_a=rows)


def test_clone_across_handles_and_config_refusals(PK):
    N = 6
    rng = np.random.default_rng(4)
    a = PK.VecGame(1000, num_players=N, seed=11)
    b = PK.VecGame(3000, num_players=N, seed=12, table_id_base=5000)
    a.reset()
    b.reset()
    a.rollout(17)
    b.rollout(3)
    sa, sb = state_of(a), state_of(b)
    dst = rng.choice(3000, 1000, replace=False).astype(np.int32)
    b.clone_tables(dst, np.arange(1000), src=a)
    nb = state_of(b)
    assert_same(sa, nb, "cross-handle clone", keys=list(sa), rows_b=dst)
    others = np.setdiff1d(np.arange(3000), dst)
    assert_same(sb, nb, "cross-handle clone, other tables", keys=list(sb), rows_a=others, rows_b=others)
    assert_same(sa, state_of(a), "cross-handle clone, source untouched", keys=list(sa))
    for other in (PK.VecGame(1000, num_players=5, seed=11), PK.VecGame(1000, num_players=N, seed=11, big_blind=4, small_blind=2),
                  PK.VecGame(1000, num_players=N, seed=11, start_credits=[100, 100, 100, 100, 100, 101])):
        other.reset()
        so = state_of(other)
        refused(lambda: other.clone_tables(np.arange(10), np.arange(10), src=a))
        refused(lambda: other.load(a.save(np.arange(10)), np.arange(10)))
        assert_same(so, state_of(other), "refused clone / load", keys=list(so))


def test_rotation_by_one_equals_host_staging(PK):
    T, N = 4096, 9
    g = PK.VecGame(T, num_players=N)
    g.reset()
    g.rollout(21)
    src = ((np.arange(T) + 1) % T).astype(np.int32)
    blob = g.save(src)
    twin = PK.VecGame(T, num_players=N)
    twin.load(g.save())
    twin.load(blob)                                          # staged on the host: all reads before any write
    g.clone_tables(np.arange(T), src)
    a, b = state_of(g), state_of(twin)
    assert_same(b, a, "rotation", keys=list(a))


# ------------------------------------------------------------------ 5. redeal
def _turn_spread(g, N, T):
    """Every turn 0 .. 4 among the tables: 64 records each are given turn 1, 2, 3 and the finished-game turn 4 (game.py:561-564) --
    what the redeal reads of a record is its turn and its cards, and at many seats random agents rarely reach the river."""
    blob = g.save()
    cur = SS.view(blob, N, T, "cursors")
    for k, turn in enumerate((1, 2, 3, 4)):
        rows = slice(64 * k, 64 * (k + 1))
        cur[rows] = (cur[rows] & ~np.uint32(0xF << 16)) | np.uint32(turn << 16)
    g.load(blob)
    assert set(g.turn.tolist()) >= {0, 1, 2, 3, 4}


@pytest.mark.parametrize("N", [2, 6, 9, 16])
def test_redeal_matches_the_spec(PK, N):
    T, seed2, base2 = 1024, 0xABCDEF12345, 777
    rng = np.random.default_rng(N)
    g = PK.VecGame(T, num_players=N, seed=99)
    g.reset()
    g.rollout(5)
    _turn_spread(g, N, T)
    src = state_of(g)
    d = PK.VecGame(T, num_players=N, seed=seed2, table_id_base=base2)
    d.reset()
    perm = rng.permutation(T).astype(np.int32)
    for observer, nonce in ((N - 1, 5), ("active", (7 << 40) | 3)):
        d.clone_tables(perm, np.arange(T), src=g, observer=observer, nonce=nonce)
        got = state_of(d)
        assert_same(src, got, "redeal: non-card fields", keys=[k for k in src if k != "cards"], rows_b=perm)
        for i in range(T):
            t = int(perm[i])
            p = N - 1 if observer != "active" else int(src["active"][i])
            exp = SS.redeal(src["cards"][i], N, int(src["turn"][i]), p, seed2, base2 + t, nonce)
            assert np.array_equal(got["cards"][t], exp), (N, observer, i)
            nb, vis = SS.visible_positions(N, int(src["turn"][i]), p)
            assert all(got["cards"][t][v] == src["cards"][i][v] for v in vis)
            assert len(set(got["cards"][t].tolist())) == 5 + 2 * N


def test_redeal_is_uniform_and_keyed_by_the_nonce(PK):
    T, N = 65536, 6
    src = PK.VecGame(1, num_players=N, seed=3)
    src.reset()
    assert int(src.turn[0]) == 0
    d = PK.VecGame(T, num_players=N, seed=4)
    d.clone_tables(np.arange(T), [0], src=src, observer=0, nonce=1)
    deck0 = src.deck[0]
    a = d.deck
    # board slot 0 is hidden from seat 0 at turn 0: uniform over the 50 cards seat 0 has not seen
    unseen = sorted(set(range(64)) - set(deck0[5:7].tolist()))
    unseen = [v for v in unseen if (v >> 4) < 4 and (v & 15) < 13]
    assert len(unseen) == 50
    counts = np.array([(a[:, 0] == v).sum() for v in unseen], np.float64)
    assert counts.sum() == T
    e = T / 50.0
    chi2 = float(((counts - e) ** 2 / e).sum())
    assert chi2 < 100.0, chi2                                  # 49 degrees of freedom: mean 49, sd 9.9
    assert (a[:, 5:7] == deck0[5:7]).all()
    d.clone_tables(np.arange(T), [0], src=src, observer=0, nonce=1)
    assert np.array_equal(d.deck, a)                           # same nonce, same deal
    d.clone_tables(np.arange(T), [0], src=src, observer=0, nonce=2)
    assert (d.deck != a).any(axis=1).mean() > 0.99            # another nonce, another deal


# ------------------------------------------------------------------ 6. refusals leave the destination untouched
def test_refusals_write_nothing(PK):
    from pokerl_amd import _lib as L
    T, N = 256, 6
    g = PK.VecGame(T, num_players=N)
    g.reset()
    g.rollout(20)
    before = state_of(g)
    two = g.save([1, 2])
    cases = [
        lambda: g.load(two, [0, T]),                              # destination out of range
        lambda: g.load(two, [5, 5]),                              # destination twice
        lambda: g.load(two, [-1, 5]),
        lambda: g.clone_tables([3, 3], [1, 2]),
        lambda: g.clone_tables([3, T], [1, 2]),
        lambda: g.clone_tables([3, 4], [1, T + 7]),               # source out of range
        lambda: g.clone_tables([3, 4], [1, 2], observer=N),       # observer outside {-2, -1, 0 .. N-1}
        lambda: g.clone_tables([3, 4], [1, 2], observer=-3),
        lambda: g.save([0, T]),
        lambda: L.check(g._lib.pk_load_tables(g._h, L.ptr(np.array([1, 2, 3], np.int32)), 3, L.ptr(two)), g._h),   # m differs
    ]
    def corrupt(field, fn):
        b = two.copy()
        fn(SS.view(b, N, 2, field) if field else b)
        return lambda: g.load(b, [7, 8])
    cases += [
        corrupt(None, lambda b: b.__setitem__(0, b[0] ^ 1)),                                         # bad magic
        corrupt(None, lambda b: b.__setitem__(4, 9)),                                                # bad version
        corrupt("cursors", lambda c: c.__setitem__(1, (c[1] & ~np.uint32(0xF)) | np.uint32(N))),     # active nibble >= N
        corrupt("cursors", lambda c: c.__setitem__(0, c[0] | np.uint32(1 << 20))),                   # in-flight bits
        corrupt("cursors", lambda c: c.__setitem__(0, (c[0] & ~np.uint32(0xF << 16)) | np.uint32(5 << 16))),   # turn 5
        corrupt("seat_states", lambda s: s.__setitem__(0, s[0] | np.uint64(1 << 6))),                # seat bit >= N
        corrupt("seat_states", lambda s: s.__setitem__(0, s[0] | np.uint64(0x10001))),                  # seat 0 ACTIVE and CALLED
        corrupt("cards", lambda c: c.__setitem__((0, 1), (c[0, 1] & ~np.uint32(0xFF00)) | ((c[0, 1] & np.uint32(0xFF)) << np.uint32(8)))),   # a card twice
        corrupt("cards", lambda c: c.__setitem__((0, 0), (c[0, 0] & ~np.uint32(0xFF)) | np.uint32(0x0D))),   # no card
        corrupt("credits", lambda c: c.__setitem__((2, 0), np.nan)),                                 # NaN credit
        corrupt("min_raise", lambda c: c.__setitem__(1, np.inf)),
    ]
    for i, fn in enumerate(cases):
        refused(fn)
        assert_same(before, state_of(g), "refusal %d" % i, keys=list(before))
    g.load(two, [7, 8])                                            # the uncorrupted blob passes
    assert_same(before, state_of(g), "good load", keys=list(GU.SNAP_FIELDS), rows_a=[1, 2], rows_b=[7, 8])


def test_busy_while_steps_are_in_flight(PK):
    from pokerl_amd.hipmem import DeviceBuffer
    T, N = 1024, 6
    g = PK.VecGame(T, num_players=N)
    g.reset()
    g.rollout(11)
    twin = copy.deepcopy(g)
    idle = PK.VecGame(T, num_players=N)
    idle.reset()
    before_idle = state_of(idle)
    blob = g.save()
    bufs = {}
    for h in (g, twin):
        b = bufs[id(h)] = [DeviceBuffer(T * 4), DeviceBuffer(T), DeviceBuffer(T), DeviceBuffer(T)]
        h.pick_actions_d(b[0], 0)
        h.step_async_d(b[0], b[1], b[2], b[3], max_hands=1)
    refused(lambda: g.save(), -6)
    refused(lambda: g.load(blob), -6)
    refused(lambda: g.clone_tables([0], [1]), -6)
    refused(lambda: idle.clone_tables([0], [1], src=g), -6)        # busy on the SOURCE handle
    assert_same(before_idle, state_of(idle), "idle destination", keys=list(before_idle))
    for h in (g, twin):
        b = bufs[id(h)]
        h.step_async_d(None, b[1], b[2], b[3], max_hands=0)
    assert_same(state_of(twin), state_of(g), "after the drain", keys=list(GU.SNAP_FIELDS))
    for b in bufs.values():
        for x in b:
            x.free()


# ------------------------------------------------------------------ 7. Game / VecGame deepcopy and pickle
def _single_state(game):
    return (game.credits.tobytes(), game.bets.tobytes(), game.pending_bets.tobytes(), game.payoffs.tobytes(), game.player_states.tobytes(),
            game.turn, game.active_player, game.hand, game.dealer_idx, [c.value for c in game.deck], game.minimum_raise_value)


def test_game_deepcopy_and_pickle_continue_identically(PK):
    rng = np.random.default_rng(7)
    game = PK.Game(num_players=4, start_credits=200, big_blind=4, small_blind=2)
    game.reset()
    def act(gm):   # uniform over the valid moves but FOLD (everybody folding is the reference's own AssertionError, game.py:473)
        valid, _ = gm.get_valid_actions()
        moves = [a for a in np.flatnonzero(valid) if a != 0]
        return int(rng.choice(moves))
    for _ in range(23):
        game.step(act(game))
    dc = copy.deepcopy(game)
    pk = pickle.loads(pickle.dumps(game))
    assert type(dc) is PK.Game and type(pk) is PK.Game
    probe = copy.deepcopy(game)
    ref = _single_state(game)
    for _ in range(5):
        probe.step(act(probe))
    assert _single_state(game) == ref                            # stepping the copy leaves the original untouched
    hands = set()
    for s in range(200):
        a = act(game)
        outs = [g.step(a) for g in (game, dc, pk)]
        assert outs[0] == outs[1] == outs[2], s
        assert _single_state(game) == _single_state(dc) == _single_state(pk), s
        hands.add(game.hand)
        if outs[0][0]:
            for g in (game, dc, pk):
                g.reset()
    assert len(hands) > 3
    env = PK.PokerGameEnv([PK.RandomAgent(), PK.RandomAgent()], num_players=3)
    env.reset()
    gv = copy.deepcopy(env.game)
    assert type(gv) is PK.Game and [c.value for c in gv.deck] == [c.value for c in env.game.deck]
    for g in (game, dc, pk, probe, gv):
        g.close()
    env.close()


def test_vecgame_deepcopy_and_pickle_continue_identically(PK):
    T, N = 4096, 6
    v = PK.VecGame(T, num_players=N)
    v.reset()
    v.rollout(30)
    dc = copy.deepcopy(v)
    pk = pickle.loads(pickle.dumps(v))
    ref = state_of(v)
    dc.rollout(9)
    assert_same(ref, state_of(v), "original after stepping the copy", keys=list(ref))
    dc = copy.deepcopy(v)
    for s in range(200):
        a = v.pick_actions(0)
        outs = [g.step(a, strict=False) for g in (v, dc, pk)]
        for o in outs[1:]:
            assert all(np.array_equal(x, y) for x, y in zip(outs[0], o)), s
        m = outs[0][0].astype(np.uint8)
        if m.any():
            for g in (v, dc, pk):
                g.reset(mask=m)
        if s % 50 == 49:
            st = state_of(v)
            assert_same(st, state_of(dc), "deepcopy step %d" % s, keys=list(st))
            assert_same(st, state_of(pk), "pickle step %d" % s, keys=list(st))


# ------------------------------------------------------------------ 8. the example
def test_determinized_search_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "determinized_search.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("action ")]
    n_valid = [l for l in r.stdout.splitlines() if l.startswith("valid actions:")]
    assert n_valid and len(lines) == int(n_valid[0].split(":")[1].split()[0]) >= 2, r.stdout


# ------------------------------------------------------------------ tables never dealt (created, not reset yet: a zero deck)
def test_fresh_game_deepcopy_and_pickle(PK):
    game = PK.Game(num_players=4)                      # a reference Game deep-copies and pickles right after __init__
    dc = copy.deepcopy(game)
    pk = pickle.loads(pickle.dumps(game))
    assert _single_state(game) == _single_state(dc) == _single_state(pk)
    for g in (game, dc, pk):
        g.reset()
    rng = np.random.default_rng(11)
    for s in range(40):
        valid, _ = game.get_valid_actions()
        a = int(rng.choice([m for m in np.flatnonzero(valid) if m != 0]))
        outs = [g.step(a) for g in (game, dc, pk)]
        assert outs[0] == outs[1] == outs[2] and _single_state(game) == _single_state(dc) == _single_state(pk), s
        if outs[0][0]:
            for g in (game, dc, pk):
                g.reset()
    for g in (game, dc, pk):
        g.close()


def test_fresh_and_partly_reset_vecgame_save_load_and_clone(PK):
    T, N = 512, 6
    v = PK.VecGame(T, num_players=N)
    st = state_of(v)
    for c in (copy.deepcopy(v), pickle.loads(pickle.dumps(v))):
        assert_same(st, state_of(c), "fresh copy", keys=list(st))
    mask = (np.arange(T) % 2 == 0).astype(np.uint8)
    v.reset(mask=mask)                                 # only half the tables dealt
    for _ in range(5):                                 # the dealt tables play on; the others are left as created (action -1)
        a = v.pick_actions(0)
        a[1::2] = -1
        v.step(a, strict=False)
    st = state_of(v)
    assert not st["cards"][1::2].any() and st["cards"][0::2].any()
    w = PK.VecGame(T, num_players=N)
    w.load(v.save())
    assert_same(st, state_of(w), "load after a masked reset", keys=list(st))
    for c in (copy.deepcopy(v), pickle.loads(pickle.dumps(v))):
        assert_same(st, state_of(c), "copy after a masked reset", keys=list(st))
    # a clone with a redeal copies a never-dealt table unchanged, and the copy deals like the original once reset
    w.clone_tables(np.arange(T), np.arange(T), src=v, observer="active", nonce=3)
    got = state_of(w)
    assert_same(st, got, "redealt clone: never-dealt tables", keys=list(st), rows_a=np.arange(1, T, 2), rows_b=np.arange(1, T, 2))
    assert not got["cards"][1::2].any()
    v.reset()
    w.reset()
    assert_same(state_of(v), state_of(w), "both reset", keys=list(st))
