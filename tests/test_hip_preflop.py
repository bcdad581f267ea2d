"""GPU tests of the pre-flop matchups (pk_preflop_count / pk_preflop_matchups / pk_equity_preflop / pk_table_equity_preflop /
pk_equity_rvr_preflop: DESIGN.md section 3.10): partial counts over small board ranges against the numpy spec on every one of the
1326 x 1326 pairs (in a fresh process with a 64-board chunk, so that a range is several chunks with a ragged last one), the full table
against the CPU-made golden matchups, its identities and 2 048 heads-up pk_equity calls, and the two families that read the table against
numpy on the table -- explicit, table and device forms."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import preflop_spec as PS
import seat_matrix as SM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = PS.HOLDINGS
BAD_CARD, DUP_CARD, IN_FLIGHT, BAD_TABLE = 1, 2, 16, 32
# the partial ranges: one board at either end, and 165 boards of the lowest cards (quads and full houses on the board: ties everywhere) cut 65 + 65 + 35
LOW, PIECES = 40, (65, 65, 35)
N_LOW = sum(PIECES)

CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import pokerl_amd
from pokerl_amd import judger as J
assert pokerl_amd.device_count() >= 1
low, pieces, out = int(sys.argv[2]), [int(x) for x in sys.argv[3].split(",")], sys.argv[4]
n = sum(pieces)
res = {}
res["first_w"], res["first_t"] = J.preflop_counts(0, 1)
res["last_w"], res["last_t"] = J.preflop_counts(2598959, 1)
res["p65_w"], res["p65_t"] = J.preflop_counts(low, pieces[0])
res["all_w"], res["all_t"] = J.preflop_counts(low, n)
# the three-way split: accumulate on (into one pair of arrays) and off (fresh arrays, summed here)
acc_w, acc_t = np.zeros((1326, 1326), np.uint32), np.zeros((1326, 1326), np.uint32)
sum_w, sum_t = np.zeros((1326, 1326), np.uint32), np.zeros((1326, 1326), np.uint32)
pos = low
for p in pieces:
    J.preflop_counts(pos, p, acc_w, acc_t)
    w, t = J.preflop_counts(pos, p)
    sum_w += w; sum_t += t
    pos += p
res["acc_w"], res["acc_t"], res["sum_w"], res["sum_t"] = acc_w, acc_t, sum_w, sum_t
# an overwriting call on arrays that hold garbage: zeros included, no memset needed; n = 0 writes nothing
from pokerl_amd import _lib as L
g_w, g_t = np.full((1326, 1326), 0xDEADBEEF, np.uint32), np.full((1326, 1326), 0xDEADBEEF, np.uint32)
L.check(L.lib().pk_preflop_count(0, low, pieces[0], 0, L.ptr(g_w), L.ptr(g_t)))
res["over_w"], res["over_t"] = g_w, g_t
z = np.full((1326, 1326), 7, np.uint32)
L.check(L.lib().pk_preflop_count(0, low, 0, 0, L.ptr(z), L.ptr(z)))
res["untouched"] = np.array([int((z == 7).all())])
np.savez(out, **res)
"""


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


@pytest.fixture(scope="module")
def spec_pieces():
    """The spec's counts of the three pieces of the low range and of the two single boards: made once."""
    out, pos = [], LOW
    for p in PIECES:
        out.append(PS.counts(pos, p))
        pos += p
    return dict(pieces=out, first=PS.counts(0, 1), last=PS.counts(PS.ALL_BOARDS - 1, 1))


@pytest.fixture(scope="module")
def partial(PK, tmp_path_factory):
    """The device's partial counts, from a fresh child process with PK_PFM_CHUNK=64: 165 boards are a storing launch of one slice (32
    boards), two whole chunks and a ragged one of 5; an accumulating piece of 35 is one ragged chunk of two slices."""
    out = str(tmp_path_factory.mktemp("preflop_partial") / "counts.npz")
    env = dict(os.environ, PK_PFM_CHUNK="64")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(LOW), ",".join(str(p) for p in PIECES), out], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return np.load(out)


@pytest.fixture(scope="module")
def M(PK):
    from pokerl_amd import judger as J
    return J.preflop_matchups()


def same(a, b, where):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and (a.astype(np.uint64) == b.astype(np.uint64)).all(), (where, np.argwhere(a.astype(np.uint64) != b.astype(np.uint64))[:4].tolist())


# ------------------------------------------------------------------------------------------------------------------ partial counts
def test_partial_counts_equal_the_spec_on_every_pair(partial, spec_pieces):
    for name, want in (("first", spec_pieces["first"]), ("last", spec_pieces["last"]), ("p65", spec_pieces["pieces"][0])):
        same(partial[name + "_w"], want[0], name + " win")
        same(partial[name + "_t"], want[1], name + " tie")
    w = sum(p[0].astype(np.uint64) for p in spec_pieces["pieces"])
    t = sum(p[1].astype(np.uint64) for p in spec_pieces["pieces"])
    assert t.any() and w.any() and not w.diagonal().any() and not t[PS.shared()].any()
    # one board: of the 1 081 holdings in play, the pairs that share no card, each decided once: win + tie + win' = 1
    one = spec_pieces["first"]
    assert 2 * int(one[0].sum()) + int(one[1].sum()) == 1081 * 990 == 2 * int(partial["first_w"].sum()) + int(partial["first_t"].sum())
    same(partial["all_w"], w, "165 boards in one call, win")
    same(partial["all_t"], t, "165 boards in one call, tie")
    # the tile edges: the last rows and columns (1 326 = 10 x 128 + 46) carry counts
    assert partial["all_w"][1280:, :].any() and partial["all_w"][:, 1280:].any()


def test_one_call_equals_a_three_way_split_with_accumulate_on_and_off(partial):
    for k in ("w", "t"):
        same(partial["acc_" + k], partial["all_" + k], "accumulate on, " + k)
        same(partial["sum_" + k], partial["all_" + k], "accumulate off, " + k)
        same(partial["over_" + k], partial["p65_" + k], "overwriting garbage, " + k)
    assert partial["untouched"][0] == 1


def test_count_refuses_a_range_past_the_last_board(PK):
    from pokerl_amd import _lib as L
    from pokerl_amd import judger as J
    w = np.zeros((H, H), np.uint32)
    assert L.lib().pk_preflop_count(0, PS.ALL_BOARDS, 1, 0, L.ptr(w), L.ptr(w)) == L.PK_E_INVALID_ARG
    assert b"pk_preflop_count" in L.lib().pk_last_error(None)
    assert L.lib().pk_preflop_count_d(0, PS.ALL_BOARDS - 1, 2, 0, None, None, None) == L.PK_E_INVALID_ARG
    with pytest.raises(ValueError):
        J.preflop_counts(PS.ALL_BOARDS - 3, 4)
    assert L.lib().pk_preflop_count(0, PS.ALL_BOARDS, 0, 0, L.ptr(w), L.ptr(w)) == L.PK_OK and not w.any()


def test_count_device_form_and_either_output_alone(PK, partial):
    """The device form on the default chunk (one storing launch of 65 boards): the same bytes; win alone and tie alone."""
    from pokerl_amd import judger as J
    from pokerl_amd.hipmem import DeviceBuffer
    w_d, t_d = DeviceBuffer(H * H * 4), DeviceBuffer(H * H * 4)
    w_d.upload(np.full(H * H, 9, np.uint32)); t_d.upload(np.full(H * H, 9, np.uint32))
    J.preflop_counts_d(LOW, PIECES[0], w_d.ptr, t_d.ptr)
    J.preflop_counts_d(LOW + PIECES[0], PIECES[1] + PIECES[2], w_d.ptr, None, accumulate=True)
    J.preflop_counts_d(LOW + PIECES[0], PIECES[1] + PIECES[2], None, t_d.ptr, accumulate=True)
    import pokerl_amd.hipmem as hm
    assert hm._lib().hipDeviceSynchronize() == 0
    same(w_d.download(np.uint32, H * H).reshape(H, H), partial["all_w"], "device form, win")
    same(t_d.download(np.uint32, H * H).reshape(H, H), partial["all_t"], "device form, tie")
    w_d.free(); t_d.free()


# ------------------------------------------------------------------------------------------------------------------ the full table
def test_table_holds_every_golden_matchup(M):
    with open(os.path.join(ROOT, "tests", "golden", "preflop_matchups.json")) as f:
        gold = json.load(f)
    assert gold["boards"] == M.boards == PS.PAIR_BOARDS and len(gold["matchups"]) >= 16
    for g in gold["matchups"]:
        h, o = g["h"], g["o"]
        assert (h, o) == (PS.holding_of_values(*g["hero"]), PS.holding_of_values(*g["villain"])), g["name"]
        got = (int(M.win[h, o]), int(M.tie[h, o]), int(M.win[o, h]))
        assert got == (g["win"], g["tie"], g["lose"]), (g["name"], got)
    w1 = next(g for g in gold["matchups"] if (g["hero"], g["villain"]) == ([0x04, 0x03], [0x1C, 0x2B]))
    w2 = next(g for g in gold["matchups"] if (g["hero"], g["villain"]) == ([0x34, 0x33], [0x0C, 0x1B]))
    assert (w1["win"], w1["tie"], w1["lose"]) == (706238, 11593, 994473) and (w2["win"], w2["tie"], w2["lose"]) == (707259, 11592, 993453)


def test_table_identities_over_all_pairs(M):
    sh = PS.shared()
    assert M.win.shape == M.tie.shape == (H, H) and M.win.dtype == M.tie.dtype == np.uint32
    assert not M.win[sh].any() and not M.tie[sh].any()
    total = M.win.astype(np.int64) + M.tie + M.win.T
    assert (total[~sh] == PS.PAIR_BOARDS).all()
    assert (M.tie == M.tie.T).all()
    e = M.equity
    assert np.isnan(e[sh]).all() and not np.isnan(e[~sh]).any() and e.dtype == np.float64
    assert np.allclose(e[~sh] + e.T[~sh], 1.0, rtol=0, atol=1e-15)
    assert (M.shared == sh).all()


def test_table_equals_2048_heads_up_showdown_equity_calls(PK, M):
    from pokerl_amd import judger as J
    rng = np.random.default_rng(2048)
    m = 2048
    holes = np.zeros((m, 2, 2), np.uint8)
    hs = np.zeros((m, 2), np.int64)
    for i in range(m):
        if i < 64:                                                   # one-gappers below the 7 with random suits: 4-2, 5-3, 6-4 (rank nibble 0 is the ace)
            r = int(rng.integers(1, 4))
            a, b = r * 4 + int(rng.integers(0, 4)), (r + 2) * 4 + int(rng.integers(0, 4))
            rest = [c for c in rng.permutation(52) if c not in (a, b)]
            cards = [a, b, rest[0], rest[1]]
        else:
            cards = [int(c) for c in rng.permutation(52)[:4]]
        holes[i] = PS.CANON_V[cards].reshape(2, 2)
        hs[i] = [PS.holding_index(cards[0], cards[1]), PS.holding_index(cards[2], cards[3])]
    e = J.showdown_equity_batch(holes, np.zeros((m, 5), np.uint8), np.zeros(m, np.uint8), np.full(m, 3, np.uint16))
    assert not e.status.any() and (e.boards == PS.PAIR_BOARDS).all()
    same(M.win[hs[:, 0], hs[:, 1]], e.win[:, 0], "win of the hero")
    same(M.tie[hs[:, 0], hs[:, 1]], e.tie[:, 0], "tie")
    same(M.win[hs[:, 1], hs[:, 0]], e.win[:, 1], "win of the villain")


def test_second_call_returns_the_same_bytes_and_the_device_form_too(PK, M):
    from pokerl_amd import judger as J
    from pokerl_amd.hipmem import DeviceBuffer
    import pokerl_amd.hipmem as hm
    again = J.preflop_matchups()
    assert again.win.tobytes() == M.win.tobytes() and again.tie.tobytes() == M.tie.tobytes()
    w_d, t_d = DeviceBuffer(H * H * 4), DeviceBuffer(H * H * 4)
    J.preflop_matchups_d(w_d.ptr, None)
    J.preflop_matchups_d(None, t_d.ptr)
    J.preflop_matchups_d(None, None)
    assert hm._lib().hipDeviceSynchronize() == 0
    assert w_d.download(np.uint32, H * H).tobytes() == M.win.tobytes() and t_d.download(np.uint32, H * H).tobytes() == M.tie.tobytes()
    w_d.free(); t_d.free()


# ------------------------------------------------------------------------------------------------------------------ pre-flop range equity
def hero_want(M, hero, weights):
    m = len(hero)
    out = dict(win=np.zeros((m, H), np.uint32), tie=np.zeros((m, H), np.uint32), agg=np.zeros((m, 3), np.uint64), boards=np.zeros(m, np.uint32),
               status=np.zeros(m, np.uint8))
    for i in range(m):
        w = None if weights is None else (weights[i] if np.ndim(weights) == 2 else weights)
        r = PS.hero_equity(M.win, M.tie, hero[i], w)
        for k in out:
            out[k][i] = r[k]
    return out


def random_heroes(rng, m):
    return np.array([PS.CANON_V[rng.permutation(52)[:2]] for _ in range(m)], np.uint8)


@pytest.mark.parametrize("wform", ["none", "shared", "spot"])
def test_explicit_spots_equal_numpy_on_the_table(PK, M, wform):
    from pokerl_amd import judger as J
    rng = np.random.default_rng(len(wform))
    m = 70
    hero = random_heroes(rng, m)
    hero[0], hero[1] = PS.CANON_V[[0, 1]], PS.CANON_V[[50, 51]]          # holdings 0 and 1325
    hero[7] = [0x4A, 0x01]                                              # no card
    hero[8] = [0x05, 0xFF]                                              # 0xFF
    hero[9] = [0x21, 0x21]                                              # the same card twice
    hero[10] = [0x0D, 0x0D]                                             # no card, twice: BAD_CARD alone
    weights = None
    if wform == "shared":
        weights = rng.integers(0, 65536, H).astype(np.uint16)
    elif wform == "spot":
        weights = rng.integers(0, 300, (m, H)).astype(np.uint16)
        weights[3] = 0                                                  # a zero row
        weights[4] = 65535                                              # the largest aggregate
    want = hero_want(M, hero, weights)
    assert want["status"][7:11].tolist() == [BAD_CARD, BAD_CARD, DUP_CARD, BAD_CARD] and not want["status"][:7].any()
    r = J.preflop_equity_batch(hero, weights)
    for k, v in want.items():
        same(getattr(r, k), v, "%s weights, %s" % (wform, k))
    ok = want["status"] == 0
    assert (r.valid.sum(axis=1)[ok] == 1225).all() and not r.valid[~ok].any() and not r.win[~r.valid].any()
    if wform == "spot":
        assert not r.agg[3].any() and int(r.agg[4, 2]) == 65535 * 1225 * PS.PAIR_BOARDS and r.strength[3] == 0.0
    only = J.preflop_equity_batch(hero, weights, per_holding=False)
    assert only.win is None
    same(only.agg, want["agg"], "aggregates alone")
    one = J.preflop_equity([int(x) for x in hero[2]], None if weights is None else (weights[2] if wform == "spot" else weights))
    same(one.agg, want["agg"][2], "one spot")
    assert 0.0 < one.strength < 1.0
    with pytest.raises(ValueError):
        J.preflop_equity([0x21, 0x21])


def game_at_every_turn(PK, n, seed):
    T = 165
    for steps in (37, 61, 9, 23, 47):
        g = PK.VecGame(T, num_players=n, seed=seed + steps)
        g.reset()
        g.rollout(steps, policy=0, auto_reset=True, fused=True)
        if set(g.turn.tolist()) == {0, 1, 2, 3}:
            return g
        g.close()
    raise AssertionError("no rollout length left tables at every turn")


@pytest.mark.parametrize("shape", ["full", "spread"])
@pytest.mark.parametrize("n", [2, 6, 16])
def test_table_form_equals_the_spec_from_the_getters(PK, M, monkeypatch, n, shape):
    SM.use_shape(monkeypatch, shape)
    g = game_at_every_turn(PK, n, 500 + n)
    T = g.num_tables
    assert g.wave_shape[0] == (64 if shape == "full" else SM.tpb_rule(T))
    before = g.save()
    deck, active = g.deck, g.active_player.astype(np.int64)
    rng = np.random.default_rng(n)
    weights = rng.integers(0, 65536, H).astype(np.uint16)
    rows = np.arange(T)
    for observer, who in (("active", active), (n - 1, np.full(T, n - 1, np.int64))):
        hero = np.stack([deck[rows, 5 + 2 * who], deck[rows, 6 + 2 * who]], axis=1)
        want = hero_want(M, hero, weights)
        assert not want["status"].any()                               # tables at turns 0 .. 3 alike: the board is not read
        r = g.equity_preflop(observer=observer, weights=weights, per_holding=True)
        for k, v in want.items():
            same(getattr(r, k), v, "%d seats %s observer %r, %s" % (n, shape, observer, k))
        assert (r.valid.sum(axis=1) == 1225).all()
        pick = np.array([3, 3, T - 1, T, 0, -1, 7, 3], np.int64)         # repeated and out-of-range indices
        okp = (pick >= 0) & (pick < T)
        r = g.equity_preflop(observer=observer, weights=weights, tables=pick, per_holding=True)
        assert r.status.tolist() == [0 if o else BAD_TABLE for o in okp]
        for k, v in want.items():
            same(getattr(r, k)[okp], v[pick[okp]], "index array, " + k)
            assert not np.asarray(getattr(r, k))[~okp].any() or k == "status"
        only = g.equity_preflop(observer=observer, weights=weights)
        assert only.win is None
        same(only.agg, want["agg"], "aggregates alone")
    assert g.save().tobytes() == before.tobytes()                      # the calls wrote nothing to the handle
    with pytest.raises(ValueError):
        g.equity_preflop(observer=None)
    with pytest.raises(ValueError):
        g.equity_preflop(observer=n)
    from pokerl_amd import _lib as L
    agg = np.zeros((T, 3), np.uint64)
    assert g._lib.pk_table_equity_preflop(g._h, None, T, L.OBSERVER_NONE, None, 0, L.ptr(agg), None, None, None, None) == L.PK_E_INVALID_ARG
    assert g._lib.pk_table_equity_preflop_d(g._h, None, T, n, None, 0, None, None, None, None, None) == L.PK_E_INVALID_ARG
    assert not agg.any()
    g.close()


def test_never_dealt_tables_the_device_form_and_the_single_game(PK, M):
    from pokerl_amd.hipmem import DeviceBuffer
    g = PK.VecGame(64, num_players=6)
    r = g.equity_preflop(per_holding=True)
    assert ((r.status & DUP_CARD) != 0).all() and not r.win.any() and not r.boards.any() and not r.agg.any()
    g.reset()
    deck, active = g.deck, g.active_player.astype(np.int64)
    hero = np.stack([deck[np.arange(64), 5 + 2 * active], deck[np.arange(64), 6 + 2 * active]], axis=1)
    want = hero_want(M, hero, None)
    agg_d, st_d, b_d = DeviceBuffer(64 * 24), DeviceBuffer(64), DeviceBuffer(64 * 4)
    g.equity_preflop_d(agg_d=agg_d, status_d=st_d, boards_d=b_d)
    g.sync()
    same(agg_d.download(np.uint64, 64 * 3).reshape(64, 3), want["agg"], "device form, agg")
    assert not st_d.download(np.uint8, 64).any() and (b_d.download(np.uint32, 64) == PS.PAIR_BOARDS).all()
    for b in (agg_d, st_d, b_d):
        b.free()
    g.close()
    single = PK.Game(num_players=3)
    with pytest.raises(ValueError):
        single.equity_preflop()                                          # never dealt
    single.reset()
    r = single.equity_preflop()
    assert r.status == 0 and r.boards == PS.PAIR_BOARDS and 0.0 < r.strength < 1.0 and r.win.shape == (H,)
    single.close()


def test_tables_in_flight_report_it_and_the_others_are_still_correct(PK, M):
    """Blinds far above the stacks: most steps roll on through further hands and stay in flight after a bounded launch."""
    from pokerl_amd.hipmem import DeviceBuffer
    T, N = 512, 3
    g = PK.VecGame(T, num_players=N, start_credits=2, big_blind=40, small_blind=20, seed=4711)
    g.reset()
    act, flags, terr, ready = DeviceBuffer(T * 4), DeviceBuffer(T), DeviceBuffer(T), DeviceBuffer(T)
    for call in range(20):                                                   # (the very first call leaves steps in flight; the loop only guards that)
        g.pick_actions_d(act, 0)
        g.sync()
        a = act.download(np.int32, T)
        a[::2] = -1                                                          # every other table gets no step: returned at once, untouched
        act.upload(a)
        g.step_async_d(act, flags, terr, ready, max_hands=1, auto_reset=True)
        g.sync()
        idle = ready.download(np.uint8, T) != 0
        if (~idle).any():
            break
    assert idle[::2].all() and (~idle).any()
    e = g.equity_preflop(observer=0, per_holding=True)
    assert e.valid is None or not e.valid.any()
    assert ((e.status[~idle] & IN_FLIGHT) != 0).all() and not (e.status[idle] & IN_FLIGHT).any()
    assert not e.win[~idle].any() and not e.tie[~idle].any() and not e.agg[~idle].any() and not e.boards[~idle].any()
    act.upload(np.full(T, -1, np.int32))                                     # the drain: idle tables get no step and stay as they are
    g.step_async_d(act, flags, terr, ready, max_hands=0, auto_reset=True)
    g.sync()
    t = np.flatnonzero(idle)
    deck = g.deck
    want = hero_want(M, deck[t][:, 5:7], None)
    for k, v in want.items():
        same(np.asarray(getattr(e, k))[t], v, "the idle tables, " + k)
    for b in (act, flags, terr, ready):
        b.free()
    g.close()


# ------------------------------------------------------------------------------------------------------------------ pre-flop range vs range
@pytest.mark.parametrize("m", [1, 3, 65])
def test_range_vs_range_equals_the_integer_mat_vec(PK, M, m):
    from pokerl_amd import judger as J
    rng = np.random.default_rng(m)
    w = rng.integers(0, 65536, (m, H)).astype(np.uint16)
    w[0, rng.random(H) < 0.5] = 0
    if m > 2:
        w[1], w[2] = 65535, 0
    r = J.preflop_range_vs_range_batch(w)
    win, tie, tot = PS.rvr(M.win, M.tie, w)
    same(r.win, w.astype(np.uint64) @ M.win.astype(np.uint64).T, "win against M.win @ w")
    same(r.win, win, "win"); same(r.tie, tie, "tie"); same(r.tot, tot, "tot")
    assert (r.boards == PS.PAIR_BOARDS).all() and not r.status.any() and r.valid.all()
    if m > 2:
        assert not r.tot[2].any() and np.isnan(r.strength[2]).all() and int(r.tot[1, 0]) == 65535 * 1225 * PS.PAIR_BOARDS
    one = J.preflop_range_vs_range(w[0])
    same(one.win, win[0], "one range")
    assert 0.0 < one.against() < 1.0


def test_range_vs_range_rows_equal_the_hero_form_and_the_device_form(PK, M):
    from pokerl_amd import judger as J
    from pokerl_amd.hipmem import DeviceBuffer
    import pokerl_amd.hipmem as hm
    rng = np.random.default_rng(32)
    w = rng.integers(0, 2000, H).astype(np.uint16)
    r = J.preflop_range_vs_range(w)
    hs = rng.permutation(H)[:32]
    hero = np.stack([PS.CANON_V[PS.HOLD_A[hs]], PS.CANON_V[PS.HOLD_B[hs]]], axis=1)
    e = J.preflop_equity_batch(hero, w, per_holding=False)
    same(np.stack([r.win[hs], r.tie[hs], r.tot[hs]], axis=1), e.agg, "row h against the hero form")
    uni = J.preflop_range_vs_range()                                      # the uniform range: every starting hand's strength
    assert uni.strength.shape == (H,) and int(np.nanargmax(uni.strength)) in [PS.holding_index(a, b) for a in range(4) for b in range(a + 1, 4)]   # a pair of aces (rank nibble 0)
    out = [DeviceBuffer(2 * H * 8) for _ in range(3)]
    J.preflop_range_vs_range_d(2, None, out[0].ptr, out[1].ptr, out[2].ptr)   # weights NULL: two rows of ones
    J.preflop_range_vs_range_d(0, None, None, None, None)
    assert hm._lib().hipDeviceSynchronize() == 0
    for b, want in zip(out, (uni.win, uni.tie, uni.tot)):
        same(b.download(np.uint64, 2 * H).reshape(2, H), np.stack([want, want]), "device form, NULL weights")
        b.free()


# ------------------------------------------------------------------------------------------------------------------ forms
def test_a_call_with_no_spot_writes_nothing_and_status_alone_equals_the_full_call(PK, M):
    from pokerl_amd import _lib as L
    lib = L.lib()
    agg, win = np.full((4, 3), 7, np.uint64), np.full((4, H), 7, np.uint32)
    st, bo = np.full(4, 7, np.uint8), np.full(4, 7, np.uint32)
    hero = np.array([[0x00, 0x01], [0x4A, 0x00], [0x05, 0x05], [0x2C, 0x3C]], np.uint8)
    assert lib.pk_equity_preflop(0, 0, L.ptr(hero), None, 0, L.ptr(agg), L.ptr(win), L.ptr(win), L.ptr(bo), L.ptr(st)) == L.PK_OK
    assert lib.pk_equity_preflop_d(0, 0, None, None, 0, None, None, None, None, None, None) == L.PK_OK
    w64 = np.full((1, H), 7, np.uint64)
    assert lib.pk_equity_rvr_preflop(0, 0, None, L.ptr(w64), L.ptr(w64), L.ptr(w64)) == L.PK_OK
    assert (agg == 7).all() and (win == 7).all() and (st == 7).all() and (bo == 7).all() and (w64 == 7).all()
    assert lib.pk_equity_preflop(0, 4, None, None, 0, L.ptr(agg), None, None, None, None) == L.PK_E_INVALID_ARG and (agg == 7).all()
    # status asked for alone (the preparation kernel only) = the full call's
    assert lib.pk_equity_preflop(0, 4, L.ptr(hero), None, 0, None, None, None, None, L.ptr(st)) == L.PK_OK
    full = np.zeros(4, np.uint8)
    assert lib.pk_equity_preflop(0, 4, L.ptr(hero), None, 0, L.ptr(agg), L.ptr(win), None, L.ptr(bo), L.ptr(full)) == L.PK_OK
    assert st.tolist() == full.tolist() == [0, BAD_CARD, DUP_CARD, 0] and bo.tolist() == [PS.PAIR_BOARDS, 0, 0, PS.PAIR_BOARDS]
    assert not agg[1:3].any() and not win[1:3].any() and agg[0].all() and agg[3].all()
    g = PK.VecGame(8, num_players=4, seed=3)
    g.reset()
    a = np.full((8, 3), 7, np.uint64)
    assert g._lib.pk_table_equity_preflop(g._h, None, 0, 0, None, 0, L.ptr(a), None, None, None, None) == L.PK_OK and (a == 7).all()
    assert g._lib.pk_table_equity_preflop_d(g._h, None, 0, L.OBSERVER_ACTIVE, None, 0, None, None, None, None, None) == L.PK_OK
    s1, s2 = np.full(8, 7, np.uint8), np.full(8, 7, np.uint8)
    assert g._lib.pk_table_equity_preflop(g._h, None, 8, 1, None, 0, None, None, None, None, L.ptr(s1)) == L.PK_OK
    assert g._lib.pk_table_equity_preflop(g._h, None, 8, 1, None, 0, L.ptr(a), None, None, None, L.ptr(s2)) == L.PK_OK
    assert s1.tolist() == s2.tolist() == [0] * 8 and a.all()
    g.close()


def test_device_forms_no_spot_writes_nothing_and_status_alone_equals_the_full_call(PK, M):
    """pk_preflop_count_d with n = 0, and status asked for alone through pk_equity_preflop_d and pk_table_equity_preflop_d."""
    import ctypes as C
    from pokerl_amd import _lib as L
    from pokerl_amd import hipmem
    from pokerl_amd.hipmem import DeviceBuffer
    lib, hip = L.lib(), hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    w_d = DeviceBuffer(H * H * 4).upload(np.full(H * H, 7, np.uint32))
    for accumulate in (0, 1):
        assert lib.pk_preflop_count_d(0, 5, 0, accumulate, w_d.ptr, w_d.ptr, stream) == L.PK_OK
    assert lib.pk_preflop_matchups_d(0, None, None, stream) == L.PK_OK
    assert hip.hipStreamSynchronize(stream) == 0
    assert (w_d.download(np.uint32, H * H) == 7).all()
    hero = np.array([[0x00, 0x01], [0x4A, 0x00], [0x05, 0x05], [0x2C, 0x3C]], np.uint8)
    hero_d = DeviceBuffer(hero.nbytes).upload(hero)
    s1, s2, agg, bo = DeviceBuffer(4).upload(np.full(4, 7, np.uint8)), DeviceBuffer(4).upload(np.full(4, 7, np.uint8)), DeviceBuffer(4 * 24), DeviceBuffer(4 * 4)
    assert lib.pk_equity_preflop_d(0, 4, hero_d.ptr, None, 0, None, None, None, None, s1.ptr, stream) == L.PK_OK
    assert lib.pk_equity_preflop_d(0, 4, hero_d.ptr, None, 0, agg.ptr, None, None, bo.ptr, s2.ptr, stream) == L.PK_OK
    assert hip.hipStreamSynchronize(stream) == 0
    assert s1.download(np.uint8, 4).tolist() == s2.download(np.uint8, 4).tolist() == [0, BAD_CARD, DUP_CARD, 0]
    want = hero_want(M, hero, None)
    same(agg.download(np.uint64, 12).reshape(4, 3), want["agg"], "device form, agg")
    same(bo.download(np.uint32, 4), want["boards"], "device form, boards")
    g = PK.VecGame(8, num_players=4, seed=3)
    g.reset()
    t1, t2, tagg = DeviceBuffer(8).upload(np.full(8, 7, np.uint8)), DeviceBuffer(8).upload(np.full(8, 7, np.uint8)), DeviceBuffer(8 * 24)
    idx = np.array([0, 7, 8, -1, 3, 3, 1, 2], np.int32)                   # two indices no table has
    idx_d = DeviceBuffer(idx.nbytes).upload(idx)
    g.equity_preflop_d(8, idx_d, 1, status_d=t1)
    g.equity_preflop_d(8, idx_d, 1, agg_d=tagg, status_d=t2)
    g.sync()
    assert t1.download(np.uint8, 8).tolist() == t2.download(np.uint8, 8).tolist() == [0, 0, BAD_TABLE, BAD_TABLE, 0, 0, 0, 0]
    a = tagg.download(np.uint64, 24).reshape(8, 3)
    assert not a[2:4].any() and a[[0, 1, 4, 5, 6, 7]].all() and (a[4] == a[5]).all()
    g.close()
    assert hip.hipStreamDestroy(stream) == 0
    for b in (w_d, hero_d, s1, s2, agg, bo, t1, t2, tagg, idx_d):
        b.free()
