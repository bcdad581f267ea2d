"""GPU tests of the showdown EV through the C ABI (pk_equity_ev(_d), pk_table_equity_ev(_d)): every output against the numpy restatement of
the definition (tests/ev_spec.py) -- integers equal, `amount` and `ev` bit for bit -- and against the fixture the reference's Game.end_hand
wrote; the level rules one by one, the line-148 spot, boards that play for everyone, many-task spots and sixteen-seat ladders, bad spots
inside good batches, repeatability and the stream forms, the table form against the explicit form, and the game itself as witness."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import equity_spec as ES
import ev_spec as EV
import ev_witness as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("share", "level_seat", "amount", "ev", "boards", "status")
ROYAL = [0x09, 0x0A, 0x0B, 0x0C, 0x00]                # TS JS QS KS AS: the board plays for everyone


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


def as_dict(r):
    out = {k: getattr(r, k) for k in KEYS}
    invariants(out)
    return out


def device_ev(holes, board, nboard, live, bets):
    from pokerl_amd import judger as J
    return as_dict(J.showdown_ev_batch(holes, board, nboard, live, bets))


def invariants(out):
    """On every spot of every test: a level that pays shares 720720 * boards exactly, one that does not exist has no share and no amount, the
    amounts add up to something finite, a refused spot is all zero with level_seat 0xFF."""
    ok = out["status"] == 0
    for i in np.nonzero(ok)[0]:
        rows = out["share"][i].astype(object).sum(axis=1)
        for lv in range(out["share"].shape[1]):
            exists = out["level_seat"][i, lv] != EV.NO_LEVEL
            pays = exists and out["amount"][i, lv] > 0
            assert int(rows[lv]) == (EV.SHARE_UNIT * int(out["boards"][i]) if pays else 0), (i, lv)
            assert exists or out["amount"][i, lv] == 0
    bad = ~ok
    assert not out["share"][bad].any() and not out["amount"][bad].any() and not out["ev"][bad].any() and not out["boards"][bad].any()
    assert (out["level_seat"][bad] == EV.NO_LEVEL).all() and (out["boards"][ok] > 0).all()


def one_spot(hands, board, live, bets):
    """A spot from card values: -> holes [1, n, 2], board [1, 5], nboard [1], live [1], bets [1, n]."""
    n = len(hands)
    b = np.zeros((1, 5), np.uint8)
    b[0, :len(board)] = board
    return (np.array([hands], np.uint8), b, np.array([len(board)], np.uint8), np.array([live], np.uint16), np.array([bets], np.float64).reshape(1, n))


def check_vs_spec(spot, where):
    got = device_ev(*spot)
    want = EV.batch_ev(*spot)
    EV.assert_same(got, want, where)
    return got


def deal(n, skip=()):
    """Distinct hole cards for n seats that avoid `skip`, in canonical order."""
    cards = [c for c in ES.CANON if c not in skip]
    return [[cards[2 * p], cards[2 * p + 1]] for p in range(n)]


def ladder(n):
    return [5.0 * (p + 1) for p in range(n)]


# ---------------------------------------------------------------------------------------------------------------- fixture
def test_every_fixture_spot_equals_the_spec_and_the_reference(PK):
    with open(os.path.join(ROOT, "tests", "golden", "ev_ref.json")) as f:
        spots = json.load(f)["spots"]
    for n in sorted({s["n"] for s in spots}):
        group = [s for s in spots if s["n"] == n]
        holes = np.array([s["holes"] for s in group], np.uint8)
        board = np.array([s["board"] + [0] * (5 - len(s["board"])) for s in group], np.uint8)
        nboard = np.array([len(s["board"]) for s in group], np.uint8)
        live = np.array([s["live"] for s in group], np.uint16)
        bets = np.array([s["bets"] for s in group], np.float64)
        got = device_ev(holes, board, nboard, live, bets)
        EV.assert_same(got, EV.batch_ev(holes, board, nboard, live, bets), "fixture n=%d" % n)
        assert not got["status"].any()
        for i, s in enumerate(group):
            assert got["boards"][i] == s["boards"]
            EV.check_against_reference(got["ev"][i], s, "fixture n=%d spot %d" % (n, i))


# ---------------------------------------------------------------------------------------------------------------- levels
LEVEL_CASES = {
    "equal bets: one level carries all the money": (3, 0b111, [10, 10, 10]),
    "ladder at three seats": (3, 0b111, ladder(3)),
    "ladder at six seats": (6, 0b111111, ladder(6)),
    "ladder at nine seats": (9, 0b111111111, ladder(9)),
    "a live seat with bet 0": (3, 0b111, [0, 10, 10]),
    "a folded seat whose bet exceeds every live bet": (4, 0b1011, [20, 10, 50, 20]),
    "the two top live bets equal under dead money: the stable order gives it to the higher seat": (4, 0b0111, [5, 37, 37, 50]),
    "one live seat": (3, 0b010, [5, 7, 9]),
    "all bets 0": (3, 0b111, [0, 0, 0]),
    "fractional money": (6, 0b110111, [0.1, 2.5, 7.3, 100.7, 33.33, 2.5]),
}


@pytest.mark.parametrize("name", sorted(LEVEL_CASES))
def test_levels(PK, name):
    n, live, bets = LEVEL_CASES[name]
    hands = deal(n, skip=(0x00, 0x1A, 0x2B, 0x09))
    for board in ([0x00, 0x1A, 0x2B, 0x09], [0x00, 0x1A, 0x2B, 0x3C, 0x09]):          # a turn spot and a river spot
        hands = deal(n, skip=board)
        got = check_vs_spec(one_spot(hands, board, live, bets), name)
        levels = EV.levels(bets, live)
        assert [int(x) for x in got["level_seat"][0][:len(levels)]] == [lv[0] for lv in levels]
        assert float(np.sum(got["amount"][0])) == float(np.sum(np.array(bets, np.float64))) or name == "fractional money" or not levels
    if name.startswith("equal bets"):
        assert got["level_seat"][0].tolist() == [0, EV.NO_LEVEL, EV.NO_LEVEL] and got["amount"][0].tolist() == [30.0, 0.0, 0.0]
    if name.startswith("a folded seat"):
        assert got["level_seat"][0].tolist()[:3] == [1, 0, 3] and got["amount"][0][2] == 30.0 and got["share"][0][2][3] == EV.SHARE_UNIT   # the excess: to the last seat in order
    if name.startswith("the two top"):
        assert got["level_seat"][0].tolist()[:3] == [0, 1, 2] and got["share"][0][2][2] == EV.SHARE_UNIT and got["amount"][0][2] == 13.0
    if name == "one live seat":
        assert got["level_seat"][0].tolist() == [1, EV.NO_LEVEL, EV.NO_LEVEL] and got["ev"][0].tolist() == [-5.0, 14.0, -9.0]
    if name == "all bets 0":
        assert (got["level_seat"][0] == EV.NO_LEVEL).all() and not got["ev"][0].any()
    if name == "a live seat with bet 0":
        assert got["level_seat"][0].tolist()[0] == 0 and got["amount"][0][0] == 0.0 and not got["share"][0][0].any()


def test_line_148_changes_the_winners_of_a_higher_level(PK):
    """Fixture spot 0: three live seats of one rank class, the lowest bettor first with the lowest kicker, the other two with higher
    kickers.  The spec's W_1 differs from W_0 restricted to remain_1 on that board -- and the device follows the spec."""
    with open(os.path.join(ROOT, "tests", "golden", "ev_ref.json")) as f:
        s = json.load(f)["spots"][0]
    holes, bets = np.array(s["holes"], np.uint8), np.array(s["bets"], np.float64)
    lv = EV.levels(bets, s["live"])
    rank, kick = EV.spot_rankings(holes, s["board"], 5, s["live"], ES.check_spot(holes, s["board"], 5, s["live"])[1])
    w0, w1 = int(EV.level_winners(rank, kick, lv[0][2])[0]), int(EV.level_winners(rank, kick, lv[1][2])[0])
    assert len({int(r) for r in rank[:, 0]}) == 1 and kick[0, 0] < min(kick[1, 0], kick[2, 0]) and np.argmin(bets) == 0
    assert w1 != (w0 & lv[1][2])
    got = check_vs_spec(one_spot(s["holes"], s["board"], s["live"], s["bets"]), "line 148")
    assert [int(np.argmax(got["share"][0][i])) for i in (0, 1)] == [w0.bit_length() - 1, w1.bit_length() - 1]
    EV.check_against_reference(got["ev"][0], s, "line 148")


@pytest.mark.parametrize("n", [3, 16])
def test_a_board_that_plays_for_everyone_splits_every_level(PK, n):
    hands = deal(n, skip=[c for c in ES.CANON if c >> 4 == 0])            # no spade in a hand: nothing extends or shifts the board's run
    live = (1 << n) - 1
    got = check_vs_spec(one_spot(hands, ROYAL, live, ladder(n)), "royal flush on the table, n=%d" % n)
    for i in range(n - 1):
        remain = [p for p in range(n) if p >= i]
        assert all(int(got["share"][0][i][p]) == (EV.SHARE_UNIT // len(remain) if p in remain else 0) for p in range(n)), i
    assert int(got["share"][0][n - 1][n - 1]) == EV.SHARE_UNIT and got["level_seat"][0].tolist() == list(range(n))


# ---------------------------------------------------------------------------------------------------------------- enumeration
def test_heads_up_preflop_with_unequal_bets(PK):
    """1 712 304 boards: many tasks, combined through atomics."""
    got = check_vs_spec(one_spot([[0x00, 0x10], [0x0C, 0x1C]], [], 0b11, [37.0, 120.5]), "AA v KK pre-flop")
    assert got["boards"][0] == 1712304 and got["level_seat"][0].tolist() == [0, 1] and got["amount"][0].tolist() == [74.0, 83.5]


@pytest.mark.parametrize("nb,boards", [(0, 15504), (3, 136)])
def test_sixteen_seat_ladder(PK, nb, boards):
    """Pre-flop: pool 20, all five combination levels moving under 15 pot levels (eight groups of levels); the flop: 136 boards."""
    board = [0x00, 0x1A, 0x2B][:nb]
    hands = deal(16, skip=board)
    bets = [7.5 * (p + 1) + 0.25 * (p % 3) for p in range(16)]
    got = check_vs_spec(one_spot(hands, board, 0xFFFF, bets), "sixteen-seat ladder nb=%d" % nb)
    assert got["boards"][0] == boards and (got["level_seat"][0] == np.arange(16)).all()


# ---------------------------------------------------------------------------------------------------------------- batches
def mixed_batch():
    rng = np.random.default_rng(9)
    n, m = 6, 40
    holes, board, nboard, live = ES.random_spots(rng, n, m, unknown=False)
    nboard[:] = rng.integers(3, 6, m)
    live[:] |= 1
    bets = rng.choice([0.0, 5.0, 10.0, 20.0, 37.0, 50.0, 12.25], (m, n))
    return holes, board, nboard, live, bets


def test_bad_spots_inside_a_batch(PK):
    holes, board, nboard, live, bets = mixed_batch()
    clean = check_vs_spec((holes, board, nboard, live, bets), "clean batch")
    assert not clean["status"].any() and len({int((r != EV.NO_LEVEL).sum()) for r in clean["level_seat"]}) >= 4
    h, b, nb, lv, be = holes.copy(), board.copy(), nboard.copy(), live.copy(), bets.copy()
    want = {}
    h[3, 0, 0] = 0x4F; want[3] = ES.BAD_CARD                                 # a byte that is no card
    h[7, 0] = ES.UNKNOWN; want[7] = ES.BAD_CARD                              # unknown at a live seat
    nb[15] = 5; b[15, 4] = h[15, 2, 1]; want[15] = ES.DUP_CARD               # a card twice
    lv[19] = 0; want[19] = ES.NO_LIVE
    nb[23] = 6; want[23] = ES.BAD_NBOARD
    be[27, 2] = -0.5; want[27] = EV.BAD_BET
    be[29, 5] = np.nan; want[29] = EV.BAD_BET
    be[31, 0] = np.inf; lv[31] = 0; want[31] = EV.BAD_BET | ES.NO_LIVE
    be[33, 1] = -np.inf; h[33, 1, 1] = h[33, 1, 0]; want[33] = EV.BAD_BET | ES.DUP_CARD
    got = check_vs_spec((h, b, nb, lv, be), "bad spots vs spec")
    for i in range(len(lv)):
        if i in want:
            assert got["status"][i] == want[i], i
        else:
            EV.assert_same({k: got[k][i:i + 1] for k in KEYS}, {k: clean[k][i:i + 1] for k in KEYS}, "neighbour %d" % i)
    # the table-form bits cannot occur in an explicit call, and BAD_BET is the value range equity gives PK_EQ_PREFLOP
    assert not (got["status"] & (ES.IN_FLIGHT | ES.BAD_TABLE)).any()


def test_repeatable_and_stream_forms_agree(PK):
    from pokerl_amd import hipmem
    from pokerl_amd import judger as J
    holes, board, nboard, live, bets = mixed_batch()
    nboard[:2] = 0                                                            # two pre-flop spots among them: many tasks
    live[:2] = 0b11
    m, n = bets.shape
    a = device_ev(holes, board, nboard, live, bets)
    EV.assert_same(device_ev(holes, board, nboard, live, bets), a, "same inputs twice")
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0             # hipStreamNonBlocking: a caller's own stream
    ins = [hipmem.DeviceBuffer(x.nbytes).upload(x) for x in (holes, board, nboard, live, bets)]
    sizes = dict(share=(np.uint64, m * n * n), level_seat=(np.uint8, m * n), amount=(np.float64, m * n), ev=(np.float64, m * n), boards=(np.uint32, m), status=(np.uint8, m))
    outs = {k: hipmem.DeviceBuffer(np.dtype(dt).itemsize * cnt) for k, (dt, cnt) in sizes.items()}

    def fetch(keys):
        return {k: outs[k].download(sizes[k][0], sizes[k][1]).reshape(np.asarray(a[k]).shape) for k in keys}
    for rep in range(2):
        J.showdown_ev_d(n, m, *[x.ptr for x in ins], outs["status"].ptr, outs["share"].ptr, outs["level_seat"].ptr, outs["amount"].ptr, outs["ev"].ptr,
                        outs["boards"].ptr, stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        EV.assert_same(fetch(KEYS), a, "device form on a caller's stream, pass %d" % rep)
    # only ev and status wanted: the share counters live in the work space
    outs["ev"].upload(np.full(m * n, 7.0))
    J.showdown_ev_d(n, m, *[x.ptr for x in ins], outs["status"].ptr, ev_d=outs["ev"].ptr, stream=stream)
    assert hip.hipStreamSynchronize(stream) == 0
    d = fetch(("ev", "status"))
    assert np.array_equal(d["ev"].view(np.uint64), a["ev"].view(np.uint64)) and not d["status"].any()
    for x in ins + list(outs.values()):
        x.free()
    # sixteen calls with a synchronisation after each, at a size whose work space exceeds a megabyte: EVERY call must deliver (section 3.1:
    # the stream-ordered allocator once handed such a loop a fresh mapping on which the task count was still zero)
    m2 = 4096
    h2 = np.tile(np.array([[[0x00, 0x10], [0x0C, 0x1C]]], np.uint8), (m2, 1, 1))
    b2 = np.tile(np.array([[0x21, 0x35, 0x09, 0, 0]], np.uint8), (m2, 1))
    be2 = np.tile(np.array([[37.0, 120.5]]), (m2, 1))
    ins = [hipmem.DeviceBuffer(x.nbytes).upload(x) for x in (h2, b2, np.full(m2, 3, np.uint8), np.full(m2, 3, np.uint16), be2)]
    outs = [hipmem.DeviceBuffer(m2), hipmem.DeviceBuffer(m2 * 4 * 8), hipmem.DeviceBuffer(m2 * 2 * 8)]
    one = EV.spot_ev(h2[0], [int(x) for x in b2[0]], 3, 3, be2[0])
    for rep in range(16):
        outs[1].upload(np.full(m2 * 4, 7, np.uint64))
        outs[2].upload(np.full(m2 * 2, 7.0))
        J.showdown_ev_d(2, m2, *[x.ptr for x in ins], outs[0].ptr, share_d=outs[1].ptr, ev_d=outs[2].ptr, stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        assert (outs[1].download(np.uint64, m2 * 4).reshape(m2, 2, 2) == one["share"][None]).all(), rep
        assert (outs[2].download(np.float64, m2 * 2).reshape(m2, 2).view(np.uint64) == one["ev"].view(np.uint64)[None]).all(), rep
        assert not outs[0].download(np.uint8, m2).any(), rep
    assert hip.hipStreamDestroy(stream) == 0
    for x in ins + outs:
        x.free()


# ---------------------------------------------------------------------------------------------------------------- table form
def explicit_from_getters(g, tables=None):
    holes, board, nboard, live = ES.table_spots(g.deck, g.player_states, g.turn)
    bets = g.bets + g.pending_bets
    if tables is not None:
        holes, board, nboard, live, bets = holes[tables], board[tables], nboard[tables], live[tables], bets[tables]
    return device_ev(holes, board, nboard, live, bets), (live, bets)


@pytest.mark.parametrize("tables,n,steps", [(64, 6, 9), (200, 3, 5)])
def test_table_form_equals_explicit_form(PK, tables, n, steps):
    """After a few random steps: the whole batch without an index array and with one (permuted, repeated indices) against the explicit form
    fed from the getters; the call writes nothing to the handle."""
    g = PK.VecGame(tables, num_players=n, seed=77 + n)
    g.reset()
    g.rollout(steps, policy=0, auto_reset=True, fused=True)
    before = g.save()
    want, _ = explicit_from_getters(g)
    assert not want["status"].any()
    r = g.equity_ev()
    EV.assert_same(as_dict(r), want, "table form %dx%d, no index array" % (tables, n))
    assert np.array_equal(r.bets, g.bets + g.pending_bets) and np.array_equal(r.payout, r.ev + r.bets)
    rng = np.random.default_rng(n)
    perm = rng.permutation(tables)[:tables // 2]
    perm = np.concatenate([perm, perm[:10], perm[:1]]).astype(np.int32)
    EV.assert_same(as_dict(g.equity_ev(perm)), {k: want[k][perm] for k in KEYS}, "table form %dx%d, index array" % (tables, n))
    assert g.save().tobytes() == before.tobytes()
    g.close()


@pytest.mark.parametrize("shape", sorted(W.WITNESS))
def test_table_form_on_deep_hands_and_the_game_as_witness(PK, shape):
    """The never-fold caller on ladder stacks drives raised multi-way hands to later streets: the table form equals the explicit form, at
    least one table has three live seats and two distinct live bet levels.  Then the witness: the tables at the start of the river's betting
    round (boards = 1) are played out by seats that check, which adds no money, and the payoffs the step kernel pays equal the recorded ev
    bit for bit -- on at least one table with a side pot (the seed was chosen on the CPU oracle: tests/test_equity_ev_host.py plays the
    same hands there)."""
    from hip_backend import HipBackend
    tables, n = shape
    seed, steps = W.WITNESS[shape]
    b = HipBackend(tables, n, start_credits=W.ladder_stacks(n), seed=seed)
    snap = W.deep_steps(b, steps)
    g = b.g
    want, (live, bets) = explicit_from_getters(g)
    r = g.equity_ev()
    got = as_dict(r)
    EV.assert_same(got, want, "deep hands %dx%d" % shape)
    ll = W.live_levels(live, bets)
    assert any(a >= 3 and c >= 2 for a, c in ll)
    cand = W.river_candidates(snap)
    side = [t for t in cand if ll[t][0] >= 3 and ll[t][1] >= 2]
    assert side, [ll[t] for t in cand]
    assert all(got["status"][t] == 0 and got["boards"][t] == 1 for t in cand)
    assert all((got["level_seat"][t] != EV.NO_LEVEL).sum() >= 2 for t in side)
    one = g.equity_ev(np.array(side[:1]))                                     # ... and the spec on one side-pot table
    holes, board, nboard, lv = ES.table_spots(g.deck, g.player_states, g.turn)
    t0 = side[0]
    EV.assert_same({k: np.asarray(getattr(one, k)) for k in KEYS}, EV.batch_ev(holes[t0:t0 + 1], board[t0:t0 + 1], nboard[t0:t0 + 1], lv[t0:t0 + 1], bets[t0:t0 + 1]), "spec")
    recorded = got["ev"].copy()
    paid = W.play_out_passively(b, cand)
    for t in cand:
        assert np.array_equal(paid[t].view(np.uint64), recorded[t].view(np.uint64)), (t, paid[t], recorded[t], bets[t])
    g.close()


def test_never_reset_handle_and_bad_indices_report_a_status(PK):
    g = PK.VecGame(64, num_players=6)
    r = g.equity_ev()
    assert (r.status == ES.DUP_CARD).all() and not r.share.any() and not r.boards.any() and (r.level_seat == EV.NO_LEVEL).all() and not r.ev.any()
    g.reset()
    r = g.equity_ev(np.array([0, 64, -1, 5, 2 ** 31 - 1], np.int64))
    invariants({k: getattr(r, k) for k in KEYS})
    assert r.status.tolist() == [0, ES.BAD_TABLE, ES.BAD_TABLE, 0, ES.BAD_TABLE]
    assert r.boards[0] == r.boards[3] > 0 and not r.payout[[1, 2, 4]].any()
    assert r[0].levels == [(int(s), float(a)) for s, a in zip(r.level_seat[0], r.amount[0]) if s != EV.NO_LEVEL] and len(r[0].levels) >= 1
    single = PK.Game(num_players=3)
    with pytest.raises(ValueError):
        single.equity_ev()
    single.reset()
    e = single.equity_ev()
    assert e.status == 0 and e.boards == 46 * 45 * 44 * 43 * 42 // 120 and abs(float(np.sum(e.ev))) < 1e-9 and float(np.sum(e.payout)) > 0
    single.close()
    g.close()


def test_tables_in_flight_report_it_and_the_others_are_still_correct(PK):
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
    res = g.equity_ev()
    assert res.bets is None and res.payout is None                           # (formed from the getters, which refuse while steps are in flight)
    r = as_dict(res)
    assert (r["status"][~idle] == ES.IN_FLIGHT).all() and not r["status"][idle].any()
    act.upload(np.full(T, -1, np.int32))                                     # the drain: idle tables get no step and stay as they are
    g.step_async_d(act, flags, terr, ready, max_hands=0, auto_reset=True)
    g.sync()
    t = np.flatnonzero(idle)
    want, _ = explicit_from_getters(g, t)
    EV.assert_same({k: r[k][t] for k in KEYS}, want, "the idle tables")
    for b in (act, flags, terr, ready):
        b.free()
    g.close()


def test_showdown_ev_one_spot(PK):
    """The short stack called by two bigger ones: main-pot equity gives the wrong number, the EV pays the side pot to the right seat."""
    from pokerl_amd import judger as J
    hands, board, bets = [["AS", "AH"], ["KS", "KH"], ["QS", "QH"]], ["2C", "7D", "9H", "JC", "3S"], [10.0, 50.0, 50.0]
    r = J.showdown_ev(hands, board=board, bets=bets)
    assert r.status == 0 and r.boards == 1 and r.levels == [(0, 30.0), (1, 80.0)]
    assert r.ev.tolist() == [20.0, 30.0, -50.0] and r.payout.tolist() == [30.0, 80.0, 0.0]
    eq = J.showdown_equity(hands, board=board)
    assert eq.equity.tolist() == [1.0, 0.0, 0.0]                                       # main-pot equity: seat 0 takes "everything"
    with pytest.raises(ValueError):
        J.showdown_ev(hands, board=board + ["3S"], bets=bets)
