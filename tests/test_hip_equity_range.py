"""GPU tests of the range equity (pk_equity_range / pk_table_equity_range: DESIGN.md section 3.3): the fixture from the reference, random
spots against the numpy spec, the existing exact call with every holding filled in, ranges of weights, bad spots inside good batches,
the table form against the explicit form fed from the getters, the stream forms, and the sampled call on the same spot."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import equity_range_spec as RS
import equity_spec as ES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("win", "tie", "boards", "status", "agg")
H = RS.HOLDINGS


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


def as_dict(r):
    out = {k: np.asarray(getattr(r, k)) for k in KEYS}
    out["valid"] = np.asarray(r.valid)
    invariants(out)
    return out


def device_range(hero, board, nboard, dead=None, weights=None):
    from pokerl_amd import judger as J
    return as_dict(J.range_equity_batch(hero, board, nboard, dead, weights))


def invariants(out):
    """On every spot of every test: win + tie <= boards, nothing at an invalid holding, a refused spot all zero."""
    assert ((out["win"].astype(np.int64) + out["tie"]) <= out["boards"].astype(np.int64)[:, None]).all()
    assert not out["win"][~out["valid"]].any() and not out["tie"][~out["valid"]].any()
    bad = out["status"] != 0
    assert not out["boards"][bad].any() and not out["agg"][bad].any() and not out["valid"][bad].any()
    assert (out["boards"][~bad] > 0).all() and (out["valid"][~bad].sum(axis=1) > 0).all()


def assert_equal(got, want, where, keys=KEYS + ("valid",)):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and (a.astype(np.uint64) == b.astype(np.uint64)).all(), (where, k, np.argwhere(a.astype(np.uint64) != b.astype(np.uint64))[:4].tolist())


def test_every_fixture_spot_equals_the_reference(PK):
    with open(os.path.join(ROOT, "tests", "golden", "equity_range_ref.json")) as f:
        spots = json.load(f)["spots"]
    m = len(spots)
    hero = np.array([s["hero"] for s in spots], np.uint8)
    board = np.array([s["board"] + [0] * (5 - len(s["board"])) for s in spots], np.uint8)
    nboard = np.array([len(s["board"]) for s in spots], np.uint8)
    dead = np.array([s["dead"] for s in spots], np.uint64)
    want = dict(win=np.zeros((m, H), np.uint32), tie=np.zeros((m, H), np.uint32), valid=np.zeros((m, H), bool),
                boards=np.array([s["boards"] for s in spots]), status=np.zeros(m, np.uint8), agg=np.zeros((m, 3), np.uint64))
    for i, s in enumerate(spots):
        want["win"][i, s["h"]], want["tie"][i, s["h"]], want["valid"][i, s["h"]] = s["win"], s["tie"], True
        want["agg"][i] = [sum(s["win"]), sum(s["tie"]), s["boards"] * len(s["h"])]
    assert_equal(device_range(hero, board, nboard, dead), want, "the fixture in one batch")
    for i in range(m):                                            # ... and one spot at a time (m = 1: a lone workgroup)
        assert_equal(device_range(hero[i:i + 1], board[i:i + 1], nboard[i:i + 1], dead[i:i + 1]), {k: v[i:i + 1] for k, v in want.items()}, "fixture spot %d alone" % i)


# Pools by the number of sets S the villain pass enumerates, C(P, 7 - nb): the smallest legal pool (one, three and six holdings), and the
# pools next to a multiple of the wavefront (64) and of the workgroup (512).  No pool of 5 .. 47 cards has a set count that IS a multiple
# of 64 or one above one (C(P, s) mod 64 is 0 or 1 for no such P at s = 2, 3, 4); C(38, 2) = 703 is one below.  So: the nearest counts
# on either side -- river 55 | 66, 253, 496 | 528, 703, 990; turn 56 | 84, 120, 455 | 560, 15 180; flop 126, 330, 495 | 715 -- which
# leave the last lanes of a workgroup with a short range or none.
POOLS = {5: (2, 3, 11, 12, 23, 32, 33, 38, None), 4: (3, 4, 8, 9, 10, 15, 16, None), 3: (4, 5, 9, 11, 12, 13)}


@pytest.mark.parametrize("nb", [5, 4, 3])
def test_random_spots_equal_the_spec(PK, nb):
    rng = np.random.default_rng(2000 + nb)
    pools = [p for p in POOLS[nb] for _ in range(2)]
    hero, board, nboard, dead = RS.random_spots(rng, len(pools), nb, lambda i: pools[i])
    got = device_range(hero, board, nboard, dead)
    assert_equal(got, RS.batch_range(hero, board, nboard, dead), "random nb=%d" % nb)
    s = 7 - nb
    assert got["valid"][:2].sum(axis=1).tolist() == [math.comb(s, 2)] * 2 and got["boards"][:2].tolist() == [1, 1]   # the smallest pool: 1, 3, 6 holdings


def test_two_full_pool_flop_spots_equal_the_spec(PK):
    rng = np.random.default_rng(31)
    hero, board, nboard, dead = RS.random_spots(rng, 2, 3)
    got = device_range(hero, board, nboard, dead)
    assert got["boards"].tolist() == [990, 990] and got["valid"].sum(axis=1).tolist() == [1081, 1081]
    assert_equal(got, RS.batch_range(hero, board, nboard, dead), "two full-pool flop spots")


@pytest.mark.parametrize("m", [1, 65, 1100])
def test_batches_of_river_and_turn_spots_equal_the_spec(PK, m):
    """1 100 spots are more than the persistent grid has workgroups (768): a workgroup takes a second spot with the counters it cleared."""
    rng = np.random.default_rng(m)
    n_turn = m // 11
    hr, br, nr, dr = RS.random_spots(rng, m - n_turn, 5, lambda i: None if i % 3 == 0 else int(rng.integers(2, 46)))
    ht, bt, nt, dt = RS.random_spots(rng, n_turn, 4, lambda i: None if i % 10 == 0 else int(rng.integers(3, 30)))
    order = rng.permutation(m)
    hero, board, nboard, dead = (np.concatenate(x)[order] for x in ((hr, ht), (br, bt), (nr, nt), (dr, dt)))
    assert_equal(device_range(hero, board, nboard, dead), RS.batch_range(hero, board, nboard, dead), "%d river / turn spots" % m)


def test_equals_the_showdown_equity_of_every_holding_filled_in(PK):
    """Three full-pool flop spots against the existing exact call: all 1 081 holdings as two-seat spots through showdown_equity_batch."""
    from pokerl_amd import judger as J
    rng = np.random.default_rng(47)
    hero, board, nboard, dead = RS.random_spots(rng, 3, 3)
    got = device_range(hero, board, nboard)
    for i in range(3):
        hs = np.flatnonzero(got["valid"][i])
        assert len(hs) == 1081
        holes = np.zeros((len(hs), 2, 2), np.uint8)
        holes[:, 0] = hero[i]
        holes[:, 1] = PK.HOLDINGS[hs]
        e = J.showdown_equity_batch(holes, np.tile(board[i], (len(hs), 1)), np.full(len(hs), 3, np.uint8), np.full(len(hs), 3, np.uint16))
        assert not e.status.any() and (e.boards == got["boards"][i]).all() and got["boards"][i] == 990
        assert (e.win[:, 0] == got["win"][i, hs]).all() and (e.tie[:, 0] == got["tie"][i, hs]).all(), i


def test_weights(PK):
    from pokerl_amd import _lib as L
    from pokerl_amd import judger as J
    rng = np.random.default_rng(53)
    parts = [RS.random_spots(rng, 4, 5), RS.random_spots(rng, 3, 4), RS.random_spots(rng, 2, 3, 14), RS.random_spots(rng, 1, 3)]
    hero, board, nboard, dead = (np.concatenate([p[i] for p in parts]) for i in range(4))
    m = len(hero)

    def host_agg(r, w):
        w = np.broadcast_to(np.asarray(w, np.uint64), (m, H)).astype(object)
        return np.stack([(w * r["win"].astype(object)).sum(axis=1), (w * r["tie"].astype(object)).sum(axis=1),
                         r["boards"].astype(object) * (w * r["valid"].astype(object)).sum(axis=1)], axis=1)

    shared = rng.integers(0, 65536, H).astype(np.uint16)
    shared[rng.integers(0, H, 200)] = 0
    shared[rng.integers(0, H, 200)] = 65535
    per_spot = rng.integers(0, 65536, (m, H)).astype(np.uint16)
    per_spot[:, ::7] = 0
    per_spot[:, 3::7] = 65535
    per_spot[0] = 65535                                                      # the largest aggregate a river spot can have
    per_spot[-1] = 65535                                                     # ... and a full-pool flop spot: 65 535 * 990 * 1 081
    for name, w in (("shared", shared), ("per spot", per_spot), ("none", None)):
        r = device_range(hero, board, nboard, dead, w)
        want = host_agg(r, np.ones(H, np.uint16) if w is None else w)
        assert (r["agg"].astype(object) == want).all(), name
        assert r["agg"][:, 2].all()
        # ... identical when win / tie are not asked for
        only = J.range_equity_batch(hero, board, nboard, dead, w, per_holding=False)
        assert only.win is None and (only.agg == r["agg"]).all() and (only.boards == r["boards"]).all(), name
    ones = device_range(hero, board, nboard, dead, np.ones(H, np.uint16))
    none = device_range(hero, board, nboard, dead)
    assert_equal(ones, none, "NULL weights are all ones")
    assert int(none["agg"][-1, 2]) == 990 * 1081 and int(device_range(hero, board, nboard, dead, per_spot)["agg"][-1, 2]) == 65535 * 990 * 1081
    assert_equal(none, RS.batch_range(hero, board, nboard, dead), "uniform vs spec")
    assert (device_range(hero, board, nboard, dead, shared)["agg"] == RS.batch_range(hero, board, nboard, dead, shared)["agg"]).all()
    one = J.range_equity([int(x) for x in hero[0]], [int(x) for x in board[0]], weights=shared)
    assert one.strength == (float(one.agg[0]) + 0.5 * float(one.agg[1])) / float(one.agg[2]) and 0.0 <= one.strength <= 1.0
    assert np.array_equal(one.win, none["win"][0]) and L.EQ_HOLDINGS == H


def test_bad_spots_inside_a_batch(PK):
    rng = np.random.default_rng(9)
    parts = [RS.random_spots(rng, 16, 5, lambda i: None if i % 2 else 20), RS.random_spots(rng, 16, 4, lambda i: None if i % 2 else 12),
             RS.random_spots(rng, 12, 3, 10)]
    hero, board, nboard, dead = (np.concatenate([p[i] for p in parts]) for i in range(4))
    order = rng.permutation(len(hero))
    hero, board, nboard, dead = hero[order], board[order], nboard[order], dead[order]
    clean = device_range(hero, board, nboard, dead)
    assert not clean["status"].any()
    h, b, nb, d = hero.copy(), board.copy(), nboard.copy(), dead.copy()
    used = lambda i: {RS.canon_index(int(c)) for c in list(h[i]) + list(b[i, :nb[i]])}
    want = {}
    h[1, 0] = 0x4F; want[1] = RS.BAD_CARD                                     # a byte that is no card
    h[4, 1] = 0xFF; want[4] = RS.BAD_CARD                                     # 0xFF in the hero's hand
    b[7, 1] = 0xFF; want[7] = RS.BAD_CARD                                     # ... and in the board
    d[10] |= np.uint64(1) << np.uint64(52); want[10] = RS.BAD_CARD            # a dead bit that is no card
    d[13] = np.uint64(1) << np.uint64(63); want[13] = RS.BAD_CARD
    b[16, 2] = h[16, 0]; want[16] = RS.DUP_CARD                               # a card twice
    h[19, 1] = h[19, 0]; want[19] = RS.DUP_CARD
    d[22] |= np.uint64(1) << np.uint64(RS.canon_index(int(b[22, 0]))); want[22] = RS.DUP_CARD   # a board card that is also dead
    d[25] |= np.uint64(1) << np.uint64(RS.canon_index(int(h[25, 1]))); want[25] = RS.DUP_CARD   # ... a hero card
    nb[28] = 6; want[28] = RS.BAD_NBOARD
    nb[31] = 255; want[31] = RS.BAD_NBOARD
    nb[33] = 0; want[33] = RS.PREFLOP
    nb[35] = 1; want[35] = RS.PREFLOP
    nb[37] = 2; want[37] = RS.PREFLOP
    for i, left in ((39, 1), (41, 0)):                                        # fewer pool cards than the board to come plus one holding
        nb[i] = 5
        free = [k for k in range(52) if k not in used(i)]
        d[i] = sum(1 << k for k in free[left:])
        want[i] = RS.SMALL_POOL
    nb[43] = 3
    free = [k for k in range(52) if k not in used(43)]
    d[43] = sum(1 << k for k in free[3:]); want[43] = RS.SMALL_POOL           # a flop needs four
    got = device_range(h, b, nb, d)
    assert_equal(got, RS.batch_range(h, b, nb, d), "bad spots vs spec")
    for i in range(len(h)):
        if i in want:
            assert got["status"][i] == want[i] and not got["win"][i].any() and not got["tie"][i].any() and not got["agg"][i].any() and got["boards"][i] == 0, i
        else:
            assert_equal({k: v[i:i + 1] for k, v in got.items()}, {k: v[i:i + 1] for k, v in clean.items()}, "neighbour %d" % i)


def explicit_from_getters(g, who, tables=None, weights=None):
    hero, board, nboard = RS.table_spots(g.deck, g.turn, who)
    if tables is not None:
        hero, board, nboard = hero[tables], board[tables], nboard[tables]
    return device_range(hero, board, nboard, None, weights)


@pytest.mark.parametrize("n,steps", [(2, 9), (6, 37), (16, 61)])
def test_table_form_equals_explicit_form(PK, n, steps):
    T = 165
    g = PK.VecGame(T, num_players=n, seed=91 + n)
    g.reset()
    g.rollout(steps, policy=0, auto_reset=True, fused=True)
    turn = g.turn
    # every turn a table can rest at: 0 (pre-flop, refused), 1, 2, 3 = flop, turn, river.  (Game.turn never rests at 4: the hand ends there.)
    assert set(turn.tolist()) == {0, 1, 2, 3}, sorted(set(turn.tolist()))
    before = g.save()
    pre = turn == 0
    rng = np.random.default_rng(n)
    weights = rng.integers(0, 65536, H).astype(np.uint16)
    for observer, who in (("active", g.active_player), (n - 1, np.full(T, n - 1))):
        want = explicit_from_getters(g, who, weights=weights)
        assert (want["status"][pre] == RS.PREFLOP).all() and not want["status"][~pre].any()
        got = as_dict(g.equity_range(observer=observer, weights=weights, per_holding=True))
        assert_equal(got, want, "table form %dx%d observer %r" % (T, n, observer))
        only = g.equity_range(observer=observer, weights=weights)
        assert only.win is None and (only.agg == want["agg"]).all() and (only.status == want["status"]).all()
        pick = np.concatenate([rng.permutation(T)[:60], [5, 5, 5, T - 1, 0]]).astype(np.int32)   # permuted, repeated indices
        got = as_dict(g.equity_range(observer=observer, weights=weights, tables=pick, per_holding=True))
        assert_equal(got, {k: v[pick] for k, v in want.items()}, "table form %dx%d observer %r, index array" % (T, n, observer))
    assert g.save().tobytes() == before.tobytes()                            # the calls wrote nothing to the handle
    with pytest.raises(ValueError):
        g.equity_range(observer=None)
    with pytest.raises(ValueError):
        g.equity_range(observer=n)
    from pokerl_amd import _lib as L
    agg = np.zeros((T, 3), np.uint64)
    assert g._lib.pk_table_equity_range(g._h, None, T, L.OBSERVER_NONE, None, 0, L.ptr(agg), None, None, None, None) == L.PK_E_INVALID_ARG
    assert g._lib.pk_table_equity_range_d(g._h, None, T, n, None, 0, None, None, None, None, None) == L.PK_E_INVALID_ARG
    g.close()


def test_never_reset_handle_bad_indices_and_the_single_game(PK):
    g = PK.VecGame(64, num_players=6)
    r = g.equity_range(per_holding=True)
    assert ((r.status & RS.DUP_CARD) != 0).all() and not r.win.any() and not r.boards.any() and not r.agg.any()
    g.reset()
    g.rollout(40, policy=0, auto_reset=True, fused=True)
    post = int(np.flatnonzero(g.turn > 0)[0])
    r = g.equity_range(tables=np.array([post, 64, -1, post, 2 ** 31 - 1], np.int64), per_holding=True)
    assert r.status.tolist() == [0, RS.BAD_TABLE, RS.BAD_TABLE, 0, RS.BAD_TABLE]
    assert r.boards[0] == r.boards[3] > 0 and not r.win[[1, 2, 4]].any() and not r.agg[[1, 2, 4]].any() and (r.win[0] == r.win[3]).all()
    g.close()
    single = PK.Game(num_players=3)
    with pytest.raises(ValueError):
        single.equity_range()
    single.reset()
    with pytest.raises(ValueError, match="fewer than three board cards"):
        single.equity_range()                                                # pre-flop
    single.close()


def test_tables_in_flight_report_it_and_the_others_are_still_correct(PK):
    """Blinds far above the stacks: most steps roll on through further hands and stay in flight after a bounded launch."""
    from pokerl_amd.hipmem import DeviceBuffer
    T, N = 512, 3
    g = PK.VecGame(T, num_players=N, start_credits=2, big_blind=40, small_blind=20, seed=4711)
    g.reset()
    act, flags, terr, ready = DeviceBuffer(T * 4), DeviceBuffer(T), DeviceBuffer(T), DeviceBuffer(T)
    for call in range(20):                                                   # (the very first call leaves steps in flight; the loop only guards that)
        g.pick_actions_d(act, 0)                                             # a device reader: works while steps are in flight
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
    e = g.equity_range(observer=0, per_holding=True)
    assert e.valid is None or not e.valid.any()                              # (no mask while steps are in flight: the getters it is formed from refuse)
    r = {k: np.asarray(getattr(e, k)) for k in KEYS}
    assert ((r["status"][~idle] & RS.IN_FLIGHT) != 0).all() and not (r["status"][idle] & RS.IN_FLIGHT).any()
    assert not r["win"][~idle].any() and not r["tie"][~idle].any() and not r["agg"][~idle].any() and not r["boards"][~idle].any()
    act.upload(np.full(T, -1, np.int32))                                     # the drain: idle tables get no step and stay as they are
    g.step_async_d(act, flags, terr, ready, max_hands=0, auto_reset=True)
    g.sync()
    t = np.flatnonzero(idle)
    assert_equal({k: v[t] for k, v in r.items()}, explicit_from_getters(g, np.zeros(T, np.int64), t), "the idle tables", KEYS)
    for b in (act, flags, terr, ready):
        b.free()
    g.close()


def test_sixteen_repeated_calls_on_each_stream_form_agree(PK):
    """The work-space regression pattern of test_hip_equity.py: a loop of calls with a synchronisation after each, at a size whose work
    space exceeds a megabyte (40 000 spots of 32 bytes) -- EVERY call must deliver, on a caller's stream and on the pooled one."""
    from pokerl_amd import hipmem
    from pokerl_amd import judger as J
    rng = np.random.default_rng(77)
    distinct, m = 40, 40000
    hr, br, nr, dr = RS.random_spots(rng, distinct - 8, 5, lambda i: int(rng.integers(2, 46)))
    ht, bt, nt, dt = RS.random_spots(rng, 8, 4, lambda i: int(rng.integers(3, 20)))
    hero, board, nboard, dead = (np.concatenate(x) for x in ((hr, ht), (br, bt), (nr, nt), (dr, dt)))
    weights = rng.integers(0, 65536, H).astype(np.uint16)
    want = RS.batch_range(hero, board, nboard, dead, weights)
    pick = rng.integers(0, distinct, m)
    pick[:distinct] = np.arange(distinct)
    hero, board, nboard, dead = hero[pick], board[pick], nboard[pick], dead[pick]
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0             # hipStreamNonBlocking: a caller's own stream
    ins = [hipmem.DeviceBuffer(x.nbytes).upload(x) for x in (hero, board, nboard, dead, weights)]
    agg_d, boards_d, status_d = hipmem.DeviceBuffer(m * 24), hipmem.DeviceBuffer(m * 4), hipmem.DeviceBuffer(m)
    small = 64                                                               # ... and per-holding outputs for the first spots
    win_d, tie_d = hipmem.DeviceBuffer(small * H * 4), hipmem.DeviceBuffer(small * H * 4)
    for rep in range(16):
        agg_d.upload(np.full(m * 3, 7, np.uint64))
        boards_d.upload(np.full(m, 7, np.uint32))
        J.range_equity_d(m, *[x.ptr for x in ins[:4]], weights_d=ins[4].ptr, agg_d=agg_d.ptr, boards_d=boards_d.ptr, status_d=status_d.ptr, stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        assert (agg_d.download(np.uint64, m * 3).reshape(m, 3) == want["agg"][pick]).all(), rep
        assert (boards_d.download(np.uint32, m) == want["boards"][pick]).all() and not status_d.download(np.uint8, m).any(), rep
        win_d.upload(np.full(small * H, 7, np.uint32))
        J.range_equity_d(small, *[x.ptr for x in ins[:4]], win_d=win_d.ptr, tie_d=tie_d.ptr, stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        assert (win_d.download(np.uint32, small * H).reshape(small, H) == want["win"][pick[:small]]).all(), rep
        assert (tie_d.download(np.uint32, small * H).reshape(small, H) == want["tie"][pick[:small]]).all(), rep
    assert hip.hipStreamDestroy(stream) == 0
    for x in ins + [agg_d, boards_d, status_d, win_d, tie_d]:
        x.free()
    for rep in range(16):                                                    # the host form: a pooled stream
        r = J.range_equity_batch(hero, board, nboard, dead, weights, per_holding=False)
        assert (r.agg == want["agg"][pick]).all() and (r.boards == want["boards"][pick]).all() and not r.status.any(), rep


@pytest.mark.parametrize("nb", [3, 4, 5])
def test_sampled_equity_agrees_with_the_exact_fractions(PK, nb):
    """The sampled call on the same spot with the villain hidden, S = 2^20 samples: its win and tie fractions lie within
    5 * sqrt(p (1 - p) / S) of the exact ones, p = agg / agg[2] under the uniform range."""
    from pokerl_amd import judger as J
    rng = np.random.default_rng(600 + nb)
    hero, board, nboard, dead = RS.random_spots(rng, 1, nb)
    exact = J.range_equity([int(x) for x in hero[0]], [int(x) for x in board[0, :nb]])
    S = 1 << 20
    s = J.sampled_equity([[int(x) for x in hero[0]], None], [int(x) for x in board[0, :nb]], samples=S)
    assert s.samples == S
    for name, count, a in (("win", int(s.win[0]), int(exact.agg[0])), ("tie", int(s.tie[0]), int(exact.agg[1]))):
        p = a / int(exact.agg[2])
        bound = 5.0 * math.sqrt(p * (1.0 - p) / S)
        print("nb=%d %s: exact %.6f sampled %.6f deviation %.3g bound %.3g" % (nb, name, p, count / S, abs(count / S - p), bound))
        assert abs(count / S - p) <= bound, (nb, name)
