"""GPU tests of the ranged sampled equity through the C ABI (pk_equity_ranged(_d), pk_table_equity_ranged(_d)): exact equality on win, tie,
share, accepted and status with the Python restatement of the definition (tests/equity_ranged_spec.py) -- hidden patterns, every street,
dense / sparse / one-holding / dead ranges, one to nine Philox blocks, the three LDS size classes, ids, nonces, bad spots, the table form --
identities that need no spec, and convergence within five derived standard deviations to pk_equity_range and to a host enumeration."""
import ctypes as C

import numpy as np
import pytest

import equity_ranged_spec as WS
import equity_spec as ES
from equity_seat_matrix import disjoint_rows

pytestmark = pytest.mark.gpu
KEYS = WS.KEYS
COUNTS = ("win", "tie", "share")
SEED = 0x5EED0123456789AB
U = WS.UNIFORM


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


def invariants(out):
    """On every spot of every test: the shares add up to the accepted attempts exactly, win + tie <= accepted, a refused spot is all zero."""
    share = out["share"].astype(object).sum(axis=-1)
    assert (share == ES.SHARE_UNIT * out["accepted"].astype(object)).all()
    assert ((out["win"].astype(np.int64) + out["tie"]) <= out["accepted"].astype(np.int64)[..., None]).all()
    assert not out["accepted"][out["status"] != 0].any()


def as_dict(r):
    out = {k: np.asarray(getattr(r, k)) for k in KEYS}
    invariants(out)
    return out


def device_ranged(holes, board, nboard, live, samples, weights=None, range_of=None, seed=SEED, nonce=0, ids=None):
    from pokerl_amd import judger as J
    return as_dict(J.ranged_equity_batch(holes, board, nboard, live, weights, range_of, samples, seed, nonce, ids))


def spec(holes, board, nboard, live, samples, weights=None, range_of=None, nonce=0, ids=None):
    per = range_of is not None and np.ndim(range_of) == 2
    return WS.batch_equity(holes, board, nboard, live, samples, weights, range_of, per_spot=per, seed=SEED, nonce=nonce, ids=ids)


def assert_equal(got, want, where, keys=KEYS):
    for k in keys:
        a, b = np.asarray(got[k]).astype(np.uint64), np.asarray(want[k]).astype(np.uint64)
        assert a.shape == b.shape and (a == b).all(), (where, k, np.argwhere(a != b)[:4].tolist())


@pytest.fixture(scope="module")
def four():
    return WS.random_ranges(np.random.default_rng(1))


def mixed_rows(rng, m, n):
    """range_of [m, n]: rows 0 .. 3 and 0xFFFF."""
    return rng.choice(np.array([0, 1, 2, 3, U], np.uint16), (m, n))


@pytest.mark.parametrize("n", [2, 3, 6, 9, 16])
def test_random_spots_equal_the_spec(PK, four, n):
    """24 spots, S = 200 (one task, a ragged run of lanes): nb over 0, 3, 4, 5; all hidden, one observer, nothing hidden, a shown folded
    hand; range_of mixes the four rows (dense, ~40 holdings, one holding, all zero) with 0xFFFF; ids that are not the identity."""
    rng = np.random.default_rng(3000 + n)
    holes, board, nboard, live = WS.random_spots(rng, n, 24)
    ro = mixed_rows(rng, 24, n)
    ids = rng.integers(0, 2 ** 32, 24, dtype=np.uint64).astype(np.uint32)
    assert sorted(set(nboard.tolist())) == [0, 3, 4, 5]
    got = device_ranged(holes, board, nboard, live, 200, four, ro, nonce=n, ids=ids)
    assert not got["status"].any()
    want = spec(holes, board, nboard, live, 200, four, ro, nonce=n, ids=ids)
    print("n = %d: accepted" % n, want["accepted"].tolist())
    assert (want["accepted"] == 200).any() and (want["accepted"] == 0).any() and ((want["accepted"] > 0) & (want["accepted"] < 200)).any()
    assert_equal(got, want, "random n=%d" % n)


def test_many_tasks_per_spot_equal_the_spec(PK, four):
    """2 spots x S = 1 573: four chunks at the minimum of 8 attempts per lane, the last one partial."""
    from pokerl_amd.cards import card_value as cv
    holes = np.array([[[cv("AS"), cv("AD")], [U & 0xFF] * 2, [U & 0xFF] * 2], [[U & 0xFF] * 2, [cv("9C"), cv("8C")], [U & 0xFF] * 2]], np.uint8)
    board = np.array([[cv("KS"), cv("7D"), cv("7C"), cv("2H"), 0], [cv("TC"), cv("JC"), cv("2D"), 0, 0]], np.uint8)
    nboard, live = np.array([4, 3], np.uint8), np.array([7, 7], np.uint16)
    ro = np.array([[U, 0, 1], [0, U, U]], np.uint16)
    got = device_ranged(holes, board, nboard, live, 1573, four, ro, nonce=9)
    assert_equal(got, spec(holes, board, nboard, live, 1573, four, ro, nonce=9), "S = 1 573")
    assert (got["accepted"] > 0).all() and (got["accepted"] < 1573).all()


@pytest.mark.parametrize("hidden", [1, 2, 3, 15, 16])
def test_word_count_edges(PK, hidden):
    """H hidden seats pre-flop at S = 128: H + 1 64-bit words (odd and even counts), 1 .. 9 Philox blocks.  Disjoint three-holding rows, so
    that sixteen drawn holdings do not collide; one seat uniform where there is room."""
    n = max(hidden, 2)
    w = disjoint_rows()
    holes = np.full((2, n, 2), 0xFF, np.uint8)
    if hidden < n:
        holes[:, 0] = [ES.CANON[50], ES.CANON[51]]
    ro = np.array([np.arange(n), np.arange(n)[::-1]], np.uint16)
    if hidden <= 3:
        ro[1, n - 1] = U
    board, nboard, live = np.zeros((2, 5), np.uint8), np.zeros(2, np.uint8), np.full(2, (1 << n) - 1, np.uint16)
    got = device_ranged(holes, board, nboard, live, 128, w, ro, nonce=hidden)
    want = spec(holes, board, nboard, live, 128, w, ro, nonce=hidden)
    assert want["accepted"][0] == 128 and not want["status"].any()
    assert_equal(got, want, "H = %d" % hidden)


def test_range_count_edges(PK, four):
    """R = 0 with range_of NULL (no cumulative row in LDS), R = 1, and R = 16 with every row used at sixteen seats."""
    rng = np.random.default_rng(16)
    holes, board, nboard, live = WS.random_spots(rng, 6, 8)
    assert_equal(device_ranged(holes, board, nboard, live, 100), spec(holes, board, nboard, live, 100), "R = 0")
    one = four[1]
    ro = np.zeros((8, 6), np.uint16)
    got = device_ranged(holes, board, nboard, live, 100, one, nonce=1)                   # one vector: every hidden seat draws from it
    assert_equal(got, spec(holes, board, nboard, live, 100, one, ro, nonce=1), "R = 1")
    w = disjoint_rows(rng)
    h16 = np.full((3, 16, 2), 0xFF, np.uint8)
    b16 = np.array([[ES.CANON[48], ES.CANON[49], ES.CANON[50], ES.CANON[51], 0]] * 3, np.uint8)
    nb16, lv16 = np.array([0, 3, 4], np.uint8), np.full(3, 0xFFFF, np.uint16)
    ro16 = np.array([np.arange(16), np.arange(16)[::-1], (np.arange(16) * 5) % 16], np.uint16)
    got = device_ranged(h16, b16, nb16, lv16, 100, w, ro16, nonce=2)
    want = spec(h16, b16, nb16, lv16, 100, w, ro16, nonce=2)
    assert (want["accepted"] == 100).all()
    assert_equal(got, want, "R = 16")


def test_counts_do_not_depend_on_the_batch_and_nonces_add(PK, four):
    rng = np.random.default_rng(300)
    m = 120
    holes, board, nboard, live = WS.random_spots(rng, 6, m)
    ro = mixed_rows(rng, m, 6)
    ids = (np.arange(m, dtype=np.uint32) * np.uint32(2654435761)).astype(np.uint32)
    batch = device_ranged(holes, board, nboard, live, 130, four, ro, ids=ids)
    for k in (0, 7, 60, m - 1):
        alone = device_ranged(holes[k:k + 1], board[k:k + 1], nboard[k:k + 1], live[k:k + 1], 130, four, ro[k:k + 1], ids=ids[k:k + 1])
        assert_equal(alone, {key: batch[key][k:k + 1] for key in KEYS}, "spot %d alone" % k)
    k = 5                                                         # ids = None is the spot index
    plain = device_ranged(holes[:8], board[:8], nboard[:8], live[:8], 130, four, ro[:8])
    alone = device_ranged(holes[k:k + 1], board[k:k + 1], nboard[k:k + 1], live[k:k + 1], 130, four, ro[k:k + 1], ids=np.array([k], np.uint32))
    assert_equal(alone, {key: plain[key][k:k + 1] for key in KEYS}, "ids = None")
    assert_equal(alone, spec(holes[k:k + 1], board[k:k + 1], nboard[k:k + 1], live[k:k + 1], 130, four, ro[k:k + 1], ids=[k]), "ids = [5] v spec")
    s = slice(0, 12)
    a, b = (device_ranged(holes[s], board[s], nboard[s], live[s], 256, four, ro[s], nonce=x) for x in (3, 4))
    wa, wb = (spec(holes[s], board[s], nboard[s], live[s], 256, four, ro[s], nonce=x) for x in (3, 4))
    assert_equal(a, wa, "nonce 3")
    assert_equal(b, wb, "nonce 4")
    assert (a["win"] != b["win"]).any()
    total = {k: a[k].astype(np.uint64) + b[k] for k in KEYS}
    invariants(total)
    assert_equal(total, {k: wa[k].astype(np.uint64) + wb[k] for k in KEYS}, "the sums")


def test_back_to_back_calls_are_each_correct(PK, four):
    """Eight back-to-back calls of a 64-spot batch reuse one work space, with the size class changing in between."""
    rng = np.random.default_rng(256)
    holes, board, nboard, live = WS.random_spots(rng, 2, 64)
    ro = mixed_rows(rng, 64, 2)
    want = spec(holes, board, nboard, live, 48, four, ro)
    plain = spec(holes, board, nboard, live, 48)
    for rep in range(8):
        if rep % 2:
            assert_equal(device_ranged(holes, board, nboard, live, 48), plain, "call %d (R = 0)" % rep)
        else:
            assert_equal(device_ranged(holes, board, nboard, live, 48, four, ro), want, "call %d" % rep)


def test_device_form_on_a_callers_stream(PK, four):
    from pokerl_amd import hipmem
    from pokerl_amd import judger as J
    rng = np.random.default_rng(77)
    n, m, s = 6, 100, 96
    holes, board, nboard, live = WS.random_spots(rng, n, m)
    ro = mixed_rows(rng, m, n)
    ids = rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32)
    want = device_ranged(holes, board, nboard, live, s, four, ro, nonce=6, ids=ids)
    assert_equal({k: want[k][:24] for k in KEYS}, spec(holes[:24], board[:24], nboard[:24], live[:24], s, four, ro[:24], nonce=6, ids=ids[:24]), "host form")
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0             # hipStreamNonBlocking: a caller's own stream
    ins = [hipmem.DeviceBuffer(x.nbytes).upload(x) for x in (holes, board, nboard, live, ids, four, ro)]
    outs = [hipmem.DeviceBuffer(m * n * 4), hipmem.DeviceBuffer(m * n * 4), hipmem.DeviceBuffer(m * n * 8), hipmem.DeviceBuffer(m * 4), hipmem.DeviceBuffer(m)]

    def call(o, weights_d=ins[5].ptr, r=4, ro_d=ins[6].ptr):
        J.ranged_equity_d(n, m, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, s, weights_d, r, ro_d, ids_d=ins[4].ptr, seed=SEED, nonce=6,
                          win_d=o[0], tie_d=o[1], share_d=o[2], accepted_d=o[3], status_d=o[4], stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0

    for rep in range(2):
        outs[0].upload(np.full(m * n, 7, np.uint32))                          # (the call zeroes its outputs itself)
        outs[3].upload(np.full(m, 7, np.uint32))
        call([x.ptr for x in outs])
        d = dict(win=outs[0].download(np.uint32, m * n).reshape(m, n), tie=outs[1].download(np.uint32, m * n).reshape(m, n),
                 share=outs[2].download(np.uint64, m * n).reshape(m, n), accepted=outs[3].download(np.uint32, m), status=outs[4].download(np.uint8, m))
        assert_equal(d, want, "device form, pass %d" % rep)
    outs[1].upload(np.full(m * n, 9, np.uint32))
    call([None, None, outs[2].ptr, None, outs[4].ptr])                        # only some outputs wanted
    assert (outs[2].download(np.uint64, m * n).reshape(m, n) == want["share"]).all() and not outs[4].download(np.uint8, m).any()
    assert (outs[1].download(np.uint32, m * n) == 9).all()
    call([x.ptr for x in outs], None, 0, None)                                # no ranges at all
    assert (outs[0].download(np.uint32, m * n).reshape(m, n) == device_ranged(holes, board, nboard, live, s, nonce=6, ids=ids)["win"]).all()
    assert hip.hipStreamDestroy(stream) == 0
    for x in ins + outs:
        x.free()


def test_bad_spots_inside_a_batch(PK, four):
    rng = np.random.default_rng(9)
    n = 6
    holes, board, nboard, live = ES.random_spots(rng, n, 24, unknown=False)
    holes[:, 1:] = 0xFF                                                       # seat 0 shown, the others hidden where they are live
    live |= 0b111                                                             # seats 0, 1 and 2 live everywhere
    ro = mixed_rows(rng, 24, n)
    ro[:, 1] = 0
    clean = device_ranged(holes, board, nboard, live, 100, four, ro)
    assert not clean["status"].any()
    h, b, nb, lv, r = holes.copy(), board.copy(), nboard.copy(), live.copy(), ro.copy()
    want = {}
    h[3, 1, 0] = [c for c in ES.CANON if c not in set(h[3, 0].tolist()) | set(b[3].tolist())][0]; want[3] = ES.BAD_CARD   # a half-hidden live seat
    r[7, 1] = 4; want[7] = ES.BAD_CARD                                       # a row that does not exist, at a hidden seat
    r[9, 0] = 4                                                              # ... at a shown seat: ignored
    nb[11] = 5; h[11, 0, 0] = b[11, 4]; want[11] = ES.DUP_CARD               # a card twice
    nb[15] = 6; want[15] = ES.BAD_NBOARD
    lv[19] = 0; want[19] = ES.NO_LIVE
    r[21, 2] = 0xFFFE; want[21] = ES.BAD_CARD
    got = device_ranged(h, b, nb, lv, 100, four, r)
    assert_equal(got, spec(h, b, nb, lv, 100, four, r), "bad spots v spec")
    for i in range(24):
        if i in want:
            assert got["status"][i] & want[i] and not got["win"][i].any() and not got["share"][i].any() and got["accepted"][i] == 0, i
        else:
            assert_equal({k: got[k][i:i + 1] for k in KEYS}, {k: clean[k][i:i + 1] for k in KEYS}, "neighbour %d" % i)


def table_want(g, observer, samples, nonce, weights, range_of, tables=None):
    holes, board, nboard, live = WS.table_spots(g.deck, g.player_states, g.turn, g.active_player, observer)
    t = np.arange(g.num_tables) if tables is None else np.asarray(tables)
    ids = (g.table_id_base + t) % 2 ** 32
    ro = np.asarray(range_of)
    return WS.batch_equity(holes[t], board[t], nboard[t], live[t], samples, weights, ro, per_spot=ro.ndim == 2, nonce=nonce, ids=ids,
                           key=WS.R.seed_key(g.seed))


def played(PK, tables, n, **config):
    g = PK.VecGame(tables, num_players=n, **config)
    g.reset()
    g.rollout(40, policy=0, auto_reset=True, fused=True)
    return g


@pytest.mark.parametrize("observer", [WS.OBSERVER_ACTIVE, 0])
@pytest.mark.parametrize("tables,n,base", [(300, 6, 0), (64, 2, 0), (128, 9, 2 ** 32 - 50)])
def test_table_form_equals_the_spec_fed_from_the_getters(PK, four, tables, n, base, observer):
    g = played(PK, tables, n, seed=4242 + n, table_id_base=base)
    rng = np.random.default_rng(n)
    before = g.save()
    shared = np.array([0, 1, U, 0, 3, 2, 1, 0, U][:n], np.uint16)
    r = as_dict(g.equity_ranged(observer=observer, ranges=four, range_of=shared, samples=64, nonce=11))
    assert not r["status"].any()
    assert_equal(r, table_want(g, observer, 64, 11, four, shared), "table form %dx%d observer %d, range_of by seat" % (tables, n, observer))
    per = rng.choice(np.array([0, 1, U], np.uint16), (tables, n))
    rp = as_dict(g.equity_ranged(observer=observer, ranges=four, range_of=per, samples=64, nonce=11))
    assert_equal(rp, table_want(g, observer, 64, 11, four, per), "range_of per table")
    if observer == WS.OBSERVER_ACTIVE:
        assert_equal(as_dict(g.equity_ranged(ranges=four, range_of=shared, samples=64, nonce=11)), r, "the default observer")
    pick = np.array([5, 5, tables - 1, 0, 17, 5], np.int32)                   # an index array, repeats included: range_of per SPOT
    got = as_dict(g.equity_ranged(pick, observer=observer, ranges=four, range_of=per[pick], samples=64, nonce=11))
    assert_equal(got, {k: rp[k][pick] for k in KEYS}, "index array")
    assert g.save().tobytes() == before.tobytes()                            # the calls wrote nothing to the handle
    g.close()


def test_a_shard_reproduces_its_slice_of_the_whole(PK, four):
    from pokerl_amd import hipmem
    base, a, b = 2 ** 32 - 50, 30, 94                                        # the ids wrap inside the slice
    g = played(PK, 128, 9, seed=99, table_id_base=base)
    shared = np.array([0, 1, U, 0, 1, U, 0, 1, U], np.uint16)
    whole = as_dict(g.equity_ranged(ranges=four, range_of=shared, samples=64, nonce=5))
    part = PK.VecGame(b - a, num_players=9, seed=99, table_id_base=(base + a) % 2 ** 32)
    part.load(g.save(np.arange(a, b)))
    assert_equal(as_dict(part.equity_ranged(ranges=four, range_of=shared, samples=64, nonce=5)), {k: whole[k][a:b] for k in KEYS}, "tables [30, 94)")
    n, m = 9, b - a                                                           # ... and the device form of the table call, NULL outputs included
    wd, rd = hipmem.DeviceBuffer(four.nbytes).upload(four), hipmem.DeviceBuffer(shared.nbytes).upload(shared)
    outs = [hipmem.DeviceBuffer(m * n * 4), hipmem.DeviceBuffer(m * n * 8), hipmem.DeviceBuffer(m * 4)]
    part.equity_ranged_d(weights_d=wd, num_ranges=4, range_of_d=rd, samples=64, nonce=5, win_d=outs[0], share_d=outs[1], accepted_d=outs[2])
    part.sync()
    assert (outs[0].download(np.uint32, m * n).reshape(m, n) == whole["win"][a:b]).all()
    assert (outs[1].download(np.uint64, m * n).reshape(m, n) == whole["share"][a:b]).all()
    assert (outs[2].download(np.uint32, m) == whole["accepted"][a:b]).all()
    for x in outs + [wd, rd]:
        x.free()
    part.close()
    g.close()


def test_bad_indices_never_dealt_tables_and_the_single_game(PK, four):
    from pokerl_amd import _lib as L
    g = PK.VecGame(64, num_players=6)
    for observer in (WS.OBSERVER_ACTIVE, 2):
        r = g.equity_ranged(observer=observer, ranges=four[0], samples=64)
        assert (r.status == ES.DUP_CARD).all() and not r.win.any() and not r.accepted.any()
    g.reset()
    r = g.equity_ranged(np.array([0, 64, -1, 5, 2 ** 31 - 1, 5], np.int64), ranges=four[0], samples=64)
    assert r.status.tolist() == [0, ES.BAD_TABLE, ES.BAD_TABLE, 0, ES.BAD_TABLE, 0]
    assert not r.win[[1, 2, 4]].any() and not r.accepted[[1, 2, 4]].any() and (r.win[3] == r.win[5]).all() and r.accepted[3] == r.accepted[5] > 0
    p = L.ptr(four)
    for observer in (6, 16, -3, L.OBSERVER_NONE):
        rc = g._lib.pk_table_equity_ranged(g._h, None, 4, observer, 64, 0, p, 4, None, 0, None, None, None, None, None)
        assert rc == L.PK_E_INVALID_ARG and b"pk_table_equity_ranged" in g._lib.pk_last_error(g._h)
    assert g._lib.pk_table_equity_ranged_d(g._h, None, 4, 0, 0, 0, None, 0, None, 0, None, None, None, None, None) == L.PK_E_INVALID_ARG
    assert g._lib.pk_table_equity_ranged_d(g._h, None, 4, 0, 64, 0, p, 17, None, 0, None, None, None, None, None) == L.PK_E_INVALID_ARG
    assert g._lib.pk_table_equity_ranged_d(g._h, None, 0, 0, 64, 0, None, 0, None, 0, None, None, None, None, None) == L.PK_OK      # m == 0: a no-op
    with pytest.raises(ValueError):
        g.equity_ranged(observer=None, ranges=four[0])
    g.close()
    single = PK.Game(num_players=3)
    with pytest.raises(ValueError):
        single.equity_ranged(ranges=four[0])
    single.reset()
    e = single.equity_ranged(ranges=four, range_of=[0, 1, U], samples=256)
    assert e.win.shape == e.tie.shape == e.share.shape == e.equity.shape == (3,) and e.status == 0 and 0 < e.accepted <= 256
    assert e.acceptance == e.accepted / 256
    want = table_want(single._v, WS.OBSERVER_ACTIVE, 256, 0, four, np.array([0, 1, U], np.uint16))
    assert_equal({k: np.asarray(getattr(e, k))[None] for k in KEYS}, want, "Game.equity_ranged")
    single.close()


def test_tables_in_flight_report_it_and_the_others_are_still_correct(PK, four):
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
    shared = np.array([U, 0, 1], np.uint16)
    r = as_dict(g.equity_ranged(observer=0, ranges=four, range_of=shared, samples=32, nonce=2))
    assert (r["status"][~idle] == ES.IN_FLIGHT).all() and not r["win"][~idle].any() and not r["status"][idle].any()
    act.upload(np.full(T, -1, np.int32))                                     # the drain: idle tables get no step and stay as they are
    g.step_async_d(act, flags, terr, ready, max_hands=0, auto_reset=True)
    g.sync()
    t = np.flatnonzero(idle)
    assert_equal({k: r[k][t] for k in KEYS}, table_want(g, 0, 32, 2, four, shared, t), "the idle tables")
    for b in (act, flags, terr, ready):
        b.free()
    g.close()


def test_one_holding_ranges_on_the_river_need_no_spec(PK):
    """Three seats on the river, the two hidden ones each with a one-holding range: every attempt is accepted and ends the same way, so
    win = S * indicator, judged by pk_equity on the shown hands."""
    from pokerl_amd import judger as J
    rng = np.random.default_rng(5)
    holes, board, nboard, live = ES.random_spots(rng, 3, 8, nb=5, unknown=False)
    live[:] = 7
    exact = J.showdown_equity_batch(holes, board, nboard, live)
    s = 333
    for i in range(8):
        w = np.zeros((2, WS.HOLDINGS), np.uint16)
        w[0, WS.holding_index(*holes[i, 1])] = 3
        w[1, WS.holding_index(*holes[i, 2])] = 65535
        hid = holes[i:i + 1].copy()
        hid[0, 1:] = 0xFF
        got = device_ranged(hid, board[i:i + 1], nboard[i:i + 1], live[i:i + 1], s, w, np.array([[U, 0, 1]], np.uint16), nonce=i)
        assert got["accepted"][0] == s and got["status"][0] == 0
        for k in COUNTS:
            assert (got[k][0].astype(np.uint64) == s * getattr(exact, k)[i].astype(np.uint64)).all(), (i, k)


def five_sigma(count, accepted, p, where):
    dev = np.abs(count / accepted - p)
    bound = 5 * np.sqrt(p * (1 - p) / accepted)
    print(where, "exact", np.asarray(p).tolist(), "sampled", np.asarray(count / accepted).tolist(), "deviation", np.asarray(dev).tolist(), "bound",
          np.asarray(bound).tolist(), "accepted", int(accepted))
    assert (dev <= bound).all(), (where, np.asarray(dev).tolist(), np.asarray(bound).tolist())


def test_converges_to_the_exact_values(PK):
    """S = 2^20: the fixed turn spot under a fixed range against pk_equity_range's aggregates, and a three-seat river spot with two sparse
    ranges against a host enumeration of the pairs of holdings; |count / accepted - p| <= 5 sqrt(p (1 - p) / accepted), the binomial
    standard deviation over the accepted attempts.  Seeds fixed; the deviations are printed before the assertion."""
    from pokerl_amd import judger as J
    from pokerl_amd.cards import card_value as cv
    s = 1 << 20
    hero, board = [cv("AS"), cv("AD")], [cv("KS"), cv("7D"), cv("7C"), cv("2H")]
    rng = np.random.default_rng(2024)
    w = (rng.integers(0, 50, WS.HOLDINGS) * (rng.random(WS.HOLDINGS) < 0.4)).astype(np.uint16)
    exact = J.range_equity(hero, board, weights=w)
    agg = np.asarray(exact.agg, np.float64)
    got = J.ranged_equity([hero, None], board, ranges=w, samples=s, seed=SEED, nonce=1)
    assert got.status == 0 and 0 < got.accepted < s
    five_sigma(np.array([got.win[0], got.tie[0]], np.float64), float(got.accepted), agg[:2] / agg[2], "turn spot under a range:")
    # three seats on the river: seat 0 shown, seats 1 and 2 with sparse ranges of <= 40 holdings
    holes, b5, nb5, lv5 = ES.random_spots(rng, 3, 1, nb=5, unknown=False)
    dead = set(holes[0, 0].tolist()) | set(b5[0].tolist())
    w2 = np.zeros((2, WS.HOLDINGS), np.uint16)
    for r in range(2):
        w2[r, rng.choice(WS.HOLDINGS, 40, replace=False)] = rng.integers(1, 100, 40)
    pairs, weights = [], []
    for h1 in np.flatnonzero(w2[0]):
        for h2 in np.flatnonzero(w2[1]):
            c = [ES.CANON[WS.PAIR_A[h1]], ES.CANON[WS.PAIR_B[h1]], ES.CANON[WS.PAIR_A[h2]], ES.CANON[WS.PAIR_B[h2]]]
            if len(set(c)) == 4 and not set(c) & dead:
                pairs.append([holes[0, 0].tolist(), c[:2], c[2:]])
                weights.append(int(w2[0, h1]) * int(w2[1, h2]))
    assert 0 < len(pairs) <= 1600
    pairs, weights = np.array(pairs, np.uint8), np.array(weights, np.float64)
    e = J.showdown_equity_batch(pairs, np.tile(b5, (len(pairs), 1)), np.full(len(pairs), 5, np.uint8), np.full(len(pairs), 7, np.uint16))
    assert (e.boards == 1).all()
    p_win = (weights[:, None] * e.win).sum(axis=0) / weights.sum()
    p_tie = (weights[:, None] * e.tie).sum(axis=0) / weights.sum()
    hid = holes.copy()
    hid[0, 1:] = 0xFF
    g3 = device_ranged(hid, b5, nb5, np.array([7], np.uint16), s, w2, np.array([[U, 0, 1]], np.uint16), nonce=1)
    acc = float(g3["accepted"][0])
    five_sigma(g3["win"][0].astype(np.float64), acc, p_win, "three seats on the river, win:")
    five_sigma(g3["tie"][0].astype(np.float64), acc, p_tie, "three seats on the river, tie:")
