"""GPU tests of the sampled showdown equity through the C ABI (pk_equity_sampled(_d), pk_table_equity_sampled(_d)): exact equality with
the Python restatement of the definition (tests/equity_sampled_spec.py) -- hidden masks, sample counts around a wavefront, many tasks per
spot, one to three Philox blocks, ids, nonces, the table form as each kind of observer sees it -- and convergence to pk_equity's exact
values within five derived standard deviations."""
import ctypes as C

import numpy as np
import pytest

import equity_sampled_spec as SS
import equity_spec as ES

pytestmark = pytest.mark.gpu
KEYS = SS.KEYS
COUNTS = ("win", "tie", "share")
SEED = 0x5EED0123456789AB


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


def as_dict(r):
    out = {k: np.asarray(getattr(r, k)) for k in KEYS}
    invariants(out)
    return out


def device_sampled(holes, board, nboard, live, samples, seed=SEED, nonce=0, ids=None):
    from pokerl_amd import judger as J
    return as_dict(J.sampled_equity_batch(holes, board, nboard, live, samples, seed, nonce, ids))


def invariants(out):
    """On every spot of every test: the shares add up to the samples exactly, win + tie <= samples, a refused spot is all zero."""
    share = out["share"].astype(object).sum(axis=-1)
    ok = out["status"] == 0
    assert (share == ES.SHARE_UNIT * out["samples"].astype(object)).all()
    assert ((out["win"].astype(np.int64) + out["tie"]) <= out["samples"].astype(np.int64)[..., None]).all()
    assert not out["samples"][~ok].any() and (out["samples"][ok] > 0).all()


def assert_equal(got, want, where, keys=KEYS):
    for k in keys:
        a, b = np.asarray(got[k]).astype(np.uint64), np.asarray(want[k]).astype(np.uint64)
        assert a.shape == b.shape and (a == b).all(), (where, k, np.argwhere(a != b)[:4].tolist())


@pytest.mark.parametrize("n", [2, 3, 6, 9, 16])
def test_random_spots_equal_the_spec(PK, n):
    """18 spots, every nb 0 .. 5 three times, hidden masks of every kind (none, all, one byte, random), ids that are not the identity;
    S = 1, 63, 65 (below / above one wavefront), 1 000 (no multiple of 64, several samples per lane)."""
    rng = np.random.default_rng(2000 + n)
    holes, board, nboard, live = SS.random_spots(rng, n, 18)      # (the hidden-mask kind is the position mod 4 ...
    nboard[:] = np.arange(18) % 6                                 # ... the board count the position mod 6: any prefix of the board is valid)
    ids = rng.integers(0, 2 ** 32, len(nboard), dtype=np.uint64).astype(np.uint32)
    kinds = {(h[(int(lv) >> np.arange(n)) & 1 == 1] == ES.UNKNOWN).mean() for h, lv in zip(holes, live)}
    assert 0.0 in kinds and 1.0 in kinds and sorted(set(nboard.tolist())) == list(range(6))
    for s in (1, 63, 65, 1000):
        got = device_sampled(holes, board, nboard, live, s, nonce=s, ids=ids)
        assert not got["status"].any() and (got["samples"] == s).all()
        assert_equal(got, SS.batch_equity(holes, board, nboard, live, s, SEED, s, ids), "random n=%d S=%d" % (n, s))


def test_many_tasks_per_spot_equal_the_spec(PK):
    """m = 2, S = 70 000: each spot is cut into many tasks whose counts are added up in the outputs.  The whole count, the first 300
    samples (S = 300 is a prefix of the same stream) and the last 300 (the difference to S = 69 700) against the spec."""
    from pokerl_amd.cards import card_value as cv
    holes = np.array([[[cv("AS"), cv("AD")], [ES.UNKNOWN, ES.UNKNOWN]], [[cv("9H"), ES.UNKNOWN], [cv("9C"), cv("8C")]]], np.uint8)
    board = np.array([[cv("KS"), cv("7D"), cv("7C"), cv("2H"), 0], [cv("TC"), cv("JC"), cv("2D"), cv("3S"), 0]], np.uint8)
    nboard, live, s = np.array([4, 4], np.uint8), np.array([3, 3], np.uint16), 70000
    key = SS.R.seed_key(SEED)
    hands = [SS.sample_cards(holes[i], [int(x) for x in board[i]], 4, 3, key, i, 9, s)[0] for i in range(2)]

    def spec(first, last):
        return {k: np.stack([SS.count(h, 3, first, last)[k] for h in hands]) for k in COUNTS}

    whole = device_sampled(holes, board, nboard, live, s, nonce=9)
    assert_equal(whole, spec(0, s), "S = 70 000", COUNTS)
    assert_equal(device_sampled(holes, board, nboard, live, 300, nonce=9), spec(0, 300), "the first 300", COUNTS)
    head = device_sampled(holes, board, nboard, live, s - 300, nonce=9)
    assert_equal({k: whole[k].astype(np.int64) - head[k].astype(np.int64) for k in COUNTS}, spec(s - 300, s), "the last 300", COUNTS)


def test_draw_count_edges(PK):
    """D = 37 (N = 16, all live, all hidden, pre-flop): three Philox blocks, the draws cross words at 9, 18, 27, 36.  D = 18 (N = 9, flop,
    eight hidden hands): exactly one block."""
    rng = np.random.default_rng(37)
    holes = np.full((2, 16, 2), ES.UNKNOWN, np.uint8)
    board = np.zeros((2, 5), np.uint8)
    got = device_sampled(holes, board, np.zeros(2, np.uint8), np.full(2, 0xFFFF, np.uint16), 200, nonce=1)
    assert_equal(got, SS.batch_equity(holes, board, np.zeros(2, np.uint8), np.full(2, 0xFFFF, np.uint16), 200, SEED, 1), "D = 37")
    h9, b9, nb9, lv9 = ES.random_spots(rng, 9, 3, nb=3, unknown=False)
    lv9[:] = 0x1FF
    h9[:, 1:] = ES.UNKNOWN
    assert len(SS.check_spot(h9[0], b9[0], 3, 0x1FF)[3]) + 2 == 18
    assert_equal(device_sampled(h9, b9, nb9, lv9, 200, nonce=2), SS.batch_equity(h9, b9, nb9, lv9, 200, SEED, 2), "D = 18")


def test_counts_do_not_depend_on_the_batch(PK):
    rng = np.random.default_rng(300)
    holes, board, nboard, live = SS.random_spots(rng, 6, 300)
    ids = (np.arange(300, dtype=np.uint32) * np.uint32(2654435761)).astype(np.uint32)
    batch = device_sampled(holes, board, nboard, live, 130, ids=ids)
    for k in (0, 7, 150, 299):
        alone = device_sampled(holes[k:k + 1], board[k:k + 1], nboard[k:k + 1], live[k:k + 1], 130, ids=ids[k:k + 1])
        assert_equal(alone, {key: batch[key][k:k + 1] for key in KEYS}, "spot %d alone" % k)
    k = 5                                                         # ids = None is the spot index: spot 5 of a batch = a lone spot with ids = [5]
    plain = device_sampled(holes[:8], board[:8], nboard[:8], live[:8], 130)
    alone = device_sampled(holes[k:k + 1], board[k:k + 1], nboard[k:k + 1], live[k:k + 1], 130, ids=np.array([k], np.uint32))
    assert_equal(alone, {key: plain[key][k:k + 1] for key in KEYS}, "ids = None")
    assert_equal(alone, SS.batch_equity(holes[k:k + 1], board[k:k + 1], nboard[k:k + 1], live[k:k + 1], 130, SEED, 0, [k]), "ids = [5] v spec")


def test_repeatable_and_back_to_back_calls_are_each_correct(PK):
    """The same call twice: equal bytes.  Sixteen back-to-back calls of a 256-spot batch reuse one work space: every one must deliver."""
    rng = np.random.default_rng(256)
    holes, board, nboard, live = SS.random_spots(rng, 2, 256)
    want = SS.batch_equity(holes, board, nboard, live, 48, SEED, 0)
    for rep in range(16):
        got = device_sampled(holes, board, nboard, live, 48)
        assert_equal(got, want, "call %d" % rep)
        assert all(got[k].tobytes() == np.asarray(want[k], got[k].dtype).tobytes() for k in KEYS)


def test_counts_of_different_nonces_add(PK):
    rng = np.random.default_rng(34)
    holes, board, nboard, live = SS.random_spots(rng, 6, 12)
    a, b = (device_sampled(holes, board, nboard, live, 512, nonce=x) for x in (3, 4))
    wa, wb = (SS.batch_equity(holes, board, nboard, live, 512, SEED, x) for x in (3, 4))
    assert_equal(a, wa, "nonce 3")
    assert_equal(b, wb, "nonce 4")
    hidden = np.array([(h == ES.UNKNOWN).any() or nb < 5 for h, nb in zip(holes, nboard)])
    assert (a["win"][hidden] != b["win"][hidden]).any()           # two streams, not one
    total = {k: a[k].astype(np.uint64) + b[k] for k in KEYS}
    invariants(total)                                             # 1 024 samples: the shares still add up to them exactly
    assert_equal(total, {k: wa[k].astype(np.uint64) + wb[k] for k in KEYS}, "the sums")
    other = device_sampled(holes, board, nboard, live, 512, seed=SEED + 1, nonce=3)
    assert (other["win"][hidden] != a["win"][hidden]).any()       # the seed is the key


def test_device_form_on_a_callers_stream(PK):
    from pokerl_amd import hipmem
    from pokerl_amd import judger as J
    rng = np.random.default_rng(77)
    n, m, s = 6, 200, 96
    holes, board, nboard, live = SS.random_spots(rng, n, m)
    ids = rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32)
    want = device_sampled(holes, board, nboard, live, s, nonce=6, ids=ids)
    assert_equal({k: want[k][:24] for k in KEYS}, SS.batch_equity(holes[:24], board[:24], nboard[:24], live[:24], s, SEED, 6, ids[:24]), "host form")
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0             # hipStreamNonBlocking: a caller's own stream
    ins = [hipmem.DeviceBuffer(x.nbytes).upload(x) for x in (holes, board, nboard, live, ids)]
    outs = [hipmem.DeviceBuffer(m * n * 4), hipmem.DeviceBuffer(m * n * 4), hipmem.DeviceBuffer(m * n * 8), hipmem.DeviceBuffer(m * 4), hipmem.DeviceBuffer(m)]

    def call(ids_d, o):
        J.sampled_equity_d(n, m, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, s, ids_d=ids_d, seed=SEED, nonce=6, win_d=o[0], tie_d=o[1],
                           share_d=o[2], samples_d=o[3], status_d=o[4], stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0

    for rep in range(2):
        outs[0].upload(np.full(m * n, 7, np.uint32))                          # (the call zeroes its outputs itself)
        call(ins[4].ptr, [x.ptr for x in outs])
        d = dict(win=outs[0].download(np.uint32, m * n).reshape(m, n), tie=outs[1].download(np.uint32, m * n).reshape(m, n),
                 share=outs[2].download(np.uint64, m * n).reshape(m, n), samples=outs[3].download(np.uint32, m), status=outs[4].download(np.uint8, m))
        assert_equal(d, want, "device form, pass %d" % rep)
    outs[1].upload(np.full(m * n, 9, np.uint32))
    call(ins[4].ptr, [None, None, outs[2].ptr, None, outs[4].ptr])            # only some outputs wanted
    assert (outs[2].download(np.uint64, m * n).reshape(m, n) == want["share"]).all() and not outs[4].download(np.uint8, m).any()
    assert (outs[1].download(np.uint32, m * n) == 9).all()
    call(None, [x.ptr for x in outs])                                         # ids NULL: the spot index
    assert (outs[0].download(np.uint32, m * n).reshape(m, n) == device_sampled(holes, board, nboard, live, s, nonce=6)["win"]).all()
    assert hip.hipStreamDestroy(stream) == 0
    for x in ins + outs:
        x.free()


def test_bad_spots_inside_a_batch(PK):
    rng = np.random.default_rng(9)
    n = 6
    holes, board, nboard, live = SS.random_spots(rng, n, 24)
    clean = device_sampled(holes, board, nboard, live, 100)
    assert not clean["status"].any()
    h, b, nb, lv = holes.copy(), board.copy(), nboard.copy(), live.copy()
    want = {}
    h[3, 0, 0] = 0x4F; want[3] = ES.BAD_CARD                                 # a byte that is no card
    nb[7] = 5; b[7, 2] = ES.UNKNOWN; want[7] = ES.BAD_CARD                   # 0xFF in the board
    nb[11] = 5; h[11, 2] = [b[11, 4], 0x00 if b[11, 4] != 0x00 else 0x01]; lv[11] |= 4; want[11] = ES.DUP_CARD
    lv[15] = 0; want[15] = ES.NO_LIVE
    nb[19] = 6; want[19] = ES.BAD_NBOARD
    lv[21] = 0xFFC0; want[21] = ES.NO_LIVE                                   # only seats >= N: ignored bits
    got = device_sampled(h, b, nb, lv, 100)
    assert_equal(got, SS.batch_equity(h, b, nb, lv, 100, SEED, 0), "bad spots v spec")
    for i in range(24):
        if i in want:
            assert got["status"][i] & want[i] and not got["win"][i].any() and not got["share"][i].any() and got["samples"][i] == 0, i
        else:
            assert_equal({k: got[k][i:i + 1] for k in KEYS}, {k: clean[k][i:i + 1] for k in KEYS}, "neighbour %d" % i)


def table_want(PK, g, observer, samples, nonce, tables=None):
    holes, board, nboard, live = SS.table_spots(g.deck, g.player_states, g.turn, g.active_player, observer)
    t = np.arange(g.num_tables) if tables is None else np.asarray(tables)
    ids = (g.table_id_base + t) % 2 ** 32
    return SS.batch_equity(holes[t], board[t], nboard[t], live[t], samples, nonce=nonce, ids=ids, key=SS.R.seed_key(g.seed))


def played(PK, tables, n, **config):
    g = PK.VecGame(tables, num_players=n, **config)
    g.reset()
    g.rollout(40, policy=0, auto_reset=True, fused=True)
    return g


@pytest.mark.parametrize("observer", [SS.OBSERVER_ACTIVE, 0, SS.OBSERVER_NONE])
@pytest.mark.parametrize("tables,n,base", [(300, 6, 0), (64, 2, 0), (128, 9, 2 ** 32 - 50)])
def test_table_form_equals_the_spec_fed_from_the_getters(PK, tables, n, base, observer):
    g = played(PK, tables, n, seed=4242 + n, table_id_base=base)
    before = g.save()
    r = as_dict(g.equity_sampled(observer=observer, samples=200, nonce=11))
    assert not r["status"].any()
    assert_equal(r, table_want(PK, g, observer, 200, 11), "table form %dx%d observer %d" % (tables, n, observer))
    if observer == SS.OBSERVER_ACTIVE:
        assert_equal(as_dict(g.equity_sampled(samples=200, nonce=11)), r, "the default observer")
        assert_equal(as_dict(g.equity_sampled(observer='active', samples=200, nonce=11)), r, "'active'")
    pick = np.array([5, 5, tables - 1, 0, 17, 5], np.int32)                   # an index array, repeats included
    assert_equal(as_dict(g.equity_sampled(pick, observer=observer, samples=200, nonce=11)), {k: r[k][pick] for k in KEYS}, "index array")
    assert g.save().tobytes() == before.tobytes()                            # the calls wrote nothing to the handle
    g.close()


def test_a_shard_reproduces_its_slice_of_the_whole(PK):
    from pokerl_amd import hipmem
    base, a, b = 2 ** 32 - 50, 30, 94                                        # the ids wrap inside the slice
    g = played(PK, 128, 9, seed=99, table_id_base=base)
    whole = as_dict(g.equity_sampled(samples=200, nonce=5))
    part = PK.VecGame(b - a, num_players=9, seed=99, table_id_base=(base + a) % 2 ** 32)
    part.load(g.save(np.arange(a, b)))
    assert_equal(as_dict(part.equity_sampled(samples=200, nonce=5)), {k: whole[k][a:b] for k in KEYS}, "tables [30, 94) in a handle of their own")
    # ... and the device form of the table call, NULL outputs included
    n, m = 9, b - a
    outs = [hipmem.DeviceBuffer(m * n * 4), hipmem.DeviceBuffer(m * n * 8), hipmem.DeviceBuffer(m * 4)]
    part.equity_sampled_d(samples=200, nonce=5, win_d=outs[0], share_d=outs[1], samples_d=outs[2])
    part.sync()
    assert (outs[0].download(np.uint32, m * n).reshape(m, n) == whole["win"][a:b]).all()
    assert (outs[1].download(np.uint64, m * n).reshape(m, n) == whole["share"][a:b]).all() and (outs[2].download(np.uint32, m) == 200).all()
    for x in outs:
        x.free()
    part.close()
    g.close()


def test_bad_indices_never_dealt_tables_and_the_single_game(PK):
    from pokerl_amd import _lib as L
    g = PK.VecGame(64, num_players=6)
    for observer in (SS.OBSERVER_ACTIVE, 2, SS.OBSERVER_NONE):
        r = g.equity_sampled(observer=observer, samples=64)
        assert (r.status == ES.DUP_CARD).all() and not r.win.any() and not r.samples.any()
    g.reset()
    r = g.equity_sampled(np.array([0, 64, -1, 5, 2 ** 31 - 1, 5], np.int64), samples=64)
    assert r.status.tolist() == [0, ES.BAD_TABLE, ES.BAD_TABLE, 0, ES.BAD_TABLE, 0]
    assert r.samples.tolist() == [64, 0, 0, 64, 0, 64] and not r.win[[1, 2, 4]].any() and (r.win[3] == r.win[5]).all()
    for observer in (6, 16, -3):
        rc = g._lib.pk_table_equity_sampled(g._h, None, 4, observer, 64, 0, None, None, None, None, None)
        assert rc == L.PK_E_INVALID_ARG and b"pk_table_equity_sampled" in g._lib.pk_last_error(g._h)
    assert g._lib.pk_table_equity_sampled_d(g._h, None, 4, 0, 0, 0, None, None, None, None, None) == L.PK_E_INVALID_ARG
    assert g._lib.pk_table_equity_sampled_d(g._h, None, 0, 0, 64, 0, None, None, None, None, None) == L.PK_OK      # m == 0: a no-op
    g.close()
    single = PK.Game(num_players=3)
    with pytest.raises(ValueError):
        single.equity_sampled()
    single.reset()
    e = single.equity_sampled(samples=256)
    assert e.win.shape == e.tie.shape == e.share.shape == e.stderr.shape == (3,) and e.status == 0 and e.samples == 256
    assert int(e.share.astype(object).sum()) == ES.SHARE_UNIT * 256
    want = table_want(PK, single._v, SS.OBSERVER_ACTIVE, 256, 0)
    assert_equal({k: np.asarray(getattr(e, k))[None] for k in KEYS}, want, "Game.equity_sampled")
    e2 = single.equity_sampled(observer=1, samples=256)
    assert_equal({k: np.asarray(getattr(e2, k))[None] for k in KEYS}, table_want(PK, single._v, 1, 256, 0), "Game.equity_sampled(observer=1)")
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
    r = as_dict(g.equity_sampled(observer=0, samples=100, nonce=2))
    assert (r["status"][~idle] == ES.IN_FLIGHT).all() and not r["win"][~idle].any() and not r["status"][idle].any()
    act.upload(np.full(T, -1, np.int32))                                     # the drain: idle tables get no step and stay as they are
    g.step_async_d(act, flags, terr, ready, max_hands=0, auto_reset=True)
    g.sync()
    t = np.flatnonzero(idle)
    assert_equal({k: r[k][t] for k in KEYS}, table_want(PK, g, 0, 100, 2, t), "the idle tables")
    for b in (act, flags, terr, ready):
        b.free()
    g.close()


def test_everything_known_is_the_exact_count_times_samples(PK):
    from pokerl_amd import judger as J
    rng = np.random.default_rng(55)
    for n in (2, 6, 16):
        holes, board, nboard, live = ES.random_spots(rng, n, 10, nb=5)
        exact = J.showdown_equity_batch(holes, board, nboard, live)
        got = device_sampled(holes, board, nboard, live, 777)
        assert (exact.boards == 1).all() and (got["samples"] == 777).all()
        for k in COUNTS:
            assert (got[k].astype(np.uint64) == 777 * getattr(exact, k).astype(np.uint64)).all(), (n, k)


def five_sigma(win, samples, p, where):
    dev = np.abs(win / samples - p)
    bound = 5 * np.sqrt(p * (1 - p) / samples)
    print(where, "exact", p.tolist(), "sampled", (win / samples).tolist(), "deviation", dev.tolist(), "bound", bound.tolist())
    assert (dev <= bound).all(), (where, dev.tolist(), bound.tolist())


def test_converges_to_the_exact_equity(PK):
    """S = 2^20 on the device against pk_equity (not against the spec): |win / S - p| <= 5 sqrt(p (1 - p) / S) per seat, the binomial
    standard deviation of a count of S independent samples; seeds fixed.  The deviations are printed before the assertion."""
    from pokerl_amd import judger as J
    from pokerl_amd.cards import card_value as cv
    s = 1 << 20
    hero, board = [cv("AS"), cv("AD")], [cv("KS"), cv("7D"), cv("7C"), cv("2H")]
    pool = [c for c in ES.CANON if c not in set(hero + board)]
    opp = np.array([[a, b] for i, a in enumerate(pool) for b in pool[i + 1:]], np.uint8)
    assert len(opp) == 1035
    holes = np.stack([np.tile(np.array(hero, np.uint8), (1035, 1)), opp], axis=1)
    exact = J.showdown_equity_batch(holes, np.tile(np.array(board + [0], np.uint8), (1035, 1)), np.full(1035, 4, np.uint8), np.full(1035, 3, np.uint16))
    assert (exact.boards == 44).all() and not exact.status.any()                # equal weights: every opponent hand leaves 44 rivers
    p = exact.win.astype(np.float64).sum(axis=0) / (1035 * 44)
    got = J.sampled_equity([hero, None], board, samples=s, seed=SEED, nonce=1)
    assert got.samples == s
    five_sigma(got.win.astype(np.float64), s, p, "turn spot, opponent hidden:")
    assert np.allclose(got.stderr, np.sqrt(((got.win + got.tie) / s) * (1 - (got.win + got.tie) / s) / s))
    rng = np.random.default_rng(66)
    h6, b6, nb6, lv6 = ES.random_spots(rng, 6, 1, nb=3, unknown=False)
    lv6[:] = 0x3F
    e6 = J.showdown_equity_batch(h6, b6, nb6, lv6)
    g6 = device_sampled(h6, b6, nb6, lv6, s, nonce=1)
    five_sigma(g6["win"][0].astype(np.float64), s, e6.win[0] / float(e6.boards[0]), "six seats on the flop, all known:")
