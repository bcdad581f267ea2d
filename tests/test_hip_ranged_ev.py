"""GPU tests of the ranged showdown EV through the C ABI (pk_ev_ranged(_d), pk_table_ev_ranged(_d)) and the Python helpers: exact equality on
share, level_seat, accepted and status, bit patterns on amount and ev, with the numpy restatement of the definition (tests/ranged_ev_spec.py)
-- hidden patterns, every street, dense / sparse / one-holding / dead ranges, equal bets, ladders, ties, zeros and dead money, one to eight
groups of levels, the three LDS size classes, several chunks, bad spots, the table form, the device forms -- identities that need no spec
(against pk_equity_ranged and pk_equity_ev), and convergence within five derived standard deviations."""
import ctypes as C

import numpy as np
import pytest

import equity_range_spec as RS
import equity_ranged_spec as WS
import equity_spec as ES
import ev_witness as W
import ranged_ev_spec as XS
from equity_seat_matrix import disjoint_rows

pytestmark = pytest.mark.gpu
KEYS = XS.KEYS
SEED = 0x5EED0123456789AB
U = WS.UNIFORM


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def invariants(out):
    """On every spot of every test: a level with amount > 0 pays out 720720 * accepted in all, any other level nothing; a refused spot is all
    zero with level_seat 0xFF."""
    sums = out["share"].astype(object).sum(axis=-1)
    paid = out["amount"] > 0
    acc = out["accepted"].astype(object)[..., None] * ES.SHARE_UNIT
    assert (np.where(paid, sums == acc, sums == 0)).all()
    bad = out["status"] != 0
    assert not out["accepted"][bad].any() and not out["share"][bad].any() and not bits(out["ev"][bad]).any() and not bits(out["amount"][bad]).any()
    assert (out["level_seat"][bad] == XS.NO_LEVEL).all()
    assert not bits(out["ev"][out["accepted"] == 0]).any()


def as_dict(r):
    out = {k: np.asarray(getattr(r, k)) for k in KEYS}
    invariants(out)
    return out


def device_ev(holes, board, nboard, live, bets, samples, weights=None, range_of=None, seed=SEED, nonce=0, ids=None):
    from pokerl_amd import judger as J
    return as_dict(J.ranged_ev_batch(holes, board, nboard, live, bets, weights, range_of, samples, seed, nonce, ids))


def spec(holes, board, nboard, live, bets, samples, weights=None, range_of=None, nonce=0, ids=None):
    per = range_of is not None and np.ndim(range_of) == 2
    return XS.batch_ev(holes, board, nboard, live, bets, samples, weights, range_of, per_spot=per, seed=SEED, nonce=nonce, ids=ids)


def pick(d, s):
    return {k: d[k][s] for k in KEYS}


@pytest.fixture(scope="module")
def four():
    return WS.random_ranges(np.random.default_rng(1))


def mixed_rows(rng, m, n):
    """range_of [m, n]: rows 0 .. 3 and 0xFFFF."""
    return rng.choice(np.array([0, 1, 2, 3, U], np.uint16), (m, n))


def pattern_bets(n, live):
    return np.array([XS.bet_patterns(n, live[i], i) for i in range(len(live))], np.float64)


@pytest.mark.parametrize("n", [2, 3, 6, 9, 16])
def test_random_spots_equal_the_spec(PK, four, n):
    """24 spots, S = 200 (one chunk, a ragged run of lanes): nb over 0, 3, 4, 5; all hidden, one observer, nothing hidden, a shown folded hand;
    range_of mixes the four rows with 0xFFFF; ids that are not the identity; bets cycle through equal, a full ladder, a ladder with ties and
    zeros, and dead money at folded seats."""
    rng = np.random.default_rng(5100 + n)
    holes, board, nboard, live = WS.random_spots(rng, n, 24)
    ro = mixed_rows(rng, 24, n)
    ids = rng.integers(0, 2 ** 32, 24, dtype=np.uint64).astype(np.uint32)
    bets = pattern_bets(n, live)
    assert sorted(set(nboard.tolist())) == [0, 3, 4, 5]
    got = device_ev(holes, board, nboard, live, bets, 200, four, ro, nonce=n, ids=ids)
    assert not got["status"].any()
    want = spec(holes, board, nboard, live, bets, 200, four, ro, nonce=n, ids=ids)
    nlev = (want["level_seat"] != XS.NO_LEVEL).sum(axis=1)
    print("n = %d: accepted" % n, want["accepted"].tolist(), "levels", nlev.tolist())
    assert (want["accepted"] == 200).any() and (want["accepted"] == 0).any() and ((want["accepted"] > 0) & (want["accepted"] < 200)).any()
    assert (nlev == 1).any() and (nlev == 2).any()
    if n >= 6:
        assert (nlev >= 4).any()
    XS.assert_same(got, want, "random n=%d" % n)


def test_many_chunks_per_spot_equal_the_spec(PK, four):
    """2 spots x S = 1 573: several chunks at the minimum of 8 attempts per lane, the last one partial; two levels and a last stand."""
    from pokerl_amd.cards import card_value as cv
    holes = np.array([[[cv("AS"), cv("AD")], [0xFF] * 2, [0xFF] * 2], [[0xFF] * 2, [cv("9C"), cv("8C")], [0xFF] * 2]], np.uint8)
    board = np.array([[cv("KS"), cv("7D"), cv("7C"), cv("2H"), 0], [cv("TC"), cv("JC"), cv("2D"), 0, 0]], np.uint8)
    nboard, live = np.array([4, 3], np.uint8), np.array([7, 7], np.uint16)
    ro = np.array([[U, 0, 1], [0, U, U]], np.uint16)
    bets = np.array([[20.0, 10.0, 30.0], [7.5, 7.5, 40.0]])
    got = device_ev(holes, board, nboard, live, bets, 1573, four, ro, nonce=9)
    XS.assert_same(got, spec(holes, board, nboard, live, bets, 1573, four, ro, nonce=9), "S = 1 573")
    assert (got["accepted"] > 0).all() and (got["accepted"] < 1573).all()


def test_the_three_lds_classes(PK, four):
    """R = 0 with range_of NULL (no cumulative row in LDS), R = 1, and R = 16 with every row used at sixteen seats on a full ladder: all eight
    groups of levels run."""
    rng = np.random.default_rng(16)
    holes, board, nboard, live = WS.random_spots(rng, 6, 8)
    bets = pattern_bets(6, live)
    XS.assert_same(device_ev(holes, board, nboard, live, bets, 100), spec(holes, board, nboard, live, bets, 100), "R = 0")
    one = four[1]
    ro = np.zeros((8, 6), np.uint16)
    got = device_ev(holes, board, nboard, live, bets, 100, one, nonce=1)                 # one vector: every hidden seat draws from it
    XS.assert_same(got, spec(holes, board, nboard, live, bets, 100, one, ro, nonce=1), "R = 1")
    w = disjoint_rows(rng)
    h16 = np.full((3, 16, 2), 0xFF, np.uint8)
    b16 = np.array([[ES.CANON[48], ES.CANON[49], ES.CANON[50], ES.CANON[51], 0]] * 3, np.uint8)
    nb16, lv16 = np.array([0, 3, 4], np.uint8), np.full(3, 0xFFFF, np.uint16)
    ro16 = np.array([np.arange(16), np.arange(16)[::-1], (np.arange(16) * 5) % 16], np.uint16)
    ladder = np.tile(10.0 * (np.arange(16) + 1), (3, 1))
    got = device_ev(h16, b16, nb16, lv16, ladder, 100, w, ro16, nonce=2)
    want = spec(h16, b16, nb16, lv16, ladder, 100, w, ro16, nonce=2)
    assert (want["accepted"] == 100).all() and (want["level_seat"] != XS.NO_LEVEL).all() and (want["amount"][:, :15] > 0).all()
    XS.assert_same(got, want, "R = 16")


def test_identities_on_the_device_that_need_no_spec(PK, four):
    from pokerl_amd import judger as J
    rng = np.random.default_rng(300)
    m, n = 40, 6
    holes, board, nboard, live = WS.random_spots(rng, n, m)
    ro = mixed_rows(rng, m, n)
    ids = (np.arange(m, dtype=np.uint32) * np.uint32(2654435761)).astype(np.uint32)
    # equal bets: one level, whose share row and `accepted` are pk_equity_ranged's for the same arguments
    equal = np.full((m, n), 12.5)
    got = device_ev(holes, board, nboard, live, equal, 130, four, ro, nonce=3, ids=ids)
    eq = J.ranged_equity_batch(holes, board, nboard, live, four, ro, 130, SEED, 3, ids)
    assert not got["status"].any() and np.array_equal(got["accepted"], eq.accepted) and (got["accepted"] > 0).any()
    assert np.array_equal(got["share"][:, 0, :], eq.share) and not got["share"][:, 1:].any()
    # nothing hidden on complete boards with integer bets: every attempt is the same showdown, ev is bit-equal to pk_equity_ev's (both
    # quotients are correctly rounded from the same real number: the products amount * share stay far below 2^53)
    h5, b5, nb5, lv5 = ES.random_spots(rng, n, 16, nb=5, unknown=False)
    ibets = pattern_bets(n, lv5).round()
    shown = device_ev(h5, b5, nb5, lv5, ibets, 77, four, mixed_rows(rng, 16, n), nonce=1)
    exact = J.showdown_ev_batch(h5, b5, nb5, lv5, ibets)
    assert (shown["accepted"] == 77).all() and not exact.status.any() and (exact.boards == 1).all()
    assert float(ibets.sum(axis=1).max()) * 77 * ES.SHARE_UNIT < 2.0 ** 53
    assert np.array_equal(shown["share"], 77 * exact.share) and np.array_equal(shown["level_seat"], exact.level_seat)
    assert np.array_equal(bits(shown["amount"]), bits(exact.amount)) and np.array_equal(bits(shown["ev"]), bits(exact.ev))
    # nonces add; merged re-forms ev by the formula on the sums
    bets = pattern_bets(n, live)
    ra, rb = (J.ranged_ev_batch(holes[:12], board[:12], nboard[:12], live[:12], bets[:12], four, ro[:12], 256, SEED, x) for x in (3, 4))
    a, b = as_dict(ra), as_dict(rb)
    assert (a["share"] != b["share"]).any()
    total = as_dict(ra.merged(rb))
    assert np.array_equal(total["share"], a["share"] + b["share"]) and np.array_equal(total["accepted"], a["accepted"].astype(np.uint64) + b["accepted"])
    want = XS.merged(a, b, bets[:12])
    assert np.array_equal(bits(total["ev"]), bits(want["ev"]))
    # a spot's result does not depend on the batch around it
    for k in (0, 7, m - 1):
        alone = device_ev(holes[k:k + 1], board[k:k + 1], nboard[k:k + 1], live[k:k + 1], equal[k:k + 1], 130, four, ro[k:k + 1], nonce=3, ids=ids[k:k + 1])
        XS.assert_same(alone, pick(got, slice(k, k + 1)), "spot %d alone" % k)


def test_refused_spots_inside_a_batch(PK, four):
    rng = np.random.default_rng(9)
    n = 6
    holes, board, nboard, live = ES.random_spots(rng, n, 24, unknown=False)
    holes[:, 1:] = 0xFF                                                       # seat 0 shown, the others hidden where they are live
    live |= 0b111                                                             # seats 0, 1 and 2 live everywhere
    ro = mixed_rows(rng, 24, n)
    ro[:, 1] = 0
    bets = pattern_bets(n, live)
    clean = device_ev(holes, board, nboard, live, bets, 100, four, ro)
    assert not clean["status"].any()
    h, b, nb, lv, r, be = holes.copy(), board.copy(), nboard.copy(), live.copy(), ro.copy(), bets.copy()
    want = {}
    h[3, 1, 0] = [c for c in ES.CANON if c not in set(h[3, 0].tolist()) | set(b[3].tolist())][0]; want[3] = ES.BAD_CARD   # a half-hidden live seat
    be[5, 2] = -1.0; want[5] = XS.BAD_BET
    r[7, 1] = 4; want[7] = ES.BAD_CARD                                       # a row that does not exist, at a hidden seat
    r[9, 0] = 4                                                              # ... at a shown seat: ignored
    nb[11] = 5; h[11, 0, 0] = b[11, 4]; want[11] = ES.DUP_CARD               # a card twice
    be[13, 5] = np.nan; want[13] = XS.BAD_BET                                # (at a seat that may be folded: its money still counts)
    nb[15] = 6; want[15] = ES.BAD_NBOARD
    be[17, 0] = np.inf; want[17] = XS.BAD_BET
    lv[19] = 0; want[19] = ES.NO_LIVE
    be[20, 1] = -0.0                                                         # -0.0 is a zero
    got = device_ev(h, b, nb, lv, be, 100, four, r)
    XS.assert_same(got, spec(h, b, nb, lv, be, 100, four, r), "bad spots v spec")
    for i in range(24):
        if i in want:
            assert got["status"][i] & want[i], i                             # (invariants() has checked the zeros)
        elif i != 20:
            XS.assert_same(pick(got, slice(i, i + 1)), pick(clean, slice(i, i + 1)), "neighbour %d" % i)
    assert got["status"][20] == 0
    # ... and each neighbour of a refused spot equals its single-spot result
    for i in (4, 6, 12, 14):
        alone = device_ev(h[i:i + 1], b[i:i + 1], nb[i:i + 1], lv[i:i + 1], be[i:i + 1], 100, four, r[i:i + 1], ids=np.array([i], np.uint32))
        XS.assert_same(alone, pick(got, slice(i, i + 1)), "spot %d alone" % i)
    # all bets zero: no level, ev all +0.0, the attempts are still counted
    z = device_ev(holes[:4], board[:4], nboard[:4], live[:4], np.zeros((4, n)), 100, four, ro[:4])
    assert not z["status"].any() and (z["level_seat"] == XS.NO_LEVEL).all() and not bits(z["ev"]).any()
    assert np.array_equal(z["accepted"], clean["accepted"][:4])


def table_want(g, observer, samples, nonce, weights, range_of, tables=None):
    holes, board, nboard, live, bets = XS.table_spots(g.deck, g.player_states, g.turn, g.active_player, observer, g.bets, g.pending_bets)
    t = np.arange(g.num_tables) if tables is None else np.asarray(tables)
    ids = (g.table_id_base + t) % 2 ** 32
    ro = np.asarray(range_of)
    return XS.batch_ev(holes[t], board[t], nboard[t], live[t], bets[t], samples, weights, ro, per_spot=ro.ndim == 2, nonce=nonce, ids=ids,
                       key=WS.R.seed_key(g.seed)), (live, bets)


@pytest.mark.parametrize("shape", [(64, 6), (48, 3)])
def test_table_form_equals_the_spec_fed_from_the_getters(PK, four, shape):
    """The never-fold caller on ladder stacks drives raised multi-way hands to later streets (ev_witness): side pots.  Observer 'active' and a
    fixed seat, range_of by seat and per table, table indices that repeat, an index out of range."""
    from hip_backend import HipBackend
    tables, n = shape
    seed, steps = {(64, 6): (5, 17), (48, 3): (31, 8)}[shape]
    hb = HipBackend(tables, n, start_credits=W.ladder_stacks(n), seed=seed)
    W.deep_steps(hb, steps)
    g = hb.g
    rng = np.random.default_rng(n)
    before = g.save()
    shared = np.array([0, 1, U, 0, 3, 1][:n], np.uint16)
    per = rng.choice(np.array([0, 1, U], np.uint16), (tables, n))
    for observer in ("active", 1):
        r = g.ev_ranged(observer=observer, ranges=four, range_of=shared, samples=64, nonce=11)
        got = as_dict(r)
        assert not got["status"].any()
        o = WS.OBSERVER_ACTIVE if observer == "active" else observer
        want, (live, bets) = table_want(g, o, 64, 11, four, shared)
        ll = W.live_levels(live, bets)
        assert any(a >= 3 and c >= 2 for a, c in ll)
        XS.assert_same(got, want, "table form %dx%d observer %r, range_of by seat" % (tables, n, observer))
        assert np.array_equal(r.bets, g.bets + g.pending_bets)
        ok = got["accepted"] > 0
        assert ok.any() and np.array_equal(r.payout[ok], (r.ev + r.bets)[ok])
        rp = as_dict(g.ev_ranged(observer=observer, ranges=four, range_of=per, samples=64, nonce=11))
        XS.assert_same(rp, table_want(g, o, 64, 11, four, per)[0], "range_of per table")
        idx = np.array([5, 5, tables - 1, 0, 17, 5], np.int32)                # an index array, repeats included: range_of per SPOT
        sub = as_dict(g.ev_ranged(idx, observer=observer, ranges=four, range_of=per[idx], samples=64, nonce=11))
        XS.assert_same(sub, pick(rp, idx), "index array")
    assert (got["level_seat"] != XS.NO_LEVEL).sum(axis=1).max() >= 2
    r = g.ev_ranged(np.array([0, tables, -1, 5], np.int64), ranges=four[0], samples=64)
    assert r.status.tolist() == [0, ES.BAD_TABLE, ES.BAD_TABLE, 0]
    invariants({k: np.asarray(getattr(r, k)) for k in KEYS})
    assert g.save().tobytes() == before.tobytes()                            # the calls wrote nothing to the handle
    if n == 3:                                                               # the single game
        single = PK.Game(num_players=3)
        with pytest.raises(ValueError):
            single.ev_ranged(ranges=four[0])                                  # never dealt
        single.reset()
        e = single.ev_ranged(ranges=four, range_of=[0, 1, U], samples=256)
        assert e.ev.shape == e.payout.shape == (3,) and e.share.shape == (3, 3) and e.status == 0 and 0 < e.accepted <= 256
        want, _ = table_want(single._v, WS.OBSERVER_ACTIVE, 256, 0, four, np.array([0, 1, U], np.uint16))
        XS.assert_same({k: np.asarray(getattr(e, k))[None] for k in KEYS}, want, "Game.ev_ranged")
        single.close()
    g.close()


def test_device_forms_on_a_callers_stream(PK, four):
    from pokerl_amd import hipmem
    from pokerl_amd import judger as J
    rng = np.random.default_rng(77)
    n, m, s = 6, 60, 96
    holes, board, nboard, live = WS.random_spots(rng, n, m)
    ro = mixed_rows(rng, m, n)
    ids = rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32)
    bets = pattern_bets(n, live)
    want = device_ev(holes, board, nboard, live, bets, s, four, ro, nonce=6, ids=ids)
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0             # hipStreamNonBlocking: a caller's own stream
    ins = [hipmem.DeviceBuffer(x.nbytes).upload(x) for x in (holes, board, nboard, live, bets, ids, four, ro)]
    sizes = dict(share=(m * n * n * 8, np.uint64, (m, n, n)), level_seat=(m * n, np.uint8, (m, n)), amount=(m * n * 8, np.float64, (m, n)),
                 ev=(m * n * 8, np.float64, (m, n)), accepted=(m * 4, np.uint32, (m,)), status=(m, np.uint8, (m,)))
    outs = {k: hipmem.DeviceBuffer(v[0]) for k, v in sizes.items()}

    def call(skip=None):
        for k, b in outs.items():
            b.upload(np.full(sizes[k][0], 0x5A, np.uint8))                    # (the call writes every output it is given itself)
        o = {k + "_d": (None if k == skip else b.ptr) for k, b in outs.items()}
        J.ranged_ev_d(n, m, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, ins[4].ptr, s, weights_d=ins[6].ptr, num_ranges=4, range_of_d=ins[7].ptr,
                      ids_d=ins[5].ptr, seed=SEED, nonce=6, stream=stream, **o)
        assert hip.hipStreamSynchronize(stream) == 0
        d = {k: outs[k].download(sizes[k][1], int(np.prod(sizes[k][2]))).reshape(sizes[k][2]) for k in outs}
        for k in outs:
            if k == skip:
                assert (outs[k].download(np.uint8, sizes[k][0]) == 0x5A).all(), k      # an output that was not asked for is not touched
            else:
                a, b = (d[k], want[k]) if k in XS.INT_KEYS else (bits(d[k]), bits(want[k]))
                assert np.array_equal(a, b), (skip, k)

    call()
    for skip in ("share", "level_seat", "amount", "ev", "accepted"):         # NULL for each optional output in turn
        call(skip)
    for x in ins + list(outs.values()):
        x.free()
    assert hip.hipStreamDestroy(stream) == 0
    # the table form's device call: equal to the host form, NULL outputs included
    from hip_backend import HipBackend
    hb = HipBackend(64, 6, start_credits=W.ladder_stacks(6), seed=5)
    W.deep_steps(hb, 17)
    g = hb.g
    shared = np.array([0, 1, U, 0, 3, 1], np.uint16)
    whole = as_dict(g.ev_ranged(ranges=four, range_of=shared, samples=64, nonce=5))
    T = 64
    wd, rd = hipmem.DeviceBuffer(four.nbytes).upload(four), hipmem.DeviceBuffer(shared.nbytes).upload(shared)
    ev_d, st_d, sh_d = hipmem.DeviceBuffer(T * n * 8), hipmem.DeviceBuffer(T), hipmem.DeviceBuffer(T * n * n * 8)
    g.ev_ranged_d(st_d, weights_d=wd, num_ranges=4, range_of_d=rd, samples=64, nonce=5, ev_d=ev_d)
    g.sync()
    assert np.array_equal(bits(ev_d.download(np.float64, T * n).reshape(T, n)), bits(whole["ev"])) and not st_d.download(np.uint8, T).any()
    g.ev_ranged_d(st_d, weights_d=wd, num_ranges=4, range_of_d=rd, samples=64, nonce=5, share_d=sh_d)
    g.sync()
    assert np.array_equal(sh_d.download(np.uint64, T * n * n).reshape(T, n, n), whole["share"])
    for x in (wd, rd, ev_d, st_d, sh_d):
        x.free()
    g.close()


def five_sigma(dev, bound, where):
    print(where, "deviation", np.asarray(dev).tolist(), "bound", np.asarray(bound).tolist())
    assert (np.asarray(dev) <= np.asarray(bound)).all(), (where, dev, bound)


def test_converges_to_the_exact_values(PK):
    """S = 2^20, the two spots of the CPU convergence test with the same derived bounds: heads-up on the turn, hero EV against
    2 b0 (agg0 + agg1 / 2) / agg2 - b0 within 5 * 2 b0 * sqrt(p (1 - p) / accepted); three seats on two compared levels, every seat's payout
    against the host enumeration within 5 sqrt(var / accepted).  Seeds fixed; the deviations are printed before the assertion."""
    from pokerl_amd import judger as J
    s = 1 << 20
    holes, board, nb, live = XS.turn_spot()
    w = XS.turn_range()
    agg = RS.aggregate(RS.spot_range(holes[0], board, nb), w)
    b0 = 10.0
    got = J.ranged_ev([holes[0].tolist(), None], board[:4], bets=[b0, 30.0], ranges=w, samples=s, seed=SEED, nonce=1)
    acc = float(got.accepted)
    assert got.status == 0 and 0 < acc < s and got.levels == [(0, 20.0), (1, 20.0)]
    p = (agg[0] + agg[1] / 2) / agg[2]
    five_sigma(abs(got.ev[0] - (2 * b0 * p - b0)), 5 * 2 * b0 * np.sqrt(p * (1 - p) / acc), "turn spot, hero EV (accepted %d):" % acc)
    holes, board, nb, live, w2, ro = XS.three_seat_spot()
    mean, var, _ = XS.three_seat_exact()
    assert (mean > 0).all()
    g3 = J.ranged_ev([holes[0].tolist(), None, None], board, bets=XS.THREE_BETS, ranges=w2, range_of=ro, samples=s, seed=SEED, nonce=1)
    acc = float(g3.accepted)
    assert g3.status == 0 and 0 < acc < s and [x for x, _ in g3.levels] == [1, 0, 2]
    five_sigma(np.abs(g3.payout - mean), 5 * np.sqrt(var / acc), "three seats, payouts (accepted %d):" % acc)
