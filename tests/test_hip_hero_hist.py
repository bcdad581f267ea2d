"""GPU tests of the hero strength histogram (pk_equity_hist_hero, include/pokerl_hip.h "Hero strength histogram"): every comparison is exact
integer equality -- against the reference's fixture rows, the numpy restatement tests/hero_hist_spec.py, row h of the public form
(strength_histogram) on the device, the explicit form fed from the getters, and, for the bucket stage, assign_histograms on the rows of the
same call and tests/hist_cluster_spec.py."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import equity_range_spec as RS
import hero_hist_spec as HH
import hist_cluster_spec as CS
import hist_spec as HS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("hist", "void", "completions", "status")
H = HH.HOLDINGS
BINS = (1, 2, 7, 10, 32)
NONE = 0xFFFF


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


def as_dict(r):
    """The outputs of a call, with the invariant checked on every spot of every test: the bins and `void` add up to `completions`."""
    out = {k: np.asarray(getattr(r, k)) for k in KEYS}
    assert out["hist"].dtype == np.uint16 and out["void"].dtype == np.uint16
    assert (out["hist"].sum(axis=-1, dtype=np.int64) + out["void"] == out["completions"]).all()
    bad = out["status"] != 0
    assert not out["completions"][bad].any() and (out["completions"][~bad] > 0).all()
    return out


def device(hero, board, nboard, dead=None, weights=None, bins=10, centroids=None):
    from pokerl_amd import judger as J
    return as_dict(J.hero_histogram_batch(hero, board, nboard, dead, weights, bins, centroids))


def assert_equal(got, want, where, keys=KEYS):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and (a.astype(np.int64) == b.astype(np.int64)).all(), (where, k, np.argwhere(a.astype(np.int64) != b.astype(np.int64))[:4].tolist())


def rows(d, sel):
    return {k: v[sel] for k, v in d.items()}


def random_weights(rng, shape=(H,)):
    w = rng.integers(0, 65536, shape).astype(np.uint16)
    for row in w.reshape(-1, H):
        row[rng.integers(0, H, 300)] = 0
        row[rng.integers(0, H, 100)] = 65535
    return w


def hero_of(h):
    return [RS.CANON[RS.PAIR_A[h]], RS.CANON[RS.PAIR_B[h]]]


def concat(parts):
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(len(parts[0])))


# ---- 1
def test_every_fixture_row_equals_the_reference(PK):
    with open(os.path.join(ROOT, "tests", "golden", "hist_ref.json")) as f:
        ref = json.load(f)
    hero, board, nboard, dead, where = [], [], [], [], []
    for si, s in enumerate(ref["spots"]):
        for h in s["h"]:
            hero.append(hero_of(h)); board.append(s["board"] + [0] * (5 - len(s["board"]))); nboard.append(len(s["board"])); dead.append(s["dead"])
            where.append((si, h))
    hero, board, nboard, dead = np.array(hero, np.uint8), np.array(board, np.uint8), np.array(nboard, np.uint8), np.array(dead, np.uint64)
    m = len(where)
    assert m == sum(len(s["h"]) for s in ref["spots"])
    for case in ("ones", "random", "dying"):
        weights = None if case == "ones" else np.stack([HS.fixture_weights(ref, ref["spots"][si], case) for si, _ in where])
        for bins in ref["bins"]:
            exp = {si: HS.fixture_expected(s, case, bins) for si, s in enumerate(ref["spots"])}
            want = dict(hist=np.stack([exp[si][0][h] for si, h in where]), void=np.array([exp[si][1][h] for si, h in where]),
                        completions=np.array([ref["spots"][si]["completions"] for si, _ in where]), status=np.zeros(m, np.uint8))
            assert_equal(device(hero, board, nboard, dead, weights, bins), want, "the fixture in one batch, %s, %d bins" % (case, bins))
            if bins == 7 and case != "ones":
                for i in range(0, m, 3):                          # ... and one spot at a time (m = 1: a lone workgroup)
                    assert_equal(device(hero[i:i + 1], board[i:i + 1], nboard[i:i + 1], dead[i:i + 1], weights[i], bins), rows(want, slice(i, i + 1)),
                                 "fixture row %d alone, %s" % (i, case))
                if case == "dying":
                    assert want["void"].any()
    exp = {si: HS.fixture_expected(s, "ones", 7) for si, s in enumerate(ref["spots"])}
    ones = dict(hist=np.stack([exp[si][0][h] for si, h in where]), void=np.array([exp[si][1][h] for si, h in where]),
                completions=np.array([ref["spots"][si]["completions"] for si, _ in where]), status=np.zeros(m, np.uint8))
    for i in range(m):                                            # every row alone, once
        assert_equal(device(hero[i:i + 1], board[i:i + 1], nboard[i:i + 1], dead[i:i + 1], None, 7), rows(ones, slice(i, i + 1)), "fixture row %d alone, ones" % i)


# ---- 2: the pool sizes AFTER the hero at which the set loop can break: C(P, k + 2) = 1, a few, either side of 512 lanes and of two sets per lane
POOLS = {"flop": (3, (4, 5, 10, 11, 14)), "turn": (4, (3, 4, 15, 16)), "river": (5, (2, 3, 32, 33, 47))}


@pytest.mark.parametrize("street", ["flop", "turn", "river"])
def test_random_spots_equal_the_spec(PK, street):
    nb, pools = POOLS[street]
    rng = np.random.default_rng(nb)
    hero, board, nboard, dead = concat([RS.random_spots(rng, 2, nb, p) for p in pools])
    m = len(hero)
    sets = sorted({math.comb(p, 7 - nb) for p in pools})
    assert sets[0] == 1 and any(s < 512 for s in sets[1:]) and any(s > 512 for s in sets) and any(s % 512 for s in sets)
    w = rng.integers(0, 200, H)
    w[rng.random(H) < 0.33] = 0
    ranges = np.stack([w, np.full(H, 65535), np.ones(H, np.int64), np.zeros(H, np.int64)]).astype(np.uint16)   # random / 65 535 / ones / zero
    spec = [HH.spot_hero_hist(hero[i], [int(x) for x in board[i]], nb, int(dead[i]), ranges, BINS) for i in range(m)]
    assert all(s["status"] == 0 and s["completions"] == math.comb(pools[i // 2], 5 - nb) for i, s in enumerate(spec))
    for r in range(4):
        for bins in BINS:
            want = dict(hist=np.stack([s["hist"][bins][r] for s in spec]), void=np.array([s["void"][r] for s in spec]),
                        completions=np.array([s["completions"] for s in spec]), status=np.zeros(m, np.uint8))
            got = device(hero, board, nboard, dead, ranges[r], bins)
            assert_equal(got, want, "%s, range %d, %d bins" % (street, r, bins))
            if r == 3:
                assert (got["void"] == got["completions"]).all() and not got["hist"].any()      # the zero range: every completion is void
    assert_equal(device(hero, board, nboard, dead, None, 10), dict(hist=np.stack([s["hist"][10][2] for s in spec]), void=np.array([s["void"][2] for s in spec]),
                                                                   completions=np.array([s["completions"] for s in spec]), status=np.zeros(m, np.uint8)),
                 "%s, NULL weights = ones" % street)


# ---- 3
@pytest.mark.parametrize("nb", [3, 4, 5])
def test_row_identity_on_the_device_at_the_full_pools(PK, nb):
    """All C(52 - nb, 2) hero spots of one random board in ONE batch against the public form of the board: on the flop 1 176 spots -- a
    workgroup of the persistent grid takes a second spot -- with 1 081 completions each -- the hero pass loops three times."""
    from pokerl_amd import judger as J
    rng = np.random.default_rng(30 + nb)
    deck = [int(x) for x in rng.permutation(52)]
    cards = [RS.CANON[c] for c in deck[:nb]]
    sparse = np.zeros(H, np.uint16)
    sparse[rng.integers(0, H, 200)] = 65535                                  # zeros with 65 535s
    for weights in (sparse, random_weights(rng)):
        pub = J.strength_histogram(cards, weights=weights, bins=10)
        hs = np.flatnonzero(pub.valid)
        m = len(hs)
        assert m == math.comb(52 - nb, 2) and (nb != 3 or (m == 1176 and pub.completions == 1081))
        hero = np.array([hero_of(h) for h in hs], np.uint8)
        board = np.zeros((m, 5), np.uint8)
        board[:, :nb] = cards
        got = device(hero, board, np.full(m, nb, np.uint8), None, weights, 10)
        want = dict(hist=np.asarray(pub.hist)[hs], void=np.asarray(pub.void)[hs], completions=np.full(m, int(pub.completions)), status=np.zeros(m, np.uint8))
        assert_equal(got, want, "nb = %d" % nb)
    assert want["hist"].any()


# ---- 4
@pytest.fixture(scope="module")
def mixed():
    """800 mixed river / turn / small flop spots and their spec under per-spot and under shared weights: computed once, sliced by the tests."""
    rng = np.random.default_rng(44)
    parts = []
    for i in range(800):
        nb = (5, 4, 3)[i % 3]
        parts.append(RS.random_spots(rng, 1, nb, int(rng.integers(7 - nb, (34, 14, 9)[i % 3]))))
    hero, board, nboard, dead = concat(parts)
    per_spot, shared = random_weights(rng, (800, H)), random_weights(rng)
    return dict(spots=(hero, board, nboard, dead), per_spot=per_spot, shared=shared, want_per_spot=HH.batch_hero_hist(hero, board, nboard, dead, per_spot, 10),
                want_shared=HH.batch_hero_hist(hero, board, nboard, dead, shared, 7))


@pytest.mark.parametrize("m", [1, 65, 800])
def test_batches_of_mixed_spots_equal_the_spec(PK, mixed, m):
    hero, board, nboard, dead = (x[:m] for x in mixed["spots"])
    assert_equal(device(hero, board, nboard, dead, mixed["per_spot"][:m], 10), rows(mixed["want_per_spot"], slice(0, m)), "m = %d, per-spot weights" % m)
    assert_equal(device(hero, board, nboard, dead, mixed["shared"], 7), rows(mixed["want_shared"], slice(0, m)), "m = %d, shared weights" % m)


def test_each_output_alone_and_a_call_of_nothing(PK, mixed):
    from pokerl_amd import hipmem
    from pokerl_amd import judger as J
    m, bins = 65, 7
    hero, board, nboard, dead = (x[:m] for x in mixed["spots"])
    want = rows(mixed["want_shared"], slice(0, m))
    ins = [hipmem.DeviceBuffer(x.nbytes).upload(x) for x in (hero, board, nboard, dead, mixed["shared"])]
    shapes = dict(hist=(np.uint16, m * bins), void=(np.uint16, m), completions=(np.uint32, m), status=(np.uint8, m))
    bufs = {k: hipmem.DeviceBuffer(n * np.dtype(dt).itemsize) for k, (dt, n) in shapes.items()}

    def call(keys, count=m):
        for k, (dt, n) in shapes.items():
            bufs[k].upload(np.full(n, 7, dt))                                # every entry asked for is written; nothing else is touched
        kw = {("void_d" if k == "void" else k + "_d"): bufs[k].ptr for k in keys}
        J.hero_histogram_d(count, *[x.ptr for x in ins[:4]], weights_d=ins[4].ptr, bins=bins, **kw)
        assert hipmem._lib().hipDeviceSynchronize() == 0
        return {k: bufs[k].download(dt, n) for k, (dt, n) in shapes.items()}
    for keys in (("hist",), ("void",), ("completions",), ("status",), KEYS):
        got = call(keys)
        for k in KEYS:
            if k in keys:
                assert (got[k].reshape(np.asarray(want[k]).shape) == want[k]).all(), (keys, k)
            else:
                assert (got[k] == 7).all(), (keys, k)
    got = call(KEYS, count=0)                                                # m = 0 writes nothing
    assert all((got[k] == 7).all() for k in KEYS)
    for x in ins + list(bufs.values()):
        x.free()
    r = J.hero_histogram_batch(np.zeros((0, 2), np.uint8), np.zeros((0, 5), np.uint8), np.zeros(0, np.uint8))
    assert r.hist.shape == (0, 10) and r.status.shape == (0,)


# ---- 5
def test_bad_spots_inside_a_batch(PK):
    from pokerl_amd import judger as J
    rng = np.random.default_rng(9)
    hero, board, nboard, dead = concat([RS.random_spots(rng, 16, 5, lambda i: 20), RS.random_spots(rng, 16, 4, lambda i: 12), RS.random_spots(rng, 16, 3, 8)])
    order = rng.permutation(len(hero))
    hero, board, nboard, dead = hero[order], board[order], nboard[order], dead[order]
    weights = random_weights(rng)
    clean = device(hero, board, nboard, dead, weights, 10)
    assert not clean["status"].any()
    assert_equal(clean, HH.batch_hero_hist(hero, board, nboard, dead, weights, 10), "the clean batch vs spec")
    he, b, nb, d = hero.copy(), board.copy(), nboard.copy(), dead.copy()
    used = lambda i: {RS.canon_index(int(c)) for c in list(he[i]) + list(b[i, :nb[i]])}
    want = {}
    b[1, 0] = 0x4F; want[1] = RS.BAD_CARD                                     # a byte that is no card
    b[4, 2] = 0x0D; want[4] = RS.BAD_CARD
    b[7, 1] = 0xFF; want[7] = RS.BAD_CARD                                     # 0xFF in the board
    d[10] |= np.uint64(1) << np.uint64(52); want[10] = RS.BAD_CARD            # a dead bit that is no card
    d[13] = np.uint64(1) << np.uint64(63); want[13] = RS.BAD_CARD
    b[16, 2] = b[16, 0]; want[16] = RS.DUP_CARD                               # a card twice
    d[22] |= np.uint64(1) << np.uint64(RS.canon_index(int(b[22, 0]))); want[22] = RS.DUP_CARD   # a board card that is also dead
    nb[28] = 6; want[28] = RS.BAD_NBOARD
    nb[31] = 255; want[31] = RS.BAD_NBOARD
    nb[33] = 0; want[33] = RS.PREFLOP
    nb[37] = 2; want[37] = RS.PREFLOP
    for i, n in ((39, 5), (41, 4), (43, 3)):                                  # P = k + 1: one card short of the board to come and one holding
        nb[i] = n
        free = [c for c in range(52) if c not in used(i)]
        d[i] = sum(1 << c for c in free[(5 - n) + 1:])
        want[i] = RS.SMALL_POOL
    he[2, 0] = 0x4A; want[2] = RS.BAD_CARD                                    # a bad hero card: suit 4
    he[5, 1] = 0xFF; want[5] = RS.BAD_CARD
    he[19, 1] = he[19, 0]; want[19] = RS.DUP_CARD                             # the hero holds a card twice
    he[24, 0] = b[24, 1]; want[24] = RS.DUP_CARD                              # ... a board card
    d[26] |= np.uint64(1) << np.uint64(RS.canon_index(int(he[26, 1]))); want[26] = RS.DUP_CARD   # ... a dead card
    got = device(he, b, nb, d, weights, 10)
    assert got["status"].tolist() == [RS.check_spot(he[i], b[i], nb[i], d[i])[0] for i in range(len(b))]
    assert got["status"].tolist() == J.range_equity_batch(he, b, nb, d, weights, per_holding=False).status.tolist()   # the same spot, the same status
    for i in range(len(b)):
        if i in want:
            assert got["status"][i] == want[i] and not got["hist"][i].any() and got["void"][i] == 0 and got["completions"][i] == 0, i
        else:
            assert_equal(rows(got, slice(i, i + 1)), rows(clean, slice(i, i + 1)), "neighbour %d" % i)


# ---- 6
def explicit_from_getters(g, observer, tables=None, weights=None, bins=10, centroids=None):
    deck, turn = g.deck, g.turn
    who = g.active_player.astype(np.int64) if observer == "active" else np.full(len(deck), observer, np.int64)
    hero, board, nboard = RS.table_spots(deck, turn, who)
    if tables is not None:
        hero, board, nboard = hero[tables], board[tables], nboard[tables]
        if weights is not None and np.ndim(weights) == 2:
            pass                                                              # (per-spot weights are per SPOT of the call already)
    return device(hero, board, nboard, None, weights, bins, centroids)


@pytest.mark.parametrize("n,steps", [(2, 9), (6, 37), (16, 61)])
def test_table_form_equals_explicit_form(PK, n, steps):
    T = 165
    g = PK.VecGame(T, num_players=n, seed=91 + n)
    g.reset()
    g.rollout(steps, policy=0, auto_reset=True, fused=True)
    turn = g.turn
    assert set(turn.tolist()) == {0, 1, 2, 3}, sorted(set(turn.tolist()))    # every turn a table can rest at
    before = g.save()
    pre = turn == 0
    rng = np.random.default_rng(n)
    weights = random_weights(rng)
    for observer in ("active", n - 1):
        want = explicit_from_getters(g, observer, weights=weights)
        assert (want["status"][pre] == RS.PREFLOP).all() and not want["status"][~pre].any()
        got = as_dict(g.equity_hist_hero(observer=observer, weights=weights))
        assert_equal(got, want, "table form %dx%d, observer %r" % (T, n, observer))
        assert set(got["completions"][~pre].tolist()) == {math.comb(45, 0), math.comb(46, 1), math.comb(47, 2)}
    pick = np.concatenate([rng.permutation(T)[:20], [5, 5, 5, T - 1, 0]]).astype(np.int32)   # permuted, repeated indices
    got = as_dict(g.equity_hist_hero(observer=0, weights=weights, tables=pick, bins=32))
    assert_equal(got, explicit_from_getters(g, 0, pick, weights, 32), "table form %dx%d, index array, 32 bins" % (T, n))
    r = g.equity_hist_hero(tables=np.array([int(pick[0]), T, -1, 2 ** 31 - 1], np.int64), bins=3)
    assert r.status[1:].tolist() == [RS.BAD_TABLE] * 3 and not r.completions[1:].any() and not r.hist[1:].any() and not r.void[1:].any()
    assert r.hist.shape == (4, 3) and r.label is None
    assert g.save().tobytes() == before.tobytes()                            # the calls wrote nothing to the handle
    # PK_OBSERVER_NONE is refused, in Python and at the C entry point (return code and text)
    with pytest.raises(ValueError, match="observer"):
        g.equity_hist_hero(observer=None)
    from pokerl_amd import _lib as L
    st = np.zeros(T, np.uint8)
    rc = L.lib().pk_table_equity_hist_hero(g._h, None, T, L.OBSERVER_NONE, None, 0, 10, None, None, None, L.ptr(st), 0, None, None, None)
    assert rc == L.PK_E_INVALID_ARG and b"pk_table_equity_hist_hero: observer outside" in L.lib().pk_last_error(g._h)
    rc = L.lib().pk_table_equity_hist_hero(g._h, None, T, 0, None, 0, 33, None, None, None, L.ptr(st), 0, None, None, None)
    assert rc == L.PK_E_INVALID_ARG and b"nbins must be 1 .. PK_EQ_HIST_MAX_BINS (32)" in L.lib().pk_last_error(g._h)
    g.close()


def test_never_dealt_handle_and_the_single_game(PK):
    cen = np.array([[0, 65535], [65535, 65535]], np.uint16)
    g = PK.VecGame(64, num_players=6)
    r = g.equity_hist_hero(centroids=cen, bins=2)
    # turn 0: every table is PK_EQ_PREFLOP.  The status rule is range equity's, unchanged, and that family reads the observer's hole cards
    # at any turn: on a table never dealt they are no two different cards, so the same PK_EQ_DUP_CARD bit comes with it (include/pokerl_hip.h
    # "Range equity", STATUS) -- the same spot gets the same status from both families
    assert ((r.status & RS.PREFLOP) != 0).all() and not r.hist.any() and not r.void.any() and not r.completions.any()
    assert r.status.tolist() == g.equity_range().status.tolist() and set(r.status.tolist()) == {RS.PREFLOP | RS.DUP_CARD}
    assert r.hist.shape == (64, 2) and (r.label == NONE).all() and not r.dist.any()
    assert (g.bucket(cen) == NONE).all()
    g.reset()                                                                # dealt, and still at turn 0: PK_EQ_PREFLOP alone
    r = g.equity_hist_hero(centroids=cen, bins=2)
    assert (r.status == RS.PREFLOP).all() and not r.hist.any() and not r.void.any() and not r.completions.any() and (r.label == NONE).all()
    g.close()
    single = PK.Game(num_players=3)
    with pytest.raises(ValueError, match="fewer than three board cards"):
        single.equity_hist_hero()                                            # never dealt
    single.reset()
    with pytest.raises(ValueError, match="fewer than three board cards"):
        single.equity_hist_hero(bins=4)                                      # pre-flop
    with pytest.raises(ValueError, match="fewer than three board cards"):
        single.bucket(cen)
    with pytest.raises(ValueError, match="bins"):
        single.equity_hist_hero(bins=33)
    single.close()


# ---- 7
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
    r = as_dict(g.equity_hist_hero(observer=1))
    assert ((r["status"][~idle] & RS.IN_FLIGHT) != 0).all() and not (r["status"][idle] & RS.IN_FLIGHT).any()
    assert not r["hist"][~idle].any() and not r["void"][~idle].any() and not r["completions"][~idle].any()
    act.upload(np.full(T, -1, np.int32))                                     # the drain: idle tables get no step and stay as they are
    g.step_async_d(act, flags, terr, ready, max_hands=0, auto_reset=True)
    g.sync()
    t = np.flatnonzero(idle)
    assert_equal(rows(r, t), explicit_from_getters(g, 1, t), "the idle tables")
    for b in (act, flags, terr, ready):
        b.free()
    g.close()


# ---- 8
@pytest.fixture(scope="module")
def bucket_spots():
    """Good spots of every street, a refused spot, a pre-flop spot; with the zero range every row is all void."""
    rng = np.random.default_rng(88)
    hero, board, nboard, dead = concat([RS.random_spots(rng, 30, 5, 30), RS.random_spots(rng, 20, 4, 14), RS.random_spots(rng, 20, 3, 9)])
    board[3, 1] = board[3, 0]                                                # refused: a card twice
    nboard[11] = 2                                                           # pre-flop
    return hero, board, nboard, dead, random_weights(rng)


@pytest.mark.parametrize("K", [1, 2, 70])
@pytest.mark.parametrize("bins", [1, 7, 10, 32])
def test_bucket_stage_equals_assign_on_the_rows_of_the_call(PK, bucket_spots, K, bins):
    from pokerl_amd import judger as J
    hero, board, nboard, dead, weights = bucket_spots
    m = len(hero)
    rng = np.random.default_rng(1000 * K + bins)
    plain = device(hero, board, nboard, dead, weights, bins)
    q, empty = CS.quant(plain["hist"])
    assert empty[3] and empty[11] and empty.sum() == 2
    cen = np.sort(rng.integers(0, 65536, (K, bins)), axis=1).astype(np.uint16)
    cen[:, -1] = 65535
    live = np.flatnonzero(~empty)
    cen[0] = q[live[0]]                                                      # a row's own CDF: distance 0 ...
    if K > 1:
        cen[K - 1] = q[live[0]]                                              # ... twice: the tie goes to the smaller index
        cen[1] = q[live[1]]
        if K > 2:
            cen[2] = q[live[1]]
    r = J.hero_histogram_batch(hero, board, nboard, dead, weights, bins, cen)
    assert_equal(as_dict(r), plain, "the histograms of a call with a bucket stage")
    label, dist = J.assign_histograms(r.hist, cen)
    assert np.array_equal(r.label, label) and np.array_equal(r.dist, dist)                     # assign on the rows of the same call
    slabel, sdist = CS.assign(q, empty, cen)
    assert np.array_equal(r.label, slabel) and np.array_equal(r.dist, sdist)                   # ... and the spec's assignment
    second = 1 if K > 1 and not np.array_equal(q[live[1]], q[live[0]]) else 0
    assert r.label[live[0]] == 0 and r.dist[live[0]] == 0 and r.label[live[1]] == second and (K == 1 or r.dist[live[1]] == 0)
    assert r.label[3] == NONE and r.label[11] == NONE and r.dist[3] == 0 and r.dist[11] == 0   # refused, pre-flop
    assert (r.label[live] < K).all() and r.status[3] == RS.DUP_CARD and r.status[11] == RS.PREFLOP
    # label only (hist NULL: the rows live in the work space), dist only, and both without hist
    from pokerl_amd import _lib as L
    w, per_spot = J.range_weights(weights, m)
    for want_label, want_dist in ((True, False), (False, True), (True, True)):
        lab, dst = np.full(m, 7, np.uint16), np.full(m, 7, np.uint32)
        L.check(L.lib().pk_equity_hist_hero(0, m, L.ptr(hero), L.ptr(board), L.ptr(nboard), L.ptr(dead), L.ptr(w), per_spot, bins, None, None, None, None,
                                            K, L.ptr(cen), L.ptr(lab) if want_label else None, L.ptr(dst) if want_dist else None))
        assert np.array_equal(lab, label if want_label else np.full(m, 7)) and np.array_equal(dst, dist if want_dist else np.full(m, 7))
    # the zero range: every completion of every good spot is void -> an empty row
    z = J.hero_histogram_batch(hero, board, nboard, dead, np.zeros(H, np.uint16), bins, cen)
    assert not z.hist.any() and (z.void == z.completions).all() and (z.label == NONE).all() and not z.dist.any()


def test_vecgame_bucket_equals_the_explicit_composition(PK):
    from pokerl_amd import judger as J
    rng = np.random.default_rng(5)
    T, n = 165, 6
    g = PK.VecGame(T, num_players=n, seed=97)
    g.reset()
    g.rollout(37, policy=0, auto_reset=True, fused=True)
    assert set(g.turn.tolist()) == {0, 1, 2, 3}
    weights = random_weights(rng)
    cen = np.sort(rng.integers(0, 65536, (70, 10)), axis=1).astype(np.uint16)
    cen[:, -1] = 65535
    for observer, tables in (("active", None), (2, np.array([7, 7, 0, T - 1, 33], np.int32))):
        want = explicit_from_getters(g, observer, tables, weights, 10)
        label, dist = J.assign_histograms(want["hist"], cen)
        got = g.bucket(cen, observer=observer, weights=weights, tables=tables)
        assert got.dtype == np.uint16 and np.array_equal(got, label)
        full = g.equity_hist_hero(observer=observer, weights=weights, tables=tables, bins=10, centroids=cen)
        assert np.array_equal(full.label, label) and np.array_equal(full.dist, dist) and np.array_equal(full.hist, want["hist"])
        assert (label[want["status"] != 0] == NONE).all() and (label[want["status"] == 0] < 70).all()
    # the device form, labels alone
    from pokerl_amd.hipmem import DeviceBuffer
    cen_d, lab_d = DeviceBuffer(cen.nbytes).upload(cen), DeviceBuffer(T * 2).upload(np.full(T, 7, np.uint16))
    g.equity_hist_hero_d(bins=10, k=70, centroids_d=cen_d, label_d=lab_d)
    g.sync()
    assert np.array_equal(lab_d.download(np.uint16, T), g.bucket(cen))
    cen_d.free(); lab_d.free()
    single = PK.Game(num_players=2, seed=3)
    single.reset()
    for _ in range(8):                                                       # call / check to the flop
        if single._v.turn[0] != 0:
            break
        try:
            single.step(2)
        except (ValueError, AssertionError):
            single.step(1)
    assert single._v.turn[0] == 1
    assert single.bucket(cen) == int(single.equity_hist_hero(centroids=cen).label) < 70
    single.close()
    g.close()


# ---- 9
def test_sixteen_repeated_calls_on_each_stream_form_agree(PK, mixed):
    """A loop of calls with a synchronisation after each: the device form on a caller's stream, the host form on a pooled stream and the
    table form on the handle's stream -- EVERY call must deliver, bit for bit, what the first did, and that is the spec."""
    from pokerl_amd import hipmem
    from pokerl_amd import judger as J
    m, bins = 48, 7
    hero, board, nboard, dead = (x[:m] for x in mixed["spots"])
    weights = mixed["shared"]
    want = rows(mixed["want_shared"], slice(0, m))
    rng = np.random.default_rng(99)
    cen = np.sort(rng.integers(0, 65536, (9, bins)), axis=1).astype(np.uint16)
    cen[:, -1] = 65535
    wlabel, wdist = CS.assign(*CS.quant(want["hist"]), cen)
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0             # hipStreamNonBlocking: a caller's own stream
    ins = [hipmem.DeviceBuffer(x.nbytes).upload(x) for x in (hero, board, nboard, dead, weights, cen)]
    hist_d, void_d, comp_d, status_d, lab_d, dist_d = (hipmem.DeviceBuffer(n) for n in (m * bins * 2, m * 2, m * 4, m, m * 2, m * 4))
    for rep in range(16):
        hist_d.upload(np.full(m * bins, 7, np.uint16))                       # every entry is written: the caller clears nothing
        void_d.upload(np.full(m, 7, np.uint16)); comp_d.upload(np.full(m, 7, np.uint32)); status_d.upload(np.full(m, 7, np.uint8))
        lab_d.upload(np.full(m, 7, np.uint16)); dist_d.upload(np.full(m, 7, np.uint32))
        J.hero_histogram_d(m, *[x.ptr for x in ins[:4]], weights_d=ins[4].ptr, bins=bins, hist_d=hist_d.ptr, void_d=void_d.ptr, completions_d=comp_d.ptr,
                           status_d=status_d.ptr, k=9, centroids_d=ins[5].ptr, label_d=lab_d.ptr, dist_d=dist_d.ptr, stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        assert (hist_d.download(np.uint16, m * bins).reshape(m, bins) == want["hist"]).all(), rep
        assert (void_d.download(np.uint16, m) == want["void"]).all(), rep
        assert (comp_d.download(np.uint32, m) == want["completions"]).all() and not status_d.download(np.uint8, m).any(), rep
        assert (lab_d.download(np.uint16, m) == wlabel).all() and (dist_d.download(np.uint32, m) == wdist).all(), rep
    assert hip.hipStreamDestroy(stream) == 0
    for x in ins + [hist_d, void_d, comp_d, status_d, lab_d, dist_d]:
        x.free()
    for rep in range(16):                                                    # the host form: a pooled stream
        r = J.hero_histogram_batch(hero, board, nboard, dead, weights, bins, cen)
        assert_equal(as_dict(r), want, "host form, call %d" % rep)
        assert np.array_equal(r.label, wlabel) and np.array_equal(r.dist, wdist), rep
    g = PK.VecGame(96, num_players=6, seed=5)                                # the table form: the handle's stream
    g.reset()
    g.rollout(23, policy=0, auto_reset=True, fused=True)
    first = g.equity_hist_hero(weights=weights, bins=bins, centroids=cen)
    assert (first.status == 0).any()
    assert_equal(as_dict(first), explicit_from_getters(g, "active", None, weights, bins), "table form vs explicit form")
    for rep in range(15):
        r = g.equity_hist_hero(weights=weights, bins=bins, centroids=cen)
        assert_equal(as_dict(r), as_dict(first), "table form, call %d" % rep)
        assert np.array_equal(r.label, first.label) and np.array_equal(r.dist, first.dist), rep
    g.close()
