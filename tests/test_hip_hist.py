"""GPU tests of the strength histograms (pk_equity_hist / pk_table_equity_hist: DESIGN.md section 3.5): the fixture from the reference, random
spots against the numpy spec at the smallest pools, around the sort's 64-slot pad and at the full river and turn pools, the river
decomposition on the device (a spot's histogram = the sum over its completions of the one-hot bins of pk_equity_rvr's rows on the completed
river boards) at the full pools and the pad boundaries, batches larger than the persistent grid, bad spots inside good batches, the table
form against the explicit form fed from the getters, and the stream forms.  Every comparison is exact integer equality; the row-sum
invariant is asserted on every device result."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import hist_spec as HS
import rvr_spec as VS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("hist", "void", "completions", "status")
H = HS.HOLDINGS
BINS = (1, 2, 7, 10, 32)


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


def invariants(out):
    """On every spot of every test: for a valid holding the bins and `void` add up to `completions`; nothing at an invalid holding; a
    refused spot all zero."""
    assert out["hist"].dtype == np.uint16 and out["void"].dtype == np.uint16
    total = out["hist"].sum(axis=-1, dtype=np.int64) + out["void"]
    want = np.where(out["valid"], np.asarray(out["completions"], np.int64)[:, None], 0)
    assert (total == want).all(), np.argwhere(total != want)[:4].tolist()
    bad = out["status"] != 0
    assert not out["completions"][bad].any() and not out["valid"][bad].any()
    assert (out["completions"][~bad] > 0).all() and (out["valid"][~bad].sum(axis=1) >= 6).all()


def as_dict(r):
    out = {k: np.asarray(getattr(r, k)) for k in KEYS}
    out["valid"] = np.asarray(r.valid)
    invariants(out)
    return out


def device_hist(board, nboard, dead=None, weights=None, bins=10):
    from pokerl_amd import judger as J
    return as_dict(J.strength_histogram_batch(board, nboard, dead, weights, bins))


def assert_equal(got, want, where, keys=KEYS + ("valid",)):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and (a.astype(np.int64) == b.astype(np.int64)).all(), (where, k, np.argwhere(a.astype(np.int64) != b.astype(np.int64))[:4].tolist())


def rows(d, sel):
    return {k: v[sel] for k, v in d.items()}


def random_weights(rng, shape=(H,)):
    w = rng.integers(0, 65536, shape).astype(np.uint16)
    flat = w.reshape(-1, H)
    for row in flat:
        row[rng.integers(0, H, 300)] = 0
        row[rng.integers(0, H, 100)] = 65535
    return w


def test_every_fixture_spot_equals_the_reference(PK):
    with open(os.path.join(ROOT, "tests", "golden", "hist_ref.json")) as f:
        ref = json.load(f)
    spots = ref["spots"]
    m = len(spots)
    board = np.array([s["board"] + [0] * (5 - len(s["board"])) for s in spots], np.uint8)
    nboard = np.array([len(s["board"]) for s in spots], np.uint8)
    dead = np.array([s["dead"] for s in spots], np.uint64)
    for case in ("ones", "random", "dying"):
        weights = None if case == "ones" else np.stack([HS.fixture_weights(ref, s, case) for s in spots])   # (per spot: the dying range is the spot's own)
        for bins in ref["bins"]:
            exp = [HS.fixture_expected(s, case, bins) for s in spots]
            want = dict(hist=np.stack([e[0] for e in exp]), void=np.stack([e[1] for e in exp]), valid=np.stack([e[2] for e in exp]),
                        completions=np.array([s["completions"] for s in spots]), status=np.zeros(m, np.uint8))
            assert_equal(device_hist(board, nboard, dead, weights, bins), want, "the fixture in one batch, %s, %d bins" % (case, bins))
            if bins == 7:
                for i in range(m):                                # ... and one spot at a time (m = 1: a lone workgroup)
                    w = None if weights is None else weights[i]
                    assert_equal(device_hist(board[i:i + 1], nboard[i:i + 1], dead[i:i + 1], w, bins), rows(want, slice(i, i + 1)), "fixture spot %d alone, %s" % (i, case))
        if case == "dying":
            assert want["void"].any()


# The shapes at which each mechanism can break: the full river and turn pools; on the flop P = 6 (the minimum: one villain per hero and
# completion), 7, 11 and 12 (C(P, 2) = 55 and 66: either side of the 64-slot sort pad), 16.
# river-bounds / turn-bounds: the pools on either side of each size of the sort, npad = 64 | 128 | 256 | 512 | 1 024 | 2 048 by nh = C(P, 2)
# (32 | 33 and 45 | 46 also give a lane its second and third holding); the turn's 45 | 46 in a case of their own (P completions each in the spec).
SHAPES = {"river": (5, (47,)), "turn": (4, (48, 48)), "flop": (3, (6, 7, 11, 12, 16)),
          "river-bounds": (5, (11, 12, 16, 17, 23, 24, 32, 33, 45, 46)), "turn-bounds": (4, (11, 12, 16, 17, 23, 24, 32, 33)), "turn-top": (4, (45, 46))}
RANGES = ("random", "top", "null", "zero")
_spec = {}


def spec_of(name):
    """The spots of a shape, their four ranges, and the spec under every range and number of bins: computed once per run."""
    if name not in _spec:
        nb, pools = SHAPES[name]
        rng = np.random.default_rng(3500 + nb)
        board, nboard, dead = VS.random_boards(rng, len(pools), nb, lambda i: None if pools[i] == 52 - nb else pools[i])
        shared = random_weights(rng)
        ranges = np.stack([shared.astype(np.int64), np.full(H, 65535), np.ones(H, np.int64), np.zeros(H, np.int64)])
        spec = [HS.spot_hist(board[i], nb, dead[i], ranges, BINS) for i in range(len(pools))]   # the pairwise decisions once: four ranges, five bin counts
        _spec[name] = (board, nboard, dead, shared, spec)
    return _spec[name]


@pytest.mark.parametrize("name", ["river", "flop", "turn", "river-bounds", "turn-bounds", "turn-top"])
def test_random_spots_equal_the_spec(PK, name):
    board, nboard, dead, shared, spec = spec_of(name)
    nb, pools = SHAPES[name]
    m, k = len(pools), 5 - nb
    device_weights = dict(random=shared, top=np.full(H, 65535, np.uint16), null=None, zero=np.zeros(H, np.uint16))
    for r, rname in enumerate(RANGES):
        for bins in BINS:
            want = dict(hist=np.stack([s["hist"][bins][r] for s in spec]), void=np.stack([s["void"][r] for s in spec]), valid=np.stack([s["valid"] for s in spec]),
                        completions=np.array([s["completions"] for s in spec]), status=np.zeros(m, np.uint8))
            got = device_hist(board, nboard, dead, device_weights[rname], bins)
            assert_equal(got, want, "%s, %s weights, %d bins" % (name, rname, bins))
            assert got["completions"].tolist() == [math.comb(p - 2, k) for p in pools]
            if rname == "zero":                                   # everything void
                assert not got["hist"].any() and (got["void"][got["valid"]] == np.repeat(got["completions"], got["valid"].sum(axis=1))).all()
            if rname in ("null", "top"):                          # den > 0 by count
                assert not got["void"].any()
    assert_equal(device_hist(board, nboard, dead, np.ones(H, np.uint16), 10), device_hist(board, nboard, dead, None, 10), "NULL weights are all ones")


@pytest.mark.parametrize("nb,pool", [(3, 49), (4, 48), (3, 35), (3, 36), (4, 34), (4, 35)])
def test_river_decomposition_on_the_device(PK, nb, pool):
    """The identity that pins the definition, on the device: hist / void = the host-side sum of the one-hot bins of pk_equity_rvr called once
    on all C(P, k) completed river boards (at most 1 176 spots), the same dead and weights.  The full-pool flop is out of the numpy spec's
    reach; this pins it."""
    from pokerl_amd import judger as J
    rng = np.random.default_rng(100 * nb + pool)
    board, nboard, dead = VS.random_boards(rng, 1, nb, None if pool == 52 - nb else pool)
    weights = np.where(rng.random(H) < 0.5, 0, 65535).astype(np.uint16)                  # zeros and 65 535s
    k = 5 - nb
    rivers, live = HS.river_boards(board[0], nb, dead[0])
    n = len(rivers)
    assert n == math.comb(pool, k) and n <= 1176
    r = J.range_vs_range_batch(rivers, np.full(n, 5, np.uint8), np.full(n, dead[0], np.uint64), weights)
    assert not r.status.any()
    for bins in (10, 32):
        got = device_hist(board, nboard, dead, weights, bins)
        assert got["status"][0] == 0 and got["completions"][0] == math.comb(pool - 2, k) and got["valid"][0].sum() == math.comb(pool, 2)
        hist, void = HS.one_hot_sum(r.win, r.tie, r.tot, live, bins)
        assert np.array_equal(got["hist"][0], hist), (bins, np.argwhere(got["hist"][0] != hist)[:4].tolist())
        assert np.array_equal(got["void"][0], void), (bins, np.argwhere(got["void"][0] != void)[:4].tolist())
        one = J.strength_histogram([int(x) for x in board[0, :nb]], [int(VS.CANON[c]) for c in range(52) if (int(dead[0]) >> c) & 1], weights, bins)
        assert np.array_equal(one.hist, got["hist"][0]) and np.array_equal(one.void, got["void"][0]) and one.completions == got["completions"][0]
        pdf = one.pdf
        counted = one.hist.sum(axis=1) > 0
        assert np.isnan(pdf[~counted]).all() and np.allclose(pdf[counted].sum(axis=1), 1.0) and np.allclose(one.cdf[counted][:, -1], 1.0)
        assert (J.histogram_emd(one.hist[counted], one.hist[counted][0]) >= 0).all()


@pytest.mark.parametrize("m", [1, 65, 600])
def test_batches_of_river_and_turn_spots_equal_the_spec(PK, m):
    """600 spots are more than the persistent grid has workgroups (512): a workgroup takes a second spot with fresh counters.  Per-spot and
    shared weights; every output pointer alone and all of them."""
    from pokerl_amd import _lib as L
    rng = np.random.default_rng(m)
    n_turn = m // 11
    br, nr, dr = VS.random_boards(rng, m - n_turn, 5, lambda i: int(rng.integers(4, 26)))
    bt, nt, dt = VS.random_boards(rng, n_turn, 4, lambda i: int(rng.integers(5, 16)))
    order = rng.permutation(m)
    board, nboard, dead = (np.concatenate(x)[order] for x in ((br, bt), (nr, nt), (dr, dt)))
    weights = random_weights(rng, (m, H))
    weights[:, rng.integers(0, H, 900)] = 0                       # thin ranges: some die on a completion
    bins = 7
    want = HS.batch_hist(board, nboard, dead, weights, bins)
    got = device_hist(board, nboard, dead, weights, bins)
    assert_equal(got, want, "%d river / turn spots, per-spot weights" % m)
    assert m == 1 or got["void"].any()
    assert_equal(device_hist(board, nboard, dead, weights[0], 10), HS.batch_hist(board, nboard, dead, weights[0], 10), "%d river / turn spots, shared weights" % m)
    shapes = dict(hist=(m, H, bins), void=(m, H), completions=(m,), status=(m,))
    dtypes = dict(hist=np.uint16, void=np.uint16, completions=np.uint32, status=np.uint8)
    for only in KEYS:                                             # each output alone
        out = np.full(shapes[only], 7, dtypes[only])
        ptr = {k: (L.ptr(out) if k == only else None) for k in KEYS}
        L.check(L.lib().pk_equity_hist(0, m, L.ptr(board), L.ptr(nboard), L.ptr(dead), L.ptr(weights), 1, bins, ptr["hist"], ptr["void"], ptr["completions"], ptr["status"]))
        assert (out == want[only]).all(), only


def test_bad_spots_inside_a_batch(PK):
    rng = np.random.default_rng(9)
    parts = [VS.random_boards(rng, 16, 5, lambda i: None if i % 4 == 1 else 20), VS.random_boards(rng, 16, 4, lambda i: 34 if i == 3 else 12),
             VS.random_boards(rng, 12, 3, 10)]
    board, nboard, dead = (np.concatenate([p[i] for p in parts]) for i in range(3))
    order = rng.permutation(len(board))
    board, nboard, dead = board[order], nboard[order], dead[order]
    weights = random_weights(rng)
    clean = device_hist(board, nboard, dead, weights, 10)
    assert not clean["status"].any()
    small = np.flatnonzero((clean["valid"].sum(axis=1) <= 190))   # (the spec on the pools of at most 20 cards; the others are pinned elsewhere)
    assert len(small) >= 38
    assert_equal(rows(clean, small), HS.batch_hist(board[small], nboard[small], dead[small], weights, 10), "the clean batch vs spec")
    b, nb, d = board.copy(), nboard.copy(), dead.copy()
    used = lambda i: {VS.canon_index(int(c)) for c in b[i, :nb[i]]}
    want = {}
    b[1, 0] = 0x4F; want[1] = VS.BAD_CARD                                     # a byte that is no card
    b[4, 2] = 0x0D; want[4] = VS.BAD_CARD
    b[7, 1] = 0xFF; want[7] = VS.BAD_CARD                                     # 0xFF in the board
    d[10] |= np.uint64(1) << np.uint64(52); want[10] = VS.BAD_CARD            # a dead bit that is no card
    d[13] = np.uint64(1) << np.uint64(63); want[13] = VS.BAD_CARD
    b[16, 2] = b[16, 0]; want[16] = VS.DUP_CARD                               # a card twice
    d[22] |= np.uint64(1) << np.uint64(VS.canon_index(int(b[22, 0]))); want[22] = VS.DUP_CARD   # a board card that is also dead
    nb[28] = 6; want[28] = VS.BAD_NBOARD
    nb[31] = 255; want[31] = VS.BAD_NBOARD
    nb[33] = 0; want[33] = VS.PREFLOP
    nb[37] = 2; want[37] = VS.PREFLOP
    for i, n in ((39, 5), (41, 4), (43, 3)):                                  # P = k + 3: one card short of the board to come and two holdings
        nb[i] = n
        free = [c for c in range(52) if c not in used(i)]
        d[i] = sum(1 << c for c in free[(5 - n) + 3:])
        want[i] = VS.SMALL_POOL
    got = device_hist(b, nb, d, weights, 10)
    assert got["status"].tolist() == [VS.check_spot(b[i], nb[i], d[i])[0] for i in range(len(b))]
    from pokerl_amd import judger as J
    assert got["status"].tolist() == J.range_vs_range_batch(b, nb, d, weights).status.tolist()   # the same spot, the same status from both families
    for i in range(len(b)):
        if i in want:
            assert got["status"][i] == want[i] and not got["hist"][i].any() and not got["void"][i].any() and got["completions"][i] == 0, i
        else:
            assert_equal(rows(got, slice(i, i + 1)), rows(clean, slice(i, i + 1)), "neighbour %d" % i)


def explicit_from_getters(g, tables=None, weights=None, bins=10):
    board, nboard = VS.table_boards(g.deck, g.turn)
    if tables is not None:
        board, nboard = board[tables], nboard[tables]
    return device_hist(board, nboard, None, weights, bins)


@pytest.mark.parametrize("n,steps", [(2, 9), (6, 37), (16, 61)])
def test_table_form_equals_explicit_form(PK, n, steps):
    T = 165
    g = PK.VecGame(T, num_players=n, seed=91 + n)
    g.reset()
    g.rollout(steps, policy=0, auto_reset=True, fused=True)
    turn = g.turn
    # every turn a table can rest at: 0 (pre-flop, refused), 1, 2, 3 = flop, turn, river
    assert set(turn.tolist()) == {0, 1, 2, 3}, sorted(set(turn.tolist()))
    before = g.save()
    pre = turn == 0
    rng = np.random.default_rng(n)
    weights = random_weights(rng)
    want = explicit_from_getters(g, weights=weights)
    assert (want["status"][pre] == VS.PREFLOP).all() and not want["status"][~pre].any()
    got = as_dict(g.equity_hist(weights=weights))
    assert_equal(got, want, "table form %dx%d" % (T, n))
    assert set(got["completions"][~pre].tolist()) == {1, 46, 1081}
    pick = np.concatenate([rng.permutation(T)[:20], [5, 5, 5, T - 1, 0]]).astype(np.int32)   # permuted, repeated indices
    got = as_dict(g.equity_hist(weights=weights, tables=pick, bins=32))
    assert_equal(got, rows(explicit_from_getters(g, weights=weights, bins=32), pick), "table form %dx%d, index array, 32 bins" % (T, n))
    r = g.equity_hist(tables=np.array([int(pick[0]), T, -1, 2 ** 31 - 1], np.int64), bins=3)
    assert r.status[1:].tolist() == [VS.BAD_TABLE] * 3 and not r.completions[1:].any() and not r.hist[1:].any() and not r.void[1:].any()
    assert r.status[0] == want["status"][pick[0]] and r.completions[0] == want["completions"][pick[0]] and r.hist.shape == (4, H, 3)
    assert g.save().tobytes() == before.tobytes()                            # the calls wrote nothing to the handle
    g.close()


def test_never_dealt_handle_and_the_single_game(PK):
    g = PK.VecGame(64, num_players=6)
    r = g.equity_hist()
    assert (r.status == VS.PREFLOP).all() and not r.hist.any() and not r.void.any() and not r.completions.any()   # turn 0: nothing is read
    assert r.hist.shape == (64, H, 10)
    g.close()
    single = PK.Game(num_players=3)
    with pytest.raises(ValueError, match="fewer than three board cards"):
        single.equity_hist()                                                 # never dealt
    single.reset()
    with pytest.raises(ValueError, match="fewer than three board cards"):
        single.equity_hist(bins=4)                                           # pre-flop
    with pytest.raises(ValueError, match="bins"):
        single.equity_hist(bins=33)
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
    e = g.equity_hist()
    assert e.valid is None or not e.valid.any()                              # (no mask while steps are in flight: the getters it is formed from refuse)
    r = {k: np.asarray(getattr(e, k)) for k in KEYS}
    assert ((r["status"][~idle] & VS.IN_FLIGHT) != 0).all() and not (r["status"][idle] & VS.IN_FLIGHT).any()
    assert not r["hist"][~idle].any() and not r["void"][~idle].any() and not r["completions"][~idle].any()
    act.upload(np.full(T, -1, np.int32))                                     # the drain: idle tables get no step and stay as they are
    g.step_async_d(act, flags, terr, ready, max_hands=0, auto_reset=True)
    g.sync()
    t = np.flatnonzero(idle)
    assert_equal(rows(r, t), explicit_from_getters(g, t), "the idle tables", KEYS)
    for b in (act, flags, terr, ready):
        b.free()
    g.close()


def test_sixteen_repeated_calls_on_each_stream_form_agree(PK):
    """A loop of calls with a synchronisation after each: the device form on a caller's stream, the host form on a pooled stream and the
    table form on the handle's stream -- EVERY call must deliver, bit for bit what the first did, and that is the spec."""
    from pokerl_amd import hipmem
    from pokerl_amd import judger as J
    rng = np.random.default_rng(77)
    m, bins = 48, 10
    br, nr, dr = VS.random_boards(rng, m - 8, 5, lambda i: int(rng.integers(4, 30)))
    bt, nt, dt = VS.random_boards(rng, 8, 4, lambda i: int(rng.integers(5, 14)))
    board, nboard, dead = (np.concatenate(x) for x in ((br, bt), (nr, nt), (dr, dt)))
    weights = random_weights(rng)
    want = HS.batch_hist(board, nboard, dead, weights, bins)
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0             # hipStreamNonBlocking: a caller's own stream
    ins = [hipmem.DeviceBuffer(x.nbytes).upload(x) for x in (board, nboard, dead, weights)]
    hist_d, void_d, comp_d, status_d = hipmem.DeviceBuffer(m * H * bins * 2), hipmem.DeviceBuffer(m * H * 2), hipmem.DeviceBuffer(m * 4), hipmem.DeviceBuffer(m)
    for rep in range(16):
        hist_d.upload(np.full(m * H * bins, 7, np.uint16))                   # every entry is written: the caller clears nothing
        void_d.upload(np.full(m * H, 7, np.uint16))
        comp_d.upload(np.full(m, 7, np.uint32))
        status_d.upload(np.full(m, 7, np.uint8))
        J.strength_histogram_d(m, *[x.ptr for x in ins[:3]], weights_d=ins[3].ptr, bins=bins, hist_d=hist_d.ptr, void_d=void_d.ptr,
                               completions_d=comp_d.ptr, status_d=status_d.ptr, stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        assert (hist_d.download(np.uint16, m * H * bins).reshape(m, H, bins) == want["hist"]).all(), rep
        assert (void_d.download(np.uint16, m * H).reshape(m, H) == want["void"]).all(), rep
        assert (comp_d.download(np.uint32, m) == want["completions"]).all() and not status_d.download(np.uint8, m).any(), rep
    assert hip.hipStreamDestroy(stream) == 0
    for x in ins + [hist_d, void_d, comp_d, status_d]:
        x.free()
    for rep in range(16):                                                    # the host form: a pooled stream
        assert_equal(device_hist(board, nboard, dead, weights, bins), want, "host form, call %d" % rep)
    g = PK.VecGame(96, num_players=6, seed=5)                                # the table form: the handle's stream
    g.reset()
    g.rollout(23, policy=0, auto_reset=True, fused=True)
    first = as_dict(g.equity_hist(weights=weights, bins=bins))
    assert (first["status"] == 0).any()
    assert_equal(first, explicit_from_getters(g, weights=weights, bins=bins), "table form vs explicit form")
    for rep in range(15):
        assert_equal(as_dict(g.equity_hist(weights=weights, bins=bins)), first, "table form, call %d" % rep)
    g.close()
