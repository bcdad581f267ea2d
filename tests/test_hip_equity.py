"""GPU tests of the showdown equity through the C ABI (pk_equity(_d), pk_table_equity(_d)): exact equality with the reference's fixture
and with the numpy restatement of the definition (tests/equity_spec.py), both regimes (one task per spot / a spot cut into many tasks), the
table form against the explicit form fed from the getters, bad spots inside good batches, repeatability and the stream forms."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import equity_spec as ES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("win", "tie", "share", "boards", "status")


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


def device_equity(holes, board, nboard, live):
    from pokerl_amd import judger as J
    r = J.showdown_equity_batch(holes, board, nboard, live)
    out = {k: getattr(r, k) for k in KEYS}
    invariants(out)
    return out


def invariants(out):
    """On every spot of every test: the shares add up to the boards exactly, win + tie <= boards, a refused spot is all zero."""
    share = out["share"].astype(object).sum(axis=1)
    boards = out["boards"].astype(object)
    ok = out["status"] == 0
    assert all(int(s) == ES.SHARE_UNIT * int(b) for s, b in zip(share[ok], boards[ok]))
    assert ((out["win"].astype(np.int64) + out["tie"]) <= out["boards"].astype(np.int64)[:, None]).all()
    bad = ~ok
    assert not out["win"][bad].any() and not out["tie"][bad].any() and not out["share"][bad].any() and not out["boards"][bad].any()
    assert (out["boards"][ok] > 0).all()


def assert_equal(got, want, where):
    for k in KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and (a.astype(np.uint64) == b.astype(np.uint64)).all(), (where, k, np.argwhere(a.astype(np.uint64) != b.astype(np.uint64))[:4].tolist())


def test_every_fixture_spot_equals_the_reference(PK):
    with open(os.path.join(ROOT, "tests", "golden", "equity_ref.json")) as f:
        spots = json.load(f)["spots"]
    for n in sorted({s["n"] for s in spots}):
        group = [s for s in spots if s["n"] == n]
        holes = np.array([s["holes"] for s in group], np.uint8)
        board = np.array([s["board"] + [0] * (5 - len(s["board"])) for s in group], np.uint8)
        nboard = np.array([len(s["board"]) for s in group], np.uint8)
        live = np.array([s["live"] for s in group], np.uint16)
        got = device_equity(holes, board, nboard, live)
        want = dict(win=np.array([s["win"] for s in group]), tie=np.array([s["tie"] for s in group]), share=np.array([s["share"] for s in group], np.uint64),
                    boards=np.array([s["boards"] for s in group]), status=np.zeros(len(group), np.uint8))
        assert_equal(got, want, "fixture n=%d" % n)
        for s, g in zip(group, range(len(group))):              # ... and one spot at a time (m = 1: the finest split)
            one = device_equity(holes[g:g + 1], board[g:g + 1], nboard[g:g + 1], live[g:g + 1])
            assert_equal(one, {k: want[k][g:g + 1] for k in KEYS}, "fixture n=%d spot %d alone" % (n, g))


@pytest.mark.parametrize("n", [2, 3, 6, 9, 10, 16])
def test_random_spots_equal_the_spec(PK, n):
    rng = np.random.default_rng(1000 + n)
    parts = [ES.random_spots(rng, n, 6, nb=nb) for nb in (5, 4, 3)]
    parts += [ES.random_spots(rng, n, 2, nb=2), ES.random_spots(rng, n, 1, nb=1)]      # 2 and 1 known board cards: up to C(46, 4) boards
    if n in (2, 6):
        parts.append(ES.random_spots(rng, n, 2 if n == 2 else 1, nb=0))                # pre-flop: only where the spec stays cheap
    holes, board, nboard, live = (np.concatenate([p[i] for p in parts]) for i in range(4))
    assert_equal(device_equity(holes, board, nboard, live), ES.batch_equity(holes, board, nboard, live), "random n=%d" % n)


def test_aa_v_kk_preflop(PK):
    """1 712 304 boards: the spot is cut into many tasks whose counts are added up in the outputs."""
    from pokerl_amd import judger as J
    r = J.showdown_equity([["AS", "AD"], ["KS", "KD"]])
    assert r.boards == 1712304 and r.status == 0
    hu = np.array([[J.card_value(c) for c in h] for h in (["AS", "AD"], ["KS", "KD"])], np.uint8)
    want = ES.spot_equity(hu, [0] * 5, 0, 0b11)
    assert_equal({k: np.asarray(getattr(r, k))[None] for k in KEYS}, {k: np.asarray(want[k])[None] for k in KEYS}, "AA v KK")
    assert int(r.share.astype(object).sum()) == ES.SHARE_UNIT * 1712304
    assert 0.81 < r.equity[0] < 0.83                       # (a sanity look at the number everyone knows; the equality above is the test)
    # the same spot in a large batch takes the coarse split, and with a folded third seat the pool shrinks
    many = J.showdown_equity_batch(np.tile(hu[None], (300, 1, 1)), np.zeros((300, 5), np.uint8),
                                   np.zeros(300, np.uint8), np.full(300, 3, np.uint16))
    for k in ("win", "tie", "share"):
        assert (getattr(many, k) == np.asarray(want[k])[None]).all(), k
    assert (many.boards == 1712304).all() and not many.status.any()


def test_river_equals_compare_hands_and_a_lone_seat_wins_everything(PK):
    from pokerl_amd import judger as J
    rng = np.random.default_rng(5)
    for n in (2, 3, 6, 9, 16):
        holes, board, nboard, live = ES.random_spots(rng, n, 8, nb=5, unknown=False)
        live[:] = (1 << n) - 1
        got = device_equity(holes, board, nboard, live)
        for i in range(8):
            onehot, winners, _ = PK.compare_hands([list(board[i]) + list(holes[i, p]) for p in range(n)])
            assert got["boards"][i] == 1
            assert (got["win"][i] + got["tie"][i]).tolist() == onehot, (n, i)
            assert got["share"][i].tolist() == [ES.SHARE_UNIT // len(winners) * x for x in onehot]
        for nb in (5, 4, 3, 0):
            holes, board, nboard, live = ES.random_spots(rng, n, 2, nb=nb)
            seat = [int(np.flatnonzero([(int(m) >> p) & 1 for p in range(n)])[0]) for m in live]
            live = np.array([1 << s for s in seat], np.uint16)
            got = device_equity(holes, board, nboard, live)
            for i, s in enumerate(seat):
                assert got["win"][i, s] == got["boards"][i] and got["win"][i].sum() == got["boards"][i] and not got["tie"][i].any()


def explicit_from_getters(g, tables=None):
    holes, board, nboard, live = ES.table_spots(g.deck, g.player_states, g.turn)
    if tables is not None:
        holes, board, nboard, live = holes[tables], board[tables], nboard[tables], live[tables]
    return device_equity(holes, board, nboard, live)


@pytest.mark.parametrize("tables,n,steps", [(65536, 6, 37), (4096, 2, 11), (1500, 9, 53), (300, 16, 29)])
def test_table_form_equals_explicit_form(PK, tables, n, steps):
    """The WHOLE batch, pre-flop tables included, both ways through the device: without an index array (tables = NULL: spot i is table i)
    and with one (permuted, repeated indices), against the explicit form fed from the getters.  At 65 536 x 6 a call holds several
    hundred thousand tasks, so the wavefronts take them in runs of four."""
    g = PK.VecGame(tables, num_players=n, seed=77 + n)
    g.reset()
    g.rollout(steps, policy=0, auto_reset=True, fused=True)
    turn = g.turn
    assert len(set(turn.tolist())) >= 3
    before = g.save()
    want = explicit_from_getters(g)
    assert not want["status"].any() and len(want["boards"]) == tables
    r = g.equity()                                                           # tables = NULL, m = T
    got = {k: getattr(r, k) for k in KEYS}
    invariants(got)
    assert_equal(got, want, "table form %dx%d, no index array" % (tables, n))
    rng = np.random.default_rng(n)
    perm = rng.permutation(tables)[:max(tables // 8, 200)]
    perm = np.concatenate([perm, perm[:50], perm[:1]]).astype(np.int32)      # permuted, repeated indices
    r2 = g.equity(perm)
    assert_equal({k: getattr(r2, k) for k in KEYS}, {k: want[k][perm] for k in KEYS}, "table form %dx%d, index array" % (tables, n))
    m = tables // 3                                                          # tables = NULL with m < T: the first m tables
    from pokerl_amd import _lib as L
    win, tie = np.zeros((m, n), np.uint32), np.zeros((m, n), np.uint32)
    share, boards, status = np.zeros((m, n), np.uint64), np.zeros(m, np.uint32), np.zeros(m, np.uint8)
    L.check(g._lib.pk_table_equity(g._h, None, m, L.ptr(win), L.ptr(tie), L.ptr(share), L.ptr(boards), L.ptr(status)), g._h)
    assert_equal(dict(win=win, tie=tie, share=share, boards=boards, status=status), {k: want[k][:m] for k in KEYS}, "tables = NULL, m < T")
    assert g.save().tobytes() == before.tobytes()                            # the calls wrote nothing to the handle
    g.close()


def test_large_narrow_batch_equals_the_spec(PK):
    """70 000 flop / turn / river spots in ONE explicit call (one task each; more than eight per resident wavefront, so they are taken in
    runs of four): every spot is one of 700 distinct ones, each of which is checked against the spec, in a shuffled order."""
    rng = np.random.default_rng(71)
    n, distinct, m = 6, 700, 70000
    holes, board, nboard, live = ES.random_spots(rng, n, distinct)
    nboard[:] = rng.integers(3, 6, distinct)
    want = ES.batch_equity(holes, board, nboard, live)
    pick = rng.integers(0, distinct, m)
    pick[:distinct] = np.arange(distinct)
    got = device_equity(holes[pick], board[pick], nboard[pick], live[pick])
    assert_equal(got, {k: want[k][pick] for k in KEYS}, "70 000 narrow spots")


def test_never_reset_handle_and_bad_indices_report_a_status(PK):
    g = PK.VecGame(64, num_players=6)
    r = g.equity()
    assert (r.status == ES.DUP_CARD).all() and not r.win.any() and not r.boards.any()
    g.reset()
    r = g.equity(np.array([0, 64, -1, 5, 2 ** 31 - 1], np.int64))
    assert r.status.tolist() == [0, ES.BAD_TABLE, ES.BAD_TABLE, 0, ES.BAD_TABLE]
    assert r.boards[0] == r.boards[3] > 0 and not r.win[[1, 2, 4]].any()
    single = PK.Game(num_players=3)
    with pytest.raises(ValueError):
        single.equity()
    single.reset()
    e = single.equity()
    assert e.status == 0 and e.boards == 46 * 45 * 44 * 43 * 42 // 120 and int(e.share.astype(object).sum()) == ES.SHARE_UNIT * int(e.boards)
    single.close()
    g.close()


def test_bad_spots_inside_a_batch(PK):
    rng = np.random.default_rng(9)
    n = 6
    holes, board, nboard, live = ES.random_spots(rng, n, 40, unknown=False)
    nboard[:] = rng.integers(3, 6, 40)
    live[:] |= 1
    clean = device_equity(holes, board, nboard, live)
    assert not clean["status"].any()
    h, b, nb, lv = holes.copy(), board.copy(), nboard.copy(), live.copy()
    want = {}
    h[3, 0, 0] = 0x4F; want[3] = ES.BAD_CARD                                 # a byte that is no card
    h[7, 0] = ES.UNKNOWN; want[7] = ES.BAD_CARD                              # unknown at a live seat
    nb[11] = 5; b[11, 2] = ES.UNKNOWN; want[11] = ES.BAD_CARD                # unknown in the board
    nb[15] = 5; b[15, 4] = h[15, 2, 1]; want[15] = ES.DUP_CARD               # a card twice
    lv[19] = 0; want[19] = ES.NO_LIVE
    nb[23] = 6; want[23] = ES.BAD_NBOARD
    nb[27] = 200; lv[27] = 0; want[27] = ES.BAD_NBOARD | ES.NO_LIVE
    lv[31] = 0xFFC0; want[31] = ES.NO_LIVE                                   # only seats >= N: ignored bits
    h[35, 1, 1] = h[35, 1, 0]; want[35] = ES.DUP_CARD
    got = device_equity(h, b, nb, lv)
    assert_equal(got, ES.batch_equity(h, b, nb, lv), "bad spots vs spec")
    for i in range(40):
        if i in want:
            assert got["status"][i] == want[i], i
        else:
            assert_equal({k: got[k][i:i + 1] for k in KEYS}, {k: clean[k][i:i + 1] for k in KEYS}, "neighbour %d" % i)


def test_repeatable_and_stream_forms_agree(PK):
    from pokerl_amd import _lib as L, hipmem
    from pokerl_amd import judger as J
    rng = np.random.default_rng(21)
    n, m = 6, 200
    holes, board, nboard, live = ES.random_spots(rng, n, m)
    nboard[:] = rng.integers(2, 6, m)
    nboard[:3] = 0                                                            # three pre-flop spots among them
    live[:3] = 0b11
    holes[:3, :2] = np.where(holes[:3, :2] == ES.UNKNOWN, 0, holes[:3, :2])
    holes[:3] = ES.random_spots(rng, n, 3, unknown=False)[0]
    for i in range(3):
        board[i] = 0
    a = device_equity(holes, board, nboard, live)
    assert_equal(device_equity(holes, board, nboard, live), a, "same inputs twice")
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0             # hipStreamNonBlocking: a caller's own stream
    ins = [hipmem.DeviceBuffer(x.nbytes).upload(x) for x in (holes, board, nboard, live)]
    outs = [hipmem.DeviceBuffer(m * n * 4), hipmem.DeviceBuffer(m * n * 4), hipmem.DeviceBuffer(m * n * 8), hipmem.DeviceBuffer(m * 4), hipmem.DeviceBuffer(m)]
    for rep in range(2):
        J.showdown_equity_d(n, m, *[x.ptr for x in ins], *[x.ptr for x in outs], stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        d = dict(win=outs[0].download(np.uint32, m * n).reshape(m, n), tie=outs[1].download(np.uint32, m * n).reshape(m, n),
                 share=outs[2].download(np.uint64, m * n).reshape(m, n), boards=outs[3].download(np.uint32, m), status=outs[4].download(np.uint8, m))
        assert_equal(d, a, "device form on a caller's stream, pass %d" % rep)
    # only some outputs wanted
    J.showdown_equity_d(n, m, *[x.ptr for x in ins], None, None, outs[2].ptr, None, None, stream=stream)
    assert hip.hipStreamSynchronize(stream) == 0
    assert (outs[2].download(np.uint64, m * n).reshape(m, n) == a["share"]).all()
    for x in ins + outs:
        x.free()
    # a loop of calls with a synchronisation after each, at a size whose work space exceeds a megabyte: EVERY call must deliver
    # (the device form once took its work space from the stream-ordered allocator, and every third call of this loop came back all zero)
    m2 = 4096
    h2 = np.tile(np.array([[[0x00, 0x10], [0x0C, 0x1C]]], np.uint8), (m2, 1, 1))
    ins = [hipmem.DeviceBuffer(x.nbytes).upload(x) for x in (h2, np.zeros((m2, 5), np.uint8), np.zeros(m2, np.uint8), np.full(m2, 3, np.uint16))]
    outs = [hipmem.DeviceBuffer(m2 * 2 * 4), hipmem.DeviceBuffer(m2 * 2 * 4), hipmem.DeviceBuffer(m2 * 2 * 8), hipmem.DeviceBuffer(m2 * 4), hipmem.DeviceBuffer(m2)]
    one = ES.spot_equity(h2[0], [0] * 5, 0, 3)
    for rep in range(7):
        outs[0].upload(np.full(m2 * 2, 7, np.uint32))
        outs[2].upload(np.full(m2 * 2, 7, np.uint64))
        J.showdown_equity_d(2, m2, *[x.ptr for x in ins], *[x.ptr for x in outs], stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        assert (outs[0].download(np.uint32, m2 * 2).reshape(m2, 2) == one["win"][None]).all(), rep
        assert (outs[2].download(np.uint64, m2 * 2).reshape(m2, 2) == one["share"][None]).all(), rep
        assert (outs[3].download(np.uint32, m2) == one["boards"]).all() and not outs[4].download(np.uint8, m2).any(), rep
    assert hip.hipStreamDestroy(stream) == 0
    for x in ins + outs:
        x.free()


def test_mixed_batch_exercises_both_regimes(PK):
    rng = np.random.default_rng(33)
    n = 2
    holes, board, nboard, live = ES.random_spots(rng, n, 21, nb=5, unknown=False)
    live[:] = 3
    nboard[10] = 0                                                            # a pre-flop spot between river spots
    nboard[4] = 3
    nboard[16] = 4
    got = device_equity(holes, board, nboard, live)
    assert got["boards"][10] == 1712304 and got["boards"][9] == 1 and got["boards"][4] == 990 and got["boards"][16] == 44
    assert_equal(got, ES.batch_equity(holes, board, nboard, live), "mixed batch")
    # ... and at a batch size that takes the coarse split
    reps = 14
    big = device_equity(np.tile(holes, (reps, 1, 1)), np.tile(board, (reps, 1)), np.tile(nboard, reps), np.tile(live, reps))
    assert_equal(big, {k: np.tile(got[k], (reps, 1) if got[k].ndim == 2 else reps) for k in KEYS}, "mixed batch x %d" % reps)
