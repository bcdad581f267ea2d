"""GPU tests of range vs range (pk_equity_rvr / pk_table_equity_rvr: DESIGN.md section 3.4): the fixture from the reference, random spots
against the numpy spec at the pools around the sort's edges, the identity with the existing exact call (row h = pk_equity_range of hero h) at
the full pools, batches larger than the persistent grid, bad spots inside good batches, the table form against the explicit form fed from
the getters, the stream forms, and the sampled call on the same board."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import rvr_spec as VS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("win", "tie", "tot", "boards", "status")
H = VS.HOLDINGS


@pytest.fixture(scope="module")
def PK():
    import pokerl_amd
    assert pokerl_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot run (there is no fallback)"
    return pokerl_amd


def invariants(out):
    """On every spot of every test: win + tie <= tot, nothing at an invalid holding, a refused spot all zero."""
    assert (out["win"] + out["tie"] <= out["tot"]).all()
    for k in ("win", "tie", "tot"):
        assert out[k].dtype == np.uint64 and not out[k][~out["valid"]].any()
    bad = out["status"] != 0
    assert not out["boards"][bad].any() and not out["valid"][bad].any()
    assert (out["boards"][~bad] > 0).all() and (out["valid"][~bad].sum(axis=1) >= 6).all()


def as_dict(r):
    out = {k: np.asarray(getattr(r, k)) for k in KEYS}
    out["valid"] = np.asarray(r.valid)
    invariants(out)
    return out


def device_rvr(board, nboard, dead=None, weights=None):
    from pokerl_amd import judger as J
    return as_dict(J.range_vs_range_batch(board, nboard, dead, weights))


def assert_equal(got, want, where, keys=KEYS + ("valid",)):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and (a.astype(np.uint64) == b.astype(np.uint64)).all(), (where, k, np.argwhere(a.astype(np.uint64) != b.astype(np.uint64))[:4].tolist())


def rows(d, sel):
    return {k: v[sel] for k, v in d.items()}


def random_weights(rng, shape=(H,)):
    w = rng.integers(0, 65536, shape).astype(np.uint16)
    flat = w.reshape(-1, H)
    for row in flat:
        row[rng.integers(0, H, 200)] = 0
        row[rng.integers(0, H, 100)] = 65535
    return w


def test_every_fixture_spot_equals_the_reference(PK):
    with open(os.path.join(ROOT, "tests", "golden", "rvr_ref.json")) as f:
        ref = json.load(f)
    spots = ref["spots"]
    m = len(spots)
    board = np.array([s["board"] + [0] * (5 - len(s["board"])) for s in spots], np.uint8)
    nboard = np.array([len(s["board"]) for s in spots], np.uint8)
    dead = np.array([s["dead"] for s in spots], np.uint64)
    for suffix, weights in (("", None), ("_w", np.array(ref["weights"], np.uint16))):
        want = dict(win=np.zeros((m, H), np.uint64), tie=np.zeros((m, H), np.uint64), tot=np.zeros((m, H), np.uint64), valid=np.zeros((m, H), bool),
                    boards=np.array([s["boards"] for s in spots]), status=np.zeros(m, np.uint8))
        for i, s in enumerate(spots):
            want["valid"][i, s["h"]] = True
            for k in ("win", "tie", "tot"):
                want[k][i, s["h"]] = s[k + suffix]
        assert_equal(device_rvr(board, nboard, dead, weights), want, "the fixture in one batch" + suffix)
        for i in range(m):                                        # ... and one spot at a time (m = 1: a lone workgroup)
            assert_equal(device_rvr(board[i:i + 1], nboard[i:i + 1], dead[i:i + 1], weights), rows(want, slice(i, i + 1)), "fixture spot %d alone%s" % (i, suffix))


# Pools by the number n = C(P - k, 2) of holdings one completion leaves in play: the smallest pools (n = 6, 10) and the pools around the
# sort's edges -- n = 496, 528, 561 about 512 and 990, 1 035, 1 081 about 1 024 -- where the padded sort size and the number of holdings and
# sorted positions a lane serves change.  The sort itself is padded by the POOL's holdings nh = C(P, 2): P = 11 | 12, 16 | 17, 23 | 24, 32 | 33,
# 45 | 46 lie across npad = 64 | 128 | 256 | 512 | 1 024 | 2 048 -- on the river (rest = P) every pair, on the turn (rest = P - 1) the pairs up to
# 32 | 33 twice each, and 45 | 46 once each in a case of their own ("4-top": 45 completions of 900 000 pairwise decisions each in the spec).
REST = {5: (4, 5, 11, 12, 16, 17, 23, 24, 32, 33, 34, 45, 46, 47), 4: (4, 5, 10, 11, 15, 16, 22, 23, 31, 32, 33), 3: (4, 5, 11, 12)}


@pytest.mark.parametrize("nb,rests,each", [(5, REST[5], 2), (4, REST[4], 2), (3, REST[3], 2), (4, (44, 45), 1)], ids=["5", "4", "3", "4-top"])
def test_random_spots_equal_the_spec(PK, nb, rests, each):
    rng = np.random.default_rng(3000 + nb)
    k = 5 - nb
    pools = [rest + k for rest in rests for _ in range(each)]
    m = len(pools)
    board, nboard, dead = VS.random_boards(rng, m, nb, lambda i: pools[i])
    shared = random_weights(rng)
    ranges = np.stack([shared.astype(np.int64), np.full(H, 65535), np.ones(H, np.int64)])
    spec = [VS.spot_rvr(board[i], nb, dead[i], ranges) for i in range(m)]              # the pairwise decisions once, three ranges
    want = lambda r: dict(win=np.stack([s["win"][r] for s in spec]), tie=np.stack([s["tie"][r] for s in spec]), tot=np.stack([s["tot"][r] for s in spec]),
                          valid=np.stack([s["valid"] for s in spec]), boards=np.array([s["boards"] for s in spec]), status=np.zeros(m, np.uint8))
    assert_equal(device_rvr(board, nboard, dead, shared), want(0), "random nb=%d, random weights" % nb)
    top = device_rvr(board, nboard, dead, np.full(H, 65535, np.uint16))
    assert_equal(top, want(1), "random nb=%d, every weight 65 535" % nb)
    none = device_rvr(board, nboard, dead)
    assert_equal(none, want(2), "random nb=%d, NULL weights" % nb)
    assert_equal(device_rvr(board, nboard, dead, np.ones(H, np.uint16)), none, "NULL weights are all ones")
    if rests[0] == 4:
        assert none["valid"][:2].sum(axis=1).tolist() == [math.comb(k + 4, 2)] * 2 and none["boards"][:2].tolist() == [1, 1]   # the smallest pool
        assert (none["tot"][:2][none["valid"][:2]] == math.comb(k + 2, 2)).all()
    if nb == 5:                                                   # the largest value there is on a river: 65 535 * 990 per holding
        assert (top["tot"][-1][top["valid"][-1]] == 65535 * 990).all()


def spot_boards(rng, nb, pool):
    return VS.random_boards(rng, 1, nb, pool)


@pytest.mark.parametrize("nb,pool", [(5, None), (4, None), (3, None), (3, 35), (3, 36), (3, 48), (4, 34), (4, 35), (4, 47)])
def test_rows_equal_the_range_equity_of_every_hero(PK, nb, pool):
    """The identity that pins the definition, on the device: row h = pk_equity_range's agg for hero = HOLDINGS[h], for EVERY valid h.  The
    full pools (P = 47 / 48 / 49) are out of the spec's reach on the flop: 1 176 x 1 081^2 pairs."""
    from pokerl_amd import judger as J
    rng = np.random.default_rng(100 * nb + (pool or 0))
    board, nboard, dead = spot_boards(rng, nb, pool)
    weights = random_weights(rng)
    k = 5 - nb
    P = 52 - nb if pool is None else pool
    r = as_dict(J.range_vs_range_batch(board, nboard, dead, weights))
    assert r["status"][0] == 0 and r["boards"][0] == math.comb(P - 4, k)
    hs = np.flatnonzero(r["valid"][0])
    assert len(hs) == P * (P - 1) // 2
    n = len(hs)
    e = J.range_equity_batch(PK.HOLDINGS[hs], np.tile(board, (n, 1)), np.full(n, nb, np.uint8), np.full(n, dead[0], np.uint64), weights, per_holding=False)
    assert not e.status.any() and (e.boards == math.comb(P - 4, k)).all()
    got = np.stack([r["win"][0, hs], r["tie"][0, hs], r["tot"][0, hs]], axis=1)
    assert (got == e.agg).all(), np.argwhere(got != e.agg)[:4].tolist()
    invalid = np.ones(H, bool)
    invalid[hs] = False
    assert not r["win"][0, invalid].any() and not r["tie"][0, invalid].any() and not r["tot"][0, invalid].any()
    one = J.range_vs_range([int(x) for x in board[0, :nb]], [int(VS.CANON[c]) for c in range(52) if (int(dead[0]) >> c) & 1], weights)
    assert np.array_equal(one.win, r["win"][0]) and np.array_equal(one.tot, r["tot"][0]) and one.boards == r["boards"][0]
    s = one.strength
    assert np.isnan(s[invalid]).all() and ((s[hs] >= 0) & (s[hs] <= 1)).all() and 0.0 <= one.against(weights) <= 1.0


@pytest.mark.parametrize("m", [1, 65, 1100])
def test_batches_of_river_and_turn_spots_equal_the_spec(PK, m):
    """1 100 spots are more than the persistent grid has workgroups (512): a workgroup takes a second spot with fresh accumulators.  Per-spot
    weights; every output pointer alone and all of them."""
    from pokerl_amd import _lib as L
    rng = np.random.default_rng(m)
    n_turn = m // 11
    br, nr, dr = VS.random_boards(rng, m - n_turn, 5, lambda i: int(rng.integers(4, 26)))
    bt, nt, dt = VS.random_boards(rng, n_turn, 4, lambda i: int(rng.integers(5, 16)))
    order = rng.permutation(m)
    board, nboard, dead = (np.concatenate(x)[order] for x in ((br, bt), (nr, nt), (dr, dt)))
    weights = random_weights(rng, (m, H))
    want = VS.batch_rvr(board, nboard, dead, weights)
    got = device_rvr(board, nboard, dead, weights)
    assert_equal(got, want, "%d river / turn spots" % m)
    dtypes = dict(win=np.uint64, tie=np.uint64, tot=np.uint64, boards=np.uint32, status=np.uint8)
    for only in KEYS:                                             # each output alone
        out = np.full((m, H) if dtypes[only] == np.uint64 else (m,), 7, dtypes[only])
        ptr = {k: (L.ptr(out) if k == only else None) for k in KEYS}
        L.check(L.lib().pk_equity_rvr(0, m, L.ptr(board), L.ptr(nboard), L.ptr(dead), L.ptr(weights), 1, ptr["win"], ptr["tie"], ptr["tot"], ptr["boards"], ptr["status"]))
        assert (out == want[only]).all(), only


def test_bad_spots_inside_a_batch(PK):
    rng = np.random.default_rng(9)
    parts = [VS.random_boards(rng, 16, 5, lambda i: None if i % 4 == 1 else 20), VS.random_boards(rng, 16, 4, lambda i: 34 if i == 3 else 12),
             VS.random_boards(rng, 12, 3, 10)]
    board, nboard, dead = (np.concatenate([p[i] for p in parts]) for i in range(3))
    order = rng.permutation(len(board))
    board, nboard, dead = board[order], nboard[order], dead[order]
    weights = random_weights(rng)
    clean = device_rvr(board, nboard, dead, weights)
    assert not clean["status"].any()
    assert_equal(clean, VS.batch_rvr(board, nboard, dead, weights), "the clean batch vs spec")
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
    nb[35] = 1; want[35] = VS.PREFLOP
    nb[37] = 2; want[37] = VS.PREFLOP
    for i, n in ((39, 5), (41, 4), (43, 3)):                                  # P = k + 3: one card short of the board to come and two holdings
        nb[i] = n
        free = [c for c in range(52) if c not in used(i)]
        d[i] = sum(1 << c for c in free[(5 - n) + 3:])
        want[i] = VS.SMALL_POOL
    got = device_rvr(b, nb, d, weights)
    assert got["status"].tolist() == [VS.check_spot(b[i], nb[i], d[i])[0] for i in range(len(b))]
    for i in range(len(b)):
        if i in want:
            assert got["status"][i] == want[i] and not got["win"][i].any() and not got["tie"][i].any() and not got["tot"][i].any() and got["boards"][i] == 0, i
        else:
            assert_equal(rows(got, slice(i, i + 1)), rows(clean, slice(i, i + 1)), "neighbour %d" % i)


def explicit_from_getters(g, tables=None, weights=None):
    board, nboard = VS.table_boards(g.deck, g.turn)
    if tables is not None:
        board, nboard = board[tables], nboard[tables]
    return device_rvr(board, nboard, None, weights)


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
    got = as_dict(g.equity_rvr(weights=weights))
    assert_equal(got, want, "table form %dx%d" % (T, n))
    assert set(got["boards"][~pre].tolist()) == {1, 44, 990}
    pick = np.concatenate([rng.permutation(T)[:20], [5, 5, 5, T - 1, 0]]).astype(np.int32)   # permuted, repeated indices
    got = as_dict(g.equity_rvr(weights=weights, tables=pick))
    assert_equal(got, rows(want, pick), "table form %dx%d, index array" % (T, n))
    r = g.equity_rvr(tables=np.array([int(pick[0]), T, -1, 2 ** 31 - 1], np.int64))
    assert r.status[1:].tolist() == [VS.BAD_TABLE] * 3 and not r.boards[1:].any() and not r.win[1:].any() and not r.tot[1:].any()
    assert r.status[0] == want["status"][pick[0]] and r.boards[0] == want["boards"][pick[0]]
    assert g.save().tobytes() == before.tobytes()                            # the calls wrote nothing to the handle
    g.close()


def test_never_dealt_handle_and_the_single_game(PK):
    g = PK.VecGame(64, num_players=6)
    r = g.equity_rvr()
    assert (r.status == VS.PREFLOP).all() and not r.win.any() and not r.tot.any() and not r.boards.any()   # turn 0: nothing is read
    g.close()
    single = PK.Game(num_players=3)
    with pytest.raises(ValueError, match="fewer than three board cards"):
        single.equity_rvr()                                                  # never dealt
    single.reset()
    with pytest.raises(ValueError, match="fewer than three board cards"):
        single.equity_rvr()                                                  # pre-flop
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
    e = g.equity_rvr()
    assert e.valid is None or not e.valid.any()                              # (no mask while steps are in flight: the getters it is formed from refuse)
    r = {k: np.asarray(getattr(e, k)) for k in KEYS}
    assert ((r["status"][~idle] & VS.IN_FLIGHT) != 0).all() and not (r["status"][idle] & VS.IN_FLIGHT).any()
    assert not r["win"][~idle].any() and not r["tie"][~idle].any() and not r["tot"][~idle].any() and not r["boards"][~idle].any()
    act.upload(np.full(T, -1, np.int32))                                     # the drain: idle tables get no step and stay as they are
    g.step_async_d(act, flags, terr, ready, max_hands=0, auto_reset=True)
    g.sync()
    t = np.flatnonzero(idle)
    assert_equal(rows(r, t), explicit_from_getters(g, t), "the idle tables", KEYS)
    for b in (act, flags, terr, ready):
        b.free()
    g.close()


def test_sixteen_repeated_calls_on_each_stream_form_agree(PK):
    """The work-space regression pattern of test_hip_equity.py: a loop of calls with a synchronisation after each, at a size whose work
    space exceeds a megabyte (50 000 spots of 24 bytes; boards / status only: the other outputs are 31.8 KB per spot) -- EVERY call must
    deliver, on a caller's stream and on the pooled one -- and 64 spots with all outputs."""
    from pokerl_amd import _lib as L
    from pokerl_amd import hipmem
    from pokerl_amd import judger as J
    rng = np.random.default_rng(77)
    distinct, m, small = 40, 50000, 64
    br, nr, dr = VS.random_boards(rng, distinct - 8, 5, lambda i: int(rng.integers(4, 30)))
    bt, nt, dt = VS.random_boards(rng, 8, 4, lambda i: int(rng.integers(5, 14)))
    board, nboard, dead = (np.concatenate(x) for x in ((br, bt), (nr, nt), (dr, dt)))
    weights = random_weights(rng)
    want = VS.batch_rvr(board, nboard, dead, weights)
    pick = rng.integers(0, distinct, m)
    pick[:distinct] = np.arange(distinct)
    board, nboard, dead = board[pick], nboard[pick], dead[pick]
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0             # hipStreamNonBlocking: a caller's own stream
    ins = [hipmem.DeviceBuffer(x.nbytes).upload(x) for x in (board, nboard, dead, weights)]
    boards_d, status_d = hipmem.DeviceBuffer(m * 4), hipmem.DeviceBuffer(m)
    outs = [hipmem.DeviceBuffer(small * H * 8) for _ in range(3)]
    for rep in range(16):
        boards_d.upload(np.full(m, 7, np.uint32))
        status_d.upload(np.full(m, 7, np.uint8))
        J.range_vs_range_d(m, *[x.ptr for x in ins[:3]], weights_d=ins[3].ptr, boards_d=boards_d.ptr, status_d=status_d.ptr, stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        assert (boards_d.download(np.uint32, m) == want["boards"][pick]).all() and not status_d.download(np.uint8, m).any(), rep
        for x in outs:
            x.upload(np.full(small * H, 7, np.uint64))
        J.range_vs_range_d(small, *[x.ptr for x in ins[:3]], weights_d=ins[3].ptr, win_d=outs[0].ptr, tie_d=outs[1].ptr, tot_d=outs[2].ptr, stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        for x, k in zip(outs, ("win", "tie", "tot")):
            assert (x.download(np.uint64, small * H).reshape(small, H) == want[k][pick[:small]]).all(), (rep, k)
    assert hip.hipStreamDestroy(stream) == 0
    for x in ins + [boards_d, status_d] + outs:
        x.free()
    for rep in range(16):                                                    # the host form: a pooled stream
        boards, status = np.full(m, 7, np.uint32), np.full(m, 7, np.uint8)
        L.check(L.lib().pk_equity_rvr(0, m, L.ptr(board), L.ptr(nboard), L.ptr(dead), L.ptr(weights), 0, None, None, None, L.ptr(boards), L.ptr(status)))
        assert (boards == want["boards"][pick]).all() and not status.any(), rep
        r = J.range_vs_range_batch(board[:small], nboard[:small], dead[:small], weights)
        assert all((getattr(r, k) == want[k][pick[:small]]).all() for k in KEYS), rep


def test_sampled_equity_agrees_with_the_exact_range_against_range(PK):
    """Two hidden seats on one river board, S = 2^20 samples: every sample draws an ordered pair of disjoint holdings uniformly, so seat 0's
    win and tie fractions are sum(win) / sum(tot) and sum(tie) / sum(tot) under uniform ranges, each within 5 * sqrt(p (1 - p) / S); its equity
    (1 per win, 1/2 per tie) is .against(uniform), within 5 * sqrt((p_win + p_tie / 4 - e^2) / S)."""
    from pokerl_amd import judger as J
    rng = np.random.default_rng(605)
    board, nboard, dead = VS.random_boards(rng, 1, 5)
    cards = [int(x) for x in board[0]]
    exact = J.range_vs_range(cards)
    S = 1 << 20
    s = J.sampled_equity([None, None], cards, samples=S)
    assert s.samples == S
    den = int(exact.tot.astype(object).sum())
    assert den == 1081 * 990
    pw, pt = int(exact.win.astype(object).sum()) / den, int(exact.tie.astype(object).sum()) / den
    for name, count, p in (("win", int(s.win[0]), pw), ("tie", int(s.tie[0]), pt)):
        bound = 5.0 * math.sqrt(p * (1.0 - p) / S)
        print("%s: exact %.6f sampled %.6f deviation %.3g bound %.3g" % (name, p, count / S, abs(count / S - p), bound))
        assert abs(count / S - p) <= bound, name
    e = exact.against(np.ones(H, np.int64))
    assert e == exact.against() and math.isclose(e, pw + pt / 2, rel_tol=1e-14)
    bound = 5.0 * math.sqrt((pw + pt / 4 - e * e) / S)
    print("equity: exact %.6f sampled %.6f deviation %.3g bound %.3g" % (e, float(s.equity[0]), abs(float(s.equity[0]) - e), bound))
    assert abs(float(s.equity[0]) - e) <= bound
