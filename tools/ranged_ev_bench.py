#!/usr/bin/env python3
"""Timings of the ranged showdown EV (pk_ev_ranged_d / pk_table_ev_ranged_d) on one MI355X against pk_equity_ranged(_d) on the same spots,
ranges and S -- the parent's kernel, the natural baseline -- printed as ONE JSON line and written to profiles/ranged_ev_bench.json (stamped
with the library's source hash).  Legs, each alternating call by call in one process with its baseline:
  (a) 65 536 x 6 tables as they stand, observer 'active', R = 1, S = 256;
  (b) 4 096 explicit six-seat spots on a ladder of bets (two groups of levels), the hero shown, R = 4, S = 4 096;
  (c) 256 sixteen-seat spots on a ladder (eight groups), every seat hidden behind a row of its own, R = 16, S = 4 096.
Per leg: microseconds per call (a HIP event pair on the call's stream and the host's clock, every shape warmed up, median of `--samples`),
attempts, accepted attempts, the acceptance rate, accepted attempts / s and `vs_ranged` = this call's time over the baseline's.  There is no
pass mark: a spot with g groups of levels to compare draws its attempts g times.

    python tools/ranged_ev_bench.py [--samples 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import pokerl_amd  # noqa: E402
from pokerl_amd import _lib as L  # noqa: E402
from pokerl_amd import hipmem, judger  # noqa: E402
from pokerl_amd.hipmem import DeviceBuffer  # noqa: E402
from equity_bench import CANON, time_stream  # noqa: E402
from equity_ranged_bench import top_ranges  # noqa: E402


def alternate(ev_call, base_call, stream, samples):
    """The two calls timed call by call, one after the other -> (ev us samples, ev host clock samples, baseline us samples)."""
    e_us, e_wall, b_us = [], [], []
    for i in range(samples):
        us, _, wall, _ = time_stream(ev_call, stream, 1, warmup=2 if i == 0 else 0)
        e_us.append(us); e_wall.append(wall)
        b_us.append(time_stream(base_call, stream, 1, warmup=2 if i == 0 else 0)[0])
    return e_us, e_wall, b_us


def leg(e_us, e_wall, b_us, attempts, accepted, **more):
    us, base = float(np.median(e_us)), float(np.median(b_us))
    return dict(us=round(us, 1), samples_us=[round(x, 1) for x in e_us], host_clock_us=round(float(np.median(e_wall)), 1), attempts=attempts,
                accepted=accepted, acceptance=round(accepted / attempts, 4), accepted_per_s=round(accepted / (us * 1e-6), 0),
                ranged_us=round(base, 1), ranged_samples_us=[round(x, 1) for x in b_us], vs_ranged=round(us / base, 4), **more)


def explicit_leg(stream, samples, n, m, S, holes, board, nboard, live, bets, weights, ro):
    ins = [DeviceBuffer(x.nbytes).upload(x) for x in (holes, board, nboard, live, bets, weights, ro)]
    ev_outs = [DeviceBuffer(m * n * n * 8), DeviceBuffer(m * n), DeviceBuffer(m * n * 8), DeviceBuffer(m * n * 8), DeviceBuffer(m * 4), DeviceBuffer(m)]
    eq_outs = [DeviceBuffer(m * n * 4), DeviceBuffer(m * n * 4), DeviceBuffer(m * n * 8), DeviceBuffer(m * 4), DeviceBuffer(m)]
    R = len(weights)

    def ev_call():
        judger.ranged_ev_d(n, m, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, ins[4].ptr, S, ev_outs[5].ptr, ins[5].ptr, R, ins[6].ptr, None,
                           judger.DEFAULT_SEED, 0, *[x.ptr for x in ev_outs[:5]], stream=stream)

    def base_call():
        judger.ranged_equity_d(n, m, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, S, ins[5].ptr, R, ins[6].ptr, None, judger.DEFAULT_SEED, 0,
                               *[x.ptr for x in eq_outs], stream=stream)

    e_us, e_wall, b_us = alternate(ev_call, base_call, stream, samples)
    acc = ev_outs[4].download(np.uint32, m).astype(np.int64)
    assert not ev_outs[5].download(np.uint8, m).any() and np.array_equal(acc, eq_outs[3].download(np.uint32, m))
    seat = ev_outs[1].download(np.uint8, m * n).reshape(m, n)
    out = leg(e_us, e_wall, b_us, m * S, int(acc.sum()), levels_per_spot=round(float((seat != 0xFF).sum(axis=1).mean()), 2))
    for b in ins + ev_outs + eq_outs:
        b.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ranged_ev_bench.json"))
    args = ap.parse_args()
    if pokerl_amd.device_count() < 1:
        sys.exit("ranged_ev_bench: no MI355X visible (no fallback)")
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    res = dict(tool="ranged_ev_bench", src=L.source_hash(), samples=args.samples, legs={})
    # (a): the table form, one range for every hidden seat
    T, n, S = 65536, 6, 256
    one = top_ranges((0.35,))
    by_seat = np.zeros(n, np.uint16)
    g = pokerl_amd.VecGame(T, num_players=n)
    g.reset()
    g.rollout(37)
    wd, rd = DeviceBuffer(one.nbytes).upload(one), DeviceBuffer(by_seat.nbytes).upload(by_seat)
    ev_outs = [DeviceBuffer(T * n * n * 8), DeviceBuffer(T * n), DeviceBuffer(T * n * 8), DeviceBuffer(T * n * 8), DeviceBuffer(T * 4), DeviceBuffer(T)]
    eq_outs = [DeviceBuffer(T * n * 4), DeviceBuffer(T * n * 4), DeviceBuffer(T * n * 8), DeviceBuffer(T * 4), DeviceBuffer(T)]
    gs = C.c_void_p(g.stream)
    turns = np.bincount(g.turn, minlength=5).tolist()
    e_us, e_wall, b_us = alternate(lambda: g.ev_ranged_d(ev_outs[5], T, None, L.OBSERVER_ACTIVE, wd, 1, rd, False, S, 0, *ev_outs[:5]),
                                   lambda: g.equity_ranged_d(T, None, L.OBSERVER_ACTIVE, wd, 1, rd, False, S, 0, *eq_outs), gs, args.samples)
    acc = ev_outs[4].download(np.uint32, T).astype(np.int64)
    status, eq_status = ev_outs[5].download(np.uint8, T), eq_outs[4].download(np.uint8, T)
    # a table pk_table_equity_ranged refuses is refused here too; beyond those only PK_EQ_BAD_BET: the reference's game lets a seat's credits,
    # and with them its blind, fall below zero now and then -- a few tables in ten thousand, counted in status_counts
    assert ((status & ~np.uint8(L.EQ_BAD_BET)) == eq_status).all()
    ok = status == 0
    assert np.array_equal(acc[ok], eq_outs[3].download(np.uint32, T)[ok]) and not acc[~ok].any()
    seat = ev_outs[1].download(np.uint8, T * n).reshape(T, n)
    res["legs"]["table_65536x6_active_s256_r1"] = leg(e_us, e_wall, b_us, T * S, int(acc.sum()), turns=turns,
                                                      levels_per_spot=round(float((seat[ok] != 0xFF).sum(axis=1).mean()), 2),
                                                      status_counts={str(k): int(v) for k, v in zip(*np.unique(status, return_counts=True))})
    for b in ev_outs + eq_outs + [wd, rd]:
        b.free()
    g.close()
    # (b): explicit six-seat spots on a ladder, the hero (seat 0) shown on the flop, four position ranges
    rng = np.random.default_rng(7)
    m, n, S = 4096, 6, 4096
    four = top_ranges((0.12, 0.25, 0.35, 0.50))
    holes = np.full((m, n, 2), 0xFF, np.uint8)
    board = np.zeros((m, 5), np.uint8)
    for i in range(m):
        c = rng.permutation(52)[:5]
        holes[i, 0] = [CANON[c[0]], CANON[c[1]]]
        board[i, :3] = [CANON[x] for x in c[2:]]
    ro = np.tile(np.array([L.EQW_UNIFORM, 0, 1, 2, 3, 3], np.uint16), (m, 1))
    bets = np.tile(10.0 * (np.arange(n) + 1), (m, 1))
    res["legs"]["explicit_4096x6_ladder_s4096_r4"] = explicit_leg(stream, args.samples, n, m, S, holes, board, np.full(m, 3, np.uint8),
                                                                  np.full(m, (1 << n) - 1, np.uint16), bets, four, ro)
    # (c): sixteen seats, every one hidden behind a row of its own (three holdings among the cards 3 r .. 3 r + 2: no collisions), a ladder
    m, n, S = 256, 16, 4096
    sixteen = np.zeros((16, L.EQ_HOLDINGS), np.uint16)
    for r in range(16):
        for a, b in ((3 * r, 3 * r + 1), (3 * r, 3 * r + 2), (3 * r + 1, 3 * r + 2)):
            sixteen[r, b * (b - 1) // 2 + a] = int(rng.integers(1, 65536))
    holes = np.full((m, n, 2), 0xFF, np.uint8)
    ro = np.array([np.roll(np.arange(16), i) for i in range(m)], np.uint16)
    bets = np.tile(10.0 * (np.arange(n) + 1), (m, 1))
    res["legs"]["explicit_256x16_ladder_s4096_r16"] = explicit_leg(stream, args.samples, n, m, S, holes, np.zeros((m, 5), np.uint8), np.zeros(m, np.uint8),
                                                                   np.full(m, 0xFFFF, np.uint16), bets, sixteen, ro)
    hip.hipStreamDestroy(stream)
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
