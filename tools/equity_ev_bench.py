#!/usr/bin/env python3
"""Timings of the showdown EV (pk_equity_ev_d / pk_table_equity_ev_d) on one MI355X, printed as ONE JSON line.  Two legs: 4 096 heads-up
pre-flop spots with unequal bets, and the table form at 65 536 x 6 after a rollout that leaves a natural mix of turns.  Each leg alternates,
call by call in one process, with pk_equity_d / pk_table_equity_d on the same spots: the same evaluations and ONE comparison where the EV
call makes one per pot level.  Per leg: microseconds per call of both (HIP events on the call's stream, every shape warmed up, median of
`--samples`, the samples kept), their ratio, and the levels per spot (existing / compared).  No threshold: the ratio is a finding.

    python tools/equity_ev_bench.py [--samples 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import pokerl_amd  # noqa: E402
from pokerl_amd import _lib as L  # noqa: E402
from pokerl_amd import hipmem, judger  # noqa: E402
from pokerl_amd.hipmem import DeviceBuffer, DeviceEvent  # noqa: E402

CANON = [((c % 4) << 4) | (c // 4) for c in range(52)]
NO_LEVEL = 0xFF


def timed(fn, stream):
    """One call between a HIP event pair on `stream`: microseconds."""
    hip = hipmem._lib()
    t0, t1 = DeviceEvent(), DeviceEvent()
    assert hip.hipEventRecord(t0.handle, stream) == 0
    fn()
    assert hip.hipEventRecord(t1.handle, stream) == 0
    assert hip.hipStreamSynchronize(stream) == 0
    return DeviceEvent.elapsed_ms(t0, t1) * 1e3


def alternate(ev_call, eq_call, stream, samples, warmup=2):
    hip = hipmem._lib()
    for _ in range(warmup):
        eq_call()
        ev_call()
    assert hip.hipStreamSynchronize(stream) == 0
    ev, eq = [], []
    for _ in range(samples):
        eq.append(timed(eq_call, stream))
        ev.append(timed(ev_call, stream))
    return ev, eq


def leg(ev, eq, level_seat, amount, boards, live):
    exists = level_seat != NO_LEVEL
    lv = np.array([bin(int(x)).count("1") for x in live], np.int64)
    compared = exists & (amount > 0)
    compared[np.arange(len(lv)), lv - 1] = False                     # (level nlive - 1, where it exists, is the last stand: not compared)
    b = boards.astype(np.int64)
    ev_us, eq_us = float(np.median(ev)), float(np.median(eq))
    return dict(ev_us=round(ev_us, 1), ev_samples_us=[round(x, 1) for x in ev], equity_us=round(eq_us, 1), equity_samples_us=[round(x, 1) for x in eq],
                ratio_ev_over_equity=round(ev_us / eq_us, 3), spots=int(len(b)), boards=int(b.sum()), evals=int((b * lv).sum()),
                levels_per_spot=round(float(exists.sum(axis=1).mean()), 3), compared_levels_per_spot=round(float(compared.sum(axis=1).mean()), 3),
                comparisons=int((b * compared.sum(axis=1)).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "equity_ev_bench.json"))
    args = ap.parse_args()
    if pokerl_amd.device_count() < 1:
        sys.exit("equity_ev_bench: no MI355X visible (no fallback)")
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    rng = np.random.default_rng(0)
    res = dict(tool="equity_ev_bench", src=L.source_hash(), samples=args.samples, legs={})
    # ---- 4 096 heads-up pre-flop spots with unequal bets
    m, n = 4096, 2
    holes = np.zeros((m, n, 2), np.uint8)
    for i in range(m):
        holes[i] = np.array([CANON[c] for c in rng.permutation(52)[:2 * n]], np.uint8).reshape(n, 2)
    live = np.full(m, 3, np.uint16)
    bets = np.stack([rng.integers(1, 50, m), rng.integers(50, 200, m)], axis=1).astype(np.float64)
    ins = [DeviceBuffer(x.nbytes).upload(x) for x in (holes, np.zeros((m, 5), np.uint8), np.zeros(m, np.uint8), live)]
    bets_d = DeviceBuffer(bets.nbytes).upload(bets)
    eq_outs = [DeviceBuffer(m * n * 4), DeviceBuffer(m * n * 4), DeviceBuffer(m * n * 8), DeviceBuffer(m * 4), DeviceBuffer(m)]
    ev_outs = dict(share=DeviceBuffer(m * n * n * 8), level_seat=DeviceBuffer(m * n), amount=DeviceBuffer(m * n * 8), ev=DeviceBuffer(m * n * 8),
                   boards=DeviceBuffer(m * 4), status=DeviceBuffer(m))

    def ev_call():
        judger.showdown_ev_d(n, m, *[x.ptr for x in ins], bets_d.ptr, ev_outs["status"].ptr, ev_outs["share"].ptr, ev_outs["level_seat"].ptr,
                             ev_outs["amount"].ptr, ev_outs["ev"].ptr, ev_outs["boards"].ptr, stream=stream)

    def eq_call():
        judger.showdown_equity_d(n, m, *[x.ptr for x in ins], *[x.ptr for x in eq_outs], stream=stream)
    ev, eq = alternate(ev_call, eq_call, stream, args.samples)
    assert not ev_outs["status"].download(np.uint8, m).any()
    res["legs"]["hu_preflop_4096"] = leg(ev, eq, ev_outs["level_seat"].download(np.uint8, m * n).reshape(m, n),
                                         ev_outs["amount"].download(np.float64, m * n).reshape(m, n), ev_outs["boards"].download(np.uint32, m), live)
    for b in ins + [bets_d] + eq_outs + list(ev_outs.values()):
        b.free()
    # ---- the table form at 65 536 x 6 on the natural mix of turns
    T, n = 65536, 6
    g = pokerl_amd.VecGame(T, num_players=n)
    g.reset()
    g.rollout(37)
    gs = C.c_void_p(g.stream)
    eq_outs = [DeviceBuffer(T * n * 4), DeviceBuffer(T * n * 4), DeviceBuffer(T * n * 8), DeviceBuffer(T * 4), DeviceBuffer(T)]
    ev_outs = dict(share=DeviceBuffer(T * n * n * 8), level_seat=DeviceBuffer(T * n), amount=DeviceBuffer(T * n * 8), ev=DeviceBuffer(T * n * 8),
                   boards=DeviceBuffer(T * 4), status=DeviceBuffer(T))
    ev, eq = alternate(lambda: g.equity_ev_d(ev_outs["status"], T, None, ev_outs["share"], ev_outs["level_seat"], ev_outs["amount"], ev_outs["ev"], ev_outs["boards"]),
                       lambda: g.equity_d(T, None, *eq_outs), gs, args.samples, warmup=1)
    status, eq_status = ev_outs["status"].download(np.uint8, T), eq_outs[4].download(np.uint8, T)
    # a table pk_table_equity refuses is refused here too; beyond those only PK_EQ_BAD_BET: the reference's game lets a seat's credits, and
    # with them its blind, fall below zero now and then -- a few tables in ten thousand, counted in status_counts
    assert ((status & ~np.uint8(L.EQ_BAD_BET)) == eq_status).all()
    ps = g.player_states
    live = (((ps == 1) | (ps == 2) | (ps == 3)).astype(np.uint16) << np.arange(n, dtype=np.uint16)).sum(axis=1).astype(np.uint16)
    res["legs"]["table_65536x6"] = dict(leg(ev, eq, ev_outs["level_seat"].download(np.uint8, T * n).reshape(T, n),
                                            ev_outs["amount"].download(np.float64, T * n).reshape(T, n), ev_outs["boards"].download(np.uint32, T), live),
                                        turns=np.bincount(g.turn, minlength=5).tolist(), status_counts={str(k): int(v) for k, v in zip(*np.unique(status, return_counts=True))})
    for b in eq_outs + list(ev_outs.values()):
        b.free()
    g.close()
    hip.hipStreamDestroy(stream)
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
