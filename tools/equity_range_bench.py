#!/usr/bin/env python3
"""Timings of the range equity (pk_equity_range_d / pk_table_equity_range_d) on one MI355X, printed as ONE JSON line and written to
profiles/equity_range_bench.json (stamped with the library's source hash).  Legs: 65 536 explicit flop / turn / river spots, `agg` only; the
same with the per-holding outputs at 4 096 spots; the table form at 65 536 x 6 on a natural mix of turns (pre-flop tables are refused and
cost nothing); one lone flop spot.  THE YARDSTICK, in the same run: the old way per hero spot -- 64 flop hero spots expanded on the host to
64 x 1 081 two-seat spots through pk_equity_d, DEVICE TIME ONLY, which flatters the old way: the host expansion and the upload of 69 184
spots are not counted.  And the streaming evaluator pk_time_eval7_d at 2^28 hands, for scale, alternating with the legs.
Per leg: microseconds per call (a HIP event pair on the call's stream and the host's clock, every shape warmed up, median of `--samples`),
hero spots, distinct villain evaluations (the sets S: C(P, 7 - nb) per spot) and hero evaluations (C(P, 5 - nb)), evaluations/s.
Recorded beside them: time per hero spot new against old, the ratio to the streaming evaluator, and the kernel's registers, LDS and
occupancy out of the built library's code objects.

    python tools/equity_range_bench.py [--samples 5]
"""
import argparse
import ctypes as C
import json
import math
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
from equity_bench import CANON, EVAL_HANDS, Explicit, time_stream  # noqa: E402
import kernel_meta  # noqa: E402

H = L.EQ_HOLDINGS


def random_spots(rng, m, nb):
    hero, board = np.zeros((m, 2), np.uint8), np.zeros((m, 5), np.uint8)
    for i in range(m):
        deck = [CANON[c] for c in rng.permutation(52)[:7]]
        hero[i], board[i] = deck[:2], deck[2:]
    return hero, board, np.full(m, nb, np.uint8)


def leg(timing, spots, villain_evals, hero_evals, **more):
    us, each, wall, odd = timing
    return dict(us=round(us, 1), samples_us=each, host_clock_us=round(wall, 1), event_anomalies=odd, hero_spots=spots,
                us_per_hero_spot=round(us / max(spots, 1), 4), villain_evals=villain_evals, hero_evals=hero_evals,
                villain_evals_per_s=round(villain_evals / (us * 1e-6), 0), **more)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "equity_range_bench.json"))
    args = ap.parse_args()
    if pokerl_amd.device_count() < 1:
        sys.exit("equity_range_bench: no MI355X visible (no fallback)")
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    rng = np.random.default_rng(0)
    res = dict(tool="equity_range_bench", src=L.source_hash(), samples=args.samples, legs={})
    meta = kernel_meta.kernels(L.LIB_PATH)["k_eqr"]
    waves = min(8, 512 // max(meta["vgprs"], 1)) if meta["vgprs"] > 0 else 8
    res["k_eqr"] = dict(vgprs=meta["vgprs"], sgprs=meta["sgprs"], lds=meta["lds"], scratch=meta["private_segment"], block=512,
                        workgroups_per_cu_by_lds=163840 // meta["lds"], waves_per_simd_by_vgprs=waves,
                        waves_per_simd=min(waves, 2 * (163840 // meta["lds"])))
    hands_d, out_d = DeviceBuffer(EVAL_HANDS * 8), DeviceBuffer(EVAL_HANDS * 4)
    judger.make_hands(hands_d.ptr, EVAL_HANDS)
    stream_rates = []

    def stream_rate():
        ms = judger.time_eval7_stream(hands_d.ptr, EVAL_HANDS, out_d.ptr, reps=3)
        stream_rates.append(EVAL_HANDS / (ms * 1e-3))

    stream_rate()                                                     # (warm)
    stream_rates.clear()
    weights = rng.integers(0, 65536, H).astype(np.uint16)
    w_d = DeviceBuffer(weights.nbytes).upload(weights)
    # ---- the explicit form: agg only at 65 536 spots, per-holding outputs at 4 096, one lone flop spot
    for name, m, nb, per_holding in (("flop_65536_agg", 65536, 3, False), ("turn_65536_agg", 65536, 4, False), ("river_65536_agg", 65536, 5, False),
                                     ("flop_4096_per_holding", 4096, 3, True), ("turn_4096_per_holding", 4096, 4, True),
                                     ("river_4096_per_holding", 4096, 5, True), ("flop_1", 1, 3, True)):
        hero, board, nboard = random_spots(rng, m, nb)
        ins = [DeviceBuffer(x.nbytes).upload(x) for x in (hero, board, nboard)]
        agg, boards, status = DeviceBuffer(m * 24), DeviceBuffer(m * 4), DeviceBuffer(m)
        win = DeviceBuffer(m * H * 4) if per_holding else None
        tie = DeviceBuffer(m * H * 4) if per_holding else None

        def run():
            judger.range_equity_d(m, *[x.ptr for x in ins], weights_d=w_d.ptr, agg_d=agg.ptr, win_d=win and win.ptr, tie_d=tie and tie.ptr,
                                  boards_d=boards.ptr, status_d=status.ptr, stream=stream)

        stream_rate()
        timing = time_stream(run, stream, args.samples)
        stream_rate()
        assert not status.download(np.uint8, m).any() and (boards.download(np.uint32, m) == math.comb(48 - nb, 5 - nb)).all()
        p = 50 - nb
        res["legs"][name] = leg(timing, m, m * math.comb(p, 7 - nb), m * math.comb(p, 5 - nb))
        for b in ins + [agg, boards, status] + ([win, tie] if per_holding else []):
            b.free()
    # ---- the yardstick: the old way, 64 flop hero spots as 64 x 1 081 two-seat spots through pk_equity_d (device time only)
    m0 = 64
    hero, board, _ = random_spots(rng, m0, 3)
    holes = np.zeros((m0, 1081, 2, 2), np.uint8)
    for i in range(m0):
        gone = {int(c) for c in hero[i]} | {int(c) for c in board[i, :3]}
        pool = [c for c in CANON if c not in gone]
        holes[i, :, 0] = hero[i]
        holes[i, :, 1] = [(pool[a], pool[b]) for b in range(47) for a in range(b)]
    old = Explicit(holes.reshape(-1, 2, 2), np.repeat(board, 1081, axis=0), np.full(m0 * 1081, 3, np.uint8), np.full(m0 * 1081, 3, np.uint16), stream)
    stream_rate()
    timing = time_stream(old.run, stream, args.samples)
    stream_rate()
    nboards, evals = old.evals()
    assert nboards == m0 * 1081 * 990
    us = timing[0]
    res["legs"]["old_way_flop_64"] = dict(us=round(us, 1), samples_us=timing[1], host_clock_us=round(timing[2], 1), event_anomalies=timing[3], hero_spots=m0,
                                          us_per_hero_spot=round(us / m0, 4), evals=evals, evals_per_s=round(evals / (us * 1e-6), 0),
                                          note="device time only: the host expansion to 69 184 two-seat spots and their upload are not counted")
    old.free()
    # ---- the table form on a natural mix of turns
    T, n = 65536, 6
    g = pokerl_amd.VecGame(T, num_players=n)
    g.reset()
    g.rollout(37)
    turns = np.bincount(g.turn, minlength=5).tolist()
    agg, boards, status = DeviceBuffer(T * 24), DeviceBuffer(T * 4), DeviceBuffer(T)
    gs = C.c_void_p(g.stream)
    stream_rate()
    timing = time_stream(lambda: g.equity_range_d(T, None, "active", w_d, False, agg, None, None, boards, status), gs, args.samples)
    stream_rate()
    st = status.download(np.uint8, T)
    turn = g.turn
    assert ((st == 0) == (turn > 0)).all() and (st[turn == 0] == L.EQ_PREFLOP).all()
    nbs = np.minimum(turn[turn > 0] + 2, 5)
    p = 52 - 2 - nbs
    res["legs"]["table_65536x6_active_agg"] = leg(timing, int((turn > 0).sum()), int(sum(math.comb(int(a), 7 - int(b)) for a, b in zip(p, nbs))),
                                                  int(sum(math.comb(int(a), 5 - int(b)) for a, b in zip(p, nbs))), turns=turns, tables=T)
    for b in (agg, boards, status):
        b.free()
    g.close()
    res["eval7_stream_hands_per_s"] = round(float(np.median(stream_rates)), 0)
    res["eval7_stream_samples"] = [round(x, 0) for x in stream_rates]
    hands_d.free(); out_d.free(); w_d.free()
    for k, v in res["legs"].items():
        rate = v.get("villain_evals_per_s", v.get("evals_per_s"))
        v["vs_eval7_stream"] = round(rate / res["eval7_stream_hands_per_s"], 3)
    new, old_leg = res["legs"]["flop_65536_agg"], res["legs"]["old_way_flop_64"]
    res["flop_us_per_hero_spot"] = dict(new=new["us_per_hero_spot"], old=old_leg["us_per_hero_spot"],
                                        old_over_new=round(old_leg["us_per_hero_spot"] / new["us_per_hero_spot"], 2))
    hip.hipStreamDestroy(stream)
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
