#!/usr/bin/env python3
"""Timings of the ranged sampled equity (pk_equity_ranged_d / pk_table_equity_ranged_d) on one MI355X, printed as ONE JSON line and written
to profiles/equity_ranged_bench.json (stamped with the library's source hash).  Legs:
  (a) the table form at 65 536 x 6 as each table's active seat sees it, S = 1 024, every range uniform (R = 0) -- alternating, call by call
      in one process, with pk_table_equity_sampled on the same tables: `vs_sampled` = the sampled call's time over this call's;
  (b) the same with five position ranges (the top 12 / 18 / 25 / 35 / 50 % of a high-card order), range_of by seat;
  (c) one heads-up pre-flop spot, the opponent on the 25 % range, S = 2^24.
Per leg: microseconds per call (a HIP event pair on the call's stream and the host's clock, every shape warmed up, median of `--samples`),
attempts, accepted attempts, the acceptance rate and accepted attempts / s.  There is no pass mark: leg (a) carries more Philox blocks than
k_eqs and the rejections, so it cannot beat it.

    python tools/equity_ranged_bench.py [--samples 5]
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


def top_ranges(fractions):
    """uint16 [len(fractions), 1326]: weight 1 on the best `fraction` of the holdings in a crude pre-flop order (pairs, then high cards,
    suited before offsuit) -- a stand-in for position ranges, good enough to time."""
    score = np.zeros(L.EQ_HOLDINGS)
    for b in range(52):
        for a in range(b):
            ra, rb = a // 4, b // 4                                  # canonical index = rank0 * 4 + suit, rb >= ra
            score[b * (b - 1) // 2 + a] = (100 + rb if ra == rb else 2 * rb + ra + (3 if a % 4 == b % 4 else 0))
    order = np.argsort(-score, kind="stable")
    w = np.zeros((len(fractions), L.EQ_HOLDINGS), np.uint16)
    for r, f in enumerate(fractions):
        w[r, order[:int(round(f * L.EQ_HOLDINGS))]] = 1
    return w


def leg(us, each, wall, attempts, accepted, **more):
    return dict(us=round(us, 1), samples_us=each, host_clock_us=round(wall, 1), attempts=attempts, accepted=accepted,
                acceptance=round(accepted / attempts, 4), accepted_per_s=round(accepted / (us * 1e-6), 0), **more)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "equity_ranged_bench.json"))
    args = ap.parse_args()
    if pokerl_amd.device_count() < 1:
        sys.exit("equity_ranged_bench: no MI355X visible (no fallback)")
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    res = dict(tool="equity_ranged_bench", src=L.source_hash(), samples=args.samples, legs={})
    ranges = top_ranges((0.12, 0.18, 0.25, 0.35, 0.50))
    by_seat = np.array([0, 1, 2, 3, 4, 4], np.uint16)
    T, n, S = 65536, 6, 1024
    g = pokerl_amd.VecGame(T, num_players=n)
    g.reset()
    g.rollout(37)
    outs = [DeviceBuffer(T * n * 4), DeviceBuffer(T * n * 4), DeviceBuffer(T * n * 8), DeviceBuffer(T * 4), DeviceBuffer(T)]
    wd, rd = DeviceBuffer(ranges.nbytes).upload(ranges), DeviceBuffer(by_seat.nbytes).upload(by_seat)
    gs = C.c_void_p(g.stream)
    turns = np.bincount(g.turn, minlength=5).tolist()

    def ranged(w, r, ro):
        return lambda: g.equity_ranged_d(T, None, L.OBSERVER_ACTIVE, w, r, ro, False, S, 0, *outs)

    def sampled():
        g.equity_sampled_d(T, None, L.OBSERVER_ACTIVE, S, 0, *outs)

    # (a): call by call beside the sampled family's call
    a_us, a_wall, s_us = [], [], []
    for i in range(args.samples):
        us, _, wall, _ = time_stream(ranged(None, 0, None), gs, 1, warmup=2 if i == 0 else 0)
        a_us.append(us); a_wall.append(wall)
        if i == 0:
            acc = outs[3].download(np.uint32, T).astype(np.int64)
            assert not outs[4].download(np.uint8, T).any()
        s_us.append(time_stream(sampled, gs, 1, warmup=2 if i == 0 else 0)[0])
    am, sm = float(np.median(a_us)), float(np.median(s_us))
    res["legs"]["table_65536x6_active_s1024_uniform"] = leg(am, [round(x, 1) for x in a_us], float(np.median(a_wall)), T * S, int(acc.sum()), turns=turns,
                                                            sampled_us=round(sm, 1), sampled_samples_us=[round(x, 1) for x in s_us], vs_sampled=round(sm / am, 4))
    # (b): five position ranges
    us, each, wall, _ = time_stream(ranged(wd, len(ranges), rd), gs, args.samples)
    acc = outs[3].download(np.uint32, T).astype(np.int64)
    assert not outs[4].download(np.uint8, T).any()
    res["legs"]["table_65536x6_active_s1024_five_ranges"] = leg(us, each, wall, T * S, int(acc.sum()), turns=turns, time_vs_uniform=round(us / am, 4))
    for b in outs + [rd]:
        b.free()
    g.close()
    # (c): a lone heads-up pre-flop spot
    S = 1 << 24
    holes = np.full((1, 2, 2), 0xFF, np.uint8)
    holes[0, 0] = [CANON[48], CANON[51]]
    ro = np.array([[L.EQW_UNIFORM, 2]], np.uint16)
    ins = [DeviceBuffer(x.nbytes).upload(x) for x in (holes, np.zeros((1, 5), np.uint8), np.zeros(1, np.uint8), np.full(1, 3, np.uint16), ro)]
    outs = [DeviceBuffer(2 * 4), DeviceBuffer(2 * 4), DeviceBuffer(2 * 8), DeviceBuffer(4), DeviceBuffer(1)]

    def run():
        judger.ranged_equity_d(2, 1, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, S, wd.ptr, len(ranges), ins[4].ptr, None, judger.DEFAULT_SEED, 0,
                               *[x.ptr for x in outs], stream=stream)

    us, each, wall, _ = time_stream(run, stream, args.samples)
    acc = int(outs[3].download(np.uint32, 1)[0])
    assert not outs[4].download(np.uint8, 1).any()
    share = outs[2].download(np.uint64, 2).astype(np.float64)
    res["legs"]["hu_preflop_1_s16777216_range25"] = leg(us, each, wall, S, acc, hero_equity=round(float(share[0] / (L.EQ_SHARE_UNIT * acc)), 5))
    for b in ins + outs + [wd]:
        b.free()
    hip.hipStreamDestroy(stream)
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
