#!/usr/bin/env python3
"""Timings of the sampled showdown equity (pk_equity_sampled_d / pk_table_equity_sampled_d) on one MI355X, printed as ONE JSON line and
written to profiles/equity_sampled_bench.json (stamped with the library's source hash).  Legs: the table form at 65 536 x 6 as each
table's active seat sees it, S = 1 024; 4 096 heads-up pre-flop spots with the opponent hidden, S = 65 536; one such spot at S = 2^20; the
table form at 65 536 x 6 with every hole card known (OBSERVER_NONE: only the board is drawn), S = 1 024, beside the exact pk_table_equity on
the same tables.  Per leg: microseconds per call (a HIP event pair on the call's stream and the host's clock, every shape warmed up,
median of `--samples`), samples, hand evaluations (samples x live seats) and evaluations/s -- and, in the same process, alternating with
the legs, the stand-alone streaming evaluator's rate (pk_time_eval7_d at 2^28 hands): the yardstick.

    python tools/equity_sampled_bench.py [--samples 5]
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
from equity_bench import CANON, EVAL_HANDS, time_stream  # noqa: E402


def leg(timing, samples, evals, **more):
    us, each, wall, odd = timing
    return dict(us=round(us, 1), samples_us=each, host_clock_us=round(wall, 1), event_anomalies=odd, samples=samples, evals=evals,
                evals_per_s=round(evals / (us * 1e-6), 0), **more)


def live_counts(g):
    ps = g.player_states
    return ((ps == 1) | (ps == 2) | (ps == 3)).sum(axis=1).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "equity_sampled_bench.json"))
    args = ap.parse_args()
    if pokerl_amd.device_count() < 1:
        sys.exit("equity_sampled_bench: no MI355X visible (no fallback)")
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    rng = np.random.default_rng(0)
    res = dict(tool="equity_sampled_bench", src=L.source_hash(), samples=args.samples, legs={})
    hands_d, out_d = DeviceBuffer(EVAL_HANDS * 8), DeviceBuffer(EVAL_HANDS * 4)
    judger.make_hands(hands_d.ptr, EVAL_HANDS)
    stream_rates = []

    def stream_rate():
        ms = judger.time_eval7_stream(hands_d.ptr, EVAL_HANDS, out_d.ptr, reps=3)
        stream_rates.append(EVAL_HANDS / (ms * 1e-3))

    stream_rate()                                                     # (warm)
    stream_rates.clear()
    # ---- the table forms on a natural mix of turns
    T, n, S = 65536, 6, 1024
    g = pokerl_amd.VecGame(T, num_players=n)
    g.reset()
    g.rollout(37)
    lv = live_counts(g)
    outs = [DeviceBuffer(T * n * 4), DeviceBuffer(T * n * 4), DeviceBuffer(T * n * 8), DeviceBuffer(T * 4), DeviceBuffer(T)]
    gs = C.c_void_p(g.stream)
    turns = np.bincount(g.turn, minlength=5).tolist()
    for name, observer in (("table_65536x6_active_s1024", L.OBSERVER_ACTIVE), ("table_65536x6_none_s1024", L.OBSERVER_NONE)):
        stream_rate()
        timing = time_stream(lambda: g.equity_sampled_d(T, None, observer, S, 0, *outs), gs, args.samples)
        stream_rate()
        count = outs[3].download(np.uint32, T).astype(np.int64)
        assert not outs[4].download(np.uint8, T).any() and (count == S).all()
        res["legs"][name] = leg(timing, int(count.sum()), int((count * lv).sum()), turns=turns)
    stream_rate()
    timing = time_stream(lambda: g.equity_d(T, None, *outs), gs, args.samples)       # the exact call on the same tables
    stream_rate()
    boards = outs[3].download(np.uint32, T).astype(np.int64)
    exact = leg(timing, int(boards.sum()), int((boards * lv).sum()))
    exact["boards"] = exact.pop("samples")
    res["legs"]["table_65536x6_exact"] = exact
    res["legs"]["table_65536x6_none_s1024"]["time_vs_exact"] = round(res["legs"]["table_65536x6_none_s1024"]["us"] / exact["us"], 4)
    for b in outs:
        b.free()
    g.close()
    # ---- heads-up pre-flop, the opponent hidden
    for name, m, S in (("hu_preflop_hidden_4096_s65536", 4096, 65536), ("hu_preflop_hidden_1_s1048576", 1, 1 << 20)):
        holes = np.full((m, 2, 2), 0xFF, np.uint8)
        for i in range(m):
            holes[i, 0] = [CANON[c] for c in rng.permutation(52)[:2]]
        ins = [DeviceBuffer(x.nbytes).upload(x) for x in (holes, np.zeros((m, 5), np.uint8), np.zeros(m, np.uint8), np.full(m, 3, np.uint16))]
        outs = [DeviceBuffer(m * 2 * 4), DeviceBuffer(m * 2 * 4), DeviceBuffer(m * 2 * 8), DeviceBuffer(m * 4), DeviceBuffer(m)]

        def run():
            judger.sampled_equity_d(2, m, *[x.ptr for x in ins], S, None, judger.DEFAULT_SEED, 0, *[x.ptr for x in outs], stream=stream)

        stream_rate()
        timing = time_stream(run, stream, args.samples)
        stream_rate()
        count = outs[3].download(np.uint32, m).astype(np.int64)
        assert not outs[4].download(np.uint8, m).any() and (count == S).all()
        res["legs"][name] = leg(timing, int(count.sum()), int(2 * count.sum()))
        for b in ins + outs:
            b.free()
    res["eval7_stream_hands_per_s"] = round(float(np.median(stream_rates)), 0)
    res["eval7_stream_samples"] = [round(x, 0) for x in stream_rates]
    hands_d.free(); out_d.free()
    for v in res["legs"].values():
        v["vs_eval7_stream"] = round(v["evals_per_s"] / res["eval7_stream_hands_per_s"], 3)
    hip.hipStreamDestroy(stream)
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
