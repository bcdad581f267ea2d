#!/usr/bin/env python3
"""Timings of the showdown equity (pk_equity_d / pk_table_equity_d) on one MI355X, printed as ONE JSON line.  Legs: one heads-up pre-flop
spot; one 6-seat pre-flop spot; 4 096 heads-up pre-flop spots; the table form at 65 536 x 6 and 1 048 576 x 6 after a rollout that leaves a
natural mix of turns; 65 536 x 6 forced to the flop (the same tables' cards and live seats with nb = 3, through the explicit form).  Per
leg: microseconds per call (HIP events on the call's stream, every shape warmed up, median of `--samples`), boards, hand evaluations
(boards x live seats) and evaluations/s -- and, in the same process, alternating with the wide legs, the stand-alone streaming evaluator's
rate (pk_time_eval7_d at 2^28 hands): the yardstick of the wide legs.  The yardstick of the narrow (flop) leg is what a caller could do
before: host-enumerated 7-card hands of ALL the leg's tables through pk_eval7_d in one call, then pk_compare_rankings.  Only the
evaluator's DEVICE time is set against the new call (host enumeration, every copy and the whole comparison pass excluded: flattering the
old way); the comparison pass is timed separately on `--old-tables` tables as the host call a caller has, copies included.

    python tools/equity_bench.py [--samples 5] [--skip-1m] [--out FILE]
"""
import argparse
import ctypes as C
import itertools
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
EVAL_HANDS = 1 << 28


class Explicit:
    """Device buffers of an explicit batch and its outputs; run() queues one pk_equity_d call on `stream`."""

    def __init__(self, holes, board, nboard, live, stream):
        self.m, self.n = holes.shape[:2]
        self.stream = stream
        self.ins = [DeviceBuffer(x.nbytes).upload(x) for x in (holes, board, nboard, live)]
        m, n = self.m, self.n
        self.outs = [DeviceBuffer(m * n * 4), DeviceBuffer(m * n * 4), DeviceBuffer(m * n * 8), DeviceBuffer(m * 4), DeviceBuffer(m)]
        self.live = live

    def run(self):
        judger.showdown_equity_d(self.n, self.m, *[x.ptr for x in self.ins], *[x.ptr for x in self.outs], stream=self.stream)

    def evals(self):
        boards = self.outs[3].download(np.uint32, self.m).astype(np.int64)
        status = self.outs[4].download(np.uint8, self.m)
        assert not status.any()
        lv = np.array([bin(int(x)).count("1") for x in self.live], np.int64)
        return int(boards.sum()), int((boards * lv).sum())

    def free(self):
        for b in self.ins + self.outs:
            b.free()


def time_stream(fn, stream, samples, warmup=2):
    """One call timed `samples` times by a HIP event pair on `stream` AND by the host's clock around call + synchronize.  Returns the
    median of the event times, the event samples, the median host time and how many event samples came out below half of their own host
    time on a call longer than 50 us (seen on the explicit form only, whose work space comes from the stream-ordered allocator: DESIGN.md
    section 3.1 -- reported, never corrected)."""
    import time
    hip = hipmem._lib()
    for _ in range(warmup):
        fn()
    assert hip.hipStreamSynchronize(stream) == 0
    t0, t1 = DeviceEvent(), DeviceEvent()
    out, wall = [], []
    for _ in range(samples):
        w0 = time.perf_counter()
        assert hip.hipEventRecord(t0.handle, stream) == 0
        fn()
        assert hip.hipEventRecord(t1.handle, stream) == 0
        assert hip.hipStreamSynchronize(stream) == 0
        wall.append((time.perf_counter() - w0) * 1e6)
        out.append(DeviceEvent.elapsed_ms(t0, t1) * 1e3)
    odd = sum(1 for e, w in zip(out, wall) if w > 50.0 and e < 0.5 * w)
    return float(np.median(out)), [round(x, 1) for x in out], float(np.median(wall)), odd


def leg(timing, boards, evals):
    us, samples, wall, odd = timing
    return dict(us=round(us, 1), samples_us=samples, host_clock_us=round(wall, 1), event_anomalies=odd, boards=boards, evals=evals,
                evals_per_s=round(evals / (us * 1e-6), 0))


def preflop_spots(rng, n, m):
    holes = np.zeros((m, n, 2), np.uint8)
    for i in range(m):
        holes[i] = np.array([CANON[c] for c in rng.permutation(52)[:2 * n]], np.uint8).reshape(n, 2)
    return holes, np.zeros((m, 5), np.uint8), np.zeros(m, np.uint8), np.full(m, (1 << n) - 1, np.uint16)


def table_spots(g):
    deck, ps, n = g.deck, g.player_states, g.num_players
    live = (((ps == 1) | (ps == 2) | (ps == 3)).astype(np.uint16) << np.arange(n, dtype=np.uint16)).sum(axis=1).astype(np.uint16)
    return np.ascontiguousarray(deck[:, 5:].reshape(-1, n, 2)), np.ascontiguousarray(deck[:, :5]), live


def old_way_hands(holes, board, live):
    """Every (board, live seat) 7-card hand of flop spots, one per 64-bit word (card i = byte i), enumerated on the host."""
    words = []
    for h, b, lv in zip(holes, board, live):
        dead = set(int(x) for x in b[:3]) | set(int(x) for x in h.reshape(-1))
        pool = np.array([c for c in CANON if c not in dead], np.uint64)
        i, j = np.triu_indices(len(pool), 1)
        base = sum(np.uint64(int(b[k])) << np.uint64(8 * k) for k in range(3)) | (pool[i] << np.uint64(24)) | (pool[j] << np.uint64(32))
        for p in range(h.shape[0]):
            if (int(lv) >> p) & 1:
                words.append(base | (np.uint64(int(h[p, 0])) << np.uint64(40)) | (np.uint64(int(h[p, 1])) << np.uint64(48)))
    return np.concatenate(words)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--old-tables", type=int, default=1024)
    ap.add_argument("--skip-1m", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "equity_bench.json"))
    args = ap.parse_args()
    if pokerl_amd.device_count() < 1:
        sys.exit("equity_bench: no MI355X visible (no fallback)")
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    rng = np.random.default_rng(0)
    res = dict(tool="equity_bench", src=L.source_hash(), samples=args.samples, legs={})
    hands_d, out_d = DeviceBuffer(EVAL_HANDS * 8), DeviceBuffer(EVAL_HANDS * 4)
    judger.make_hands(hands_d.ptr, EVAL_HANDS)
    stream_rates = []

    def stream_rate():
        ms = judger.time_eval7_stream(hands_d.ptr, EVAL_HANDS, out_d.ptr, reps=3)
        stream_rates.append(EVAL_HANDS / (ms * 1e-3))

    stream_rate()                                                     # (warm)
    stream_rates.clear()
    # ---- wide legs, alternating with the streaming evaluator
    for name, n, m, samples in (("hu_preflop_1", 2, 1, args.samples), ("six_preflop_1", 6, 1, args.samples), ("hu_preflop_4096", 2, 4096, args.samples)):
        e = Explicit(*preflop_spots(rng, n, m), stream)
        stream_rate()
        timing = time_stream(e.run, stream, samples)
        stream_rate()
        res["legs"][name] = leg(timing, *e.evals())
        e.free()
    res["eval7_stream_hands_per_s"] = round(float(np.median(stream_rates)), 0)
    res["eval7_stream_samples"] = [round(x, 0) for x in stream_rates]
    hands_d.free(); out_d.free()
    for k in ("hu_preflop_1", "six_preflop_1", "hu_preflop_4096"):
        res["legs"][k]["vs_eval7_stream"] = round(res["legs"][k]["evals_per_s"] / res["eval7_stream_hands_per_s"], 3)
    # ---- the table form on a natural mix of turns
    for T in [65536] + ([] if args.skip_1m else [1048576]):
        g = pokerl_amd.VecGame(T, num_players=6)
        g.reset()
        g.rollout(37)
        n = 6
        outs = [DeviceBuffer(T * n * 4), DeviceBuffer(T * n * 4), DeviceBuffer(T * n * 8), DeviceBuffer(T * 4), DeviceBuffer(T)]
        gs = C.c_void_p(g.stream)
        timing = time_stream(lambda: g.equity_d(T, None, *outs), gs, 3, warmup=1)
        boards = outs[3].download(np.uint32, T).astype(np.int64)
        holes, board, live = table_spots(g)
        lv = np.array([bin(int(x)).count("1") for x in live], np.int64)
        res["legs"]["table_%dx6" % T] = dict(leg(timing, int(boards.sum()), int((boards * lv).sum())),
                                             turns=np.bincount(g.turn, minlength=5).tolist())
        if T == 65536:
            # ---- forced to the flop: the same cards and live seats with three board cards, and the old way on a subset
            # The old way's evaluator pass on ALL the leg's tables: every (board, live seat) hand enumerated on the host, uploaded once,
            # then pk_eval7_d's device time and the new call, alternating.  NOT counted for the old way: the host enumeration, the
            # upload, and the whole pk_compare_rankings pass it still needs (timed below on `--old-tables` tables, host copies included).
            e = Explicit(holes, board, np.full(T, 3, np.uint8), live, stream)
            words = old_way_hands(holes, board, live)
            wd, od = DeviceBuffer(words.nbytes).upload(words), DeviceBuffer(len(words) * 4)
            time_stream(e.run, stream, 1)
            judger.time_eval7_stream(wd.ptr, len(words), od.ptr, reps=2)
            new, old = [], []
            for _ in range(args.samples):
                old.append(judger.time_eval7_stream(wd.ptr, len(words), od.ptr, reps=1) * 1e3)
                new.append(time_stream(e.run, stream, 1, warmup=0))
            order = int(np.argsort([t[0] for t in new])[len(new) // 2])
            fl = leg((new[order][0], [t[1][0] for t in new], float(np.median([t[2] for t in new])), sum(t[3] for t in new)), *e.evals())
            old_us = float(np.median(old))
            fl.update(old_way_tables=T, old_way_hands=int(len(words)), old_way_eval7_us=round(old_us, 1), old_way_eval7_samples_us=[round(x, 1) for x in old],
                      speedup_vs_old_way_eval7_alone=round(old_us / fl["us"], 2))
            e.free(); wd.free(); od.free()
            k = args.old_tables                       # the comparison pass the old way needs on top, on a subset, as a caller can run it
            import time
            v = np.zeros((k * 666, 6), np.uint32)
            w0 = time.perf_counter()
            judger.compare_rankings_batch((v >> 20).astype(np.uint8), v & 0xFFFFF)
            fl["old_way_compare_rankings_host_call_us_per_%d_tables" % k] = round((time.perf_counter() - w0) * 1e6, 1)
            res["legs"]["flop_65536x6"] = fl
        for b in outs:
            b.free()
        g.close()
    hip.hipStreamDestroy(stream)
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
