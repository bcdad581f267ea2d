#!/usr/bin/env python3
"""Timings of the pre-flop matchups (pk_preflop_count_d / pk_table_equity_preflop_d / pk_equity_rvr_preflop_d) on one MI355X, printed as ONE
JSON line and written to profiles/preflop_bench.json (stamped with the library's source hash).  Legs, alternating in one run:
  build        the full table: pk_preflop_count_d over all 2 598 960 boards into the caller's arrays (what the first use of the resident table runs);
  old_way      THE YARDSTICK: 16 384 random heads-up pre-flop matchups through pk_equity_d, extrapolated to the 812 175 unordered disjoint
               matchups of the table (device time only: their host arrays and uploads are not counted);
  table_65536x6   pk_table_equity_preflop_d on 65 536 tables of six seats, the seat to act, aggregates only;
  rvr_1, rvr_1024 pk_equity_rvr_preflop_d on 1 and 1 024 weight rows.
Per leg: microseconds per call (a HIP event pair on the call's stream and the host's clock, every shape warmed up, median of `--samples`).
The build and the old way alternate twice: the faster of each one's two medians is the leg's figure (with its samples), the slower is
kept beside it as `other_run_us`.
The count pass's registers, LDS and instruction mix are read off the code object.

    python tools/preflop_bench.py [--samples 5]
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
import kernel_meta  # noqa: E402

H = L.EQ_HOLDINGS
UNORDERED_MATCHUPS = 812175          # C(52, 2) * C(50, 2) / 2
PAIR_BOARDS_TOTAL = H * H * L.PREFLOP_ALL_BOARDS      # pair-boards the count pass walks (every ordered pair, the pad aside)


def leg(timing, **more):
    us, each, wall, odd = timing
    return dict(us=round(us, 1), samples_us=each, host_clock_us=round(wall, 1), event_anomalies=odd, **more)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preflop_bench.json"))
    args = ap.parse_args()
    if pokerl_amd.device_count() < 1:
        sys.exit("preflop_bench: no MI355X visible (no fallback)")
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    rng = np.random.default_rng(0)
    res = dict(tool="preflop_bench", src=L.source_hash(), samples=args.samples, chunk=int(os.environ.get("PK_PFM_CHUNK", 16384)), legs={})
    ks = kernel_meta.kernels(L.LIB_PATH)
    for name in ("k_pfm_count<false>", "k_pfm_rank"):
        meta = ks[name]
        res[name] = dict(vgprs=meta["vgprs"], sgprs=meta["sgprs"], lds=meta["lds"], scratch=meta["private_segment"])
    M = judger.preflop_matchups()                                     # (the resident table: built here, outside every timed region)
    # ---- the build and the old way, alternating
    win_d, tie_d = DeviceBuffer(H * H * 4), DeviceBuffer(H * H * 4)
    m = 16384
    holes = np.zeros((m, 2, 2), np.uint8)
    hs = np.zeros((m, 2), np.int64)
    for i in range(m):
        c = [int(x) for x in rng.permutation(52)[:4]]
        holes[i] = np.array([CANON[x] for x in c], np.uint8).reshape(2, 2)
        hs[i] = [judger.holding_index(int(holes[i, 0, 0]), int(holes[i, 0, 1])), judger.holding_index(int(holes[i, 1, 0]), int(holes[i, 1, 1]))]
    ins = [DeviceBuffer(x.nbytes).upload(x) for x in (holes, np.zeros((m, 5), np.uint8), np.zeros(m, np.uint8), np.full(m, 3, np.uint16))]
    ew, et, eb, es = DeviceBuffer(m * 8), DeviceBuffer(m * 8), DeviceBuffer(m * 4), DeviceBuffer(m)

    def build():
        judger.preflop_counts_d(0, L.PREFLOP_ALL_BOARDS, win_d.ptr, tie_d.ptr, device=0, stream=stream)

    def old():
        judger.showdown_equity_d(2, m, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, win_d=ew.ptr, tie_d=et.ptr, boards_d=eb.ptr, status_d=es.ptr, stream=stream)

    b1 = time_stream(build, stream, args.samples)
    o1 = time_stream(old, stream, args.samples)
    b2 = time_stream(build, stream, args.samples)
    o2 = time_stream(old, stream, args.samples)
    assert win_d.download(np.uint32, H * H).tobytes() == M.win.tobytes() and tie_d.download(np.uint32, H * H).tobytes() == M.tie.tobytes()
    assert not es.download(np.uint8, m).any()
    got = ew.download(np.uint32, m * 2).reshape(m, 2)
    assert (got[:, 0] == M.win[hs[:, 0], hs[:, 1]]).all() and (got[:, 1] == M.win[hs[:, 1], hs[:, 0]]).all()   # the identity, on the timed data
    bt = b1 if b1[0] <= b2[0] else b2
    ot = o1 if o1[0] <= o2[0] else o2
    res["legs"]["build"] = leg(bt, other_run_us=round(max(b1[0], b2[0]), 1), boards=L.PREFLOP_ALL_BOARDS, pair_boards=PAIR_BOARDS_TOTAL,
                               pair_boards_per_s=round(PAIR_BOARDS_TOTAL / (bt[0] * 1e-6), 0))
    res["legs"]["old_way"] = leg(ot, other_run_us=round(max(o1[0], o2[0]), 1), matchups=m, extrapolated_to=UNORDERED_MATCHUPS,
                                 extrapolated_us=round(ot[0] * UNORDERED_MATCHUPS / m, 1),
                                 note="device time only: the host arrays of the matchups and their upload are not counted")
    res["old_over_new_time"] = round(res["legs"]["old_way"]["extrapolated_us"] / res["legs"]["build"]["us"], 2)
    res["build_beats_the_old_way"] = res["old_over_new_time"] > 1.0
    for b in ins + [ew, et, eb, es, win_d, tie_d]:
        b.free()
    # ---- the table form
    T, n = 65536, 6
    g = pokerl_amd.VecGame(T, num_players=n)
    g.reset()
    g.rollout(37)
    weights = rng.integers(0, 65536, H).astype(np.uint16)
    w_d = DeviceBuffer(weights.nbytes).upload(weights)
    agg, boards, status = DeviceBuffer(T * 24), DeviceBuffer(T * 4), DeviceBuffer(T)
    gs = C.c_void_p(g.stream)
    timing = time_stream(lambda: g.equity_preflop_d(T, None, "active", w_d, False, agg, None, None, boards, status), gs, args.samples)
    assert not status.download(np.uint8, T).any()
    res["legs"]["table_65536x6"] = leg(timing, tables=T, us_per_table=round(timing[0] / T, 4), turns=np.bincount(g.turn, minlength=5).tolist())
    for b in (agg, boards, status):
        b.free()
    g.close()
    # ---- range vs range
    for m in (1, 1024):
        w = rng.integers(0, 65536, (m, H)).astype(np.uint16)
        wd = DeviceBuffer(w.nbytes).upload(w)
        out = [DeviceBuffer(m * H * 8) for _ in range(3)]
        timing = time_stream(lambda: judger.preflop_range_vs_range_d(m, wd.ptr, out[0].ptr, out[1].ptr, out[2].ptr, stream=stream), stream, args.samples)
        got = out[0].download(np.uint64, m * H).reshape(m, H)
        assert (got[0] == w[0].astype(np.uint64) @ M.win.astype(np.uint64).T).all()
        res["legs"]["rvr_%d" % m] = leg(timing, rows=m, us_per_row=round(timing[0] / m, 3))
        for b in out + [wd]:
            b.free()
    w_d.free()
    hip.hipStreamDestroy(stream)
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
