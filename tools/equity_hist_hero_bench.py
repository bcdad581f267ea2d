#!/usr/bin/env python3
"""Timings of the hero strength histogram (pk_equity_hist_hero_d / pk_table_equity_hist_hero_d) on one MI355X, printed as ONE JSON line and
written to profiles/equity_hist_hero_bench.json (stamped with the library's source hash).  Device time: a HIP event pair on the call's
stream, the median of `--samples` (7).  Legs:
  (a) table_hist     the table form on 65 536 x 6 tables at the natural mix of turns a random rollout leaves, 10 bins, hist only;
      table_range    BESIDE IT, in the same run, on the same tables: pk_table_equity_range_d, agg only -- the same enumeration without the
                     per-completion counters, so a / range is the price of the weights going to the completion;
  (b) table_label    the same tables with K = 256 centroids, label only (the rows stay in the work space);
  (c) flop_4096      4 096 explicit full-pool flop spots, 10 bins, hist only;
      old_way        BESIDE IT: the public form pk_equity_hist_d on the public boards of 8 of those spots (1 326 rows each, one of them
                     wanted), SCALED by 4 096 / 8 and labelled as scaled; the tool asserts that the wanted rows equal the new form's;
  (d) flop_1         one lone flop spot.

    python tools/equity_hist_hero_bench.py [--samples 7] [--tables 65536]
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
SETS = {0: 0, 1: 178365, 2: 15180, 3: 1035}      # C(47, 4), C(46, 3), C(45, 2): seven-card sets of a full-pool spot per turn


def leg(timing, spots, sets):
    us, each, wall, odd = timing
    return dict(spots=spots, device_us=round(us, 1), samples_us=each, host_clock_us=round(wall, 1), event_anomalies=odd, sets=sets,
                sets_per_s=round(sets / (us * 1e-6), 0) if us > 0 else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--tables", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "equity_hist_hero_bench.json"))
    args = ap.parse_args()
    if pokerl_amd.device_count() < 1:
        sys.exit("equity_hist_hero_bench: no MI355X visible (no fallback)")
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    rng = np.random.default_rng(0)
    bins, K = 10, 256
    res = dict(tool="equity_hist_hero_bench", src=L.source_hash(), samples=args.samples, bins=bins, legs={})
    meta = kernel_meta.kernels(L.LIB_PATH)
    for k in ("k_hero_hist", "k_eqr"):
        d = meta[k]
        res[k] = dict(vgprs=d["vgprs"], agprs=d["agprs"], sgprs=d["sgprs"], lds=d["lds"], scratch=d["private_segment"], block=512,
                      workgroups_per_cu_by_lds=163840 // d["lds"])
    weights = rng.integers(0, 65536, H).astype(np.uint16)
    w_d = DeviceBuffer(weights.nbytes).upload(weights)
    cen = np.sort(rng.integers(0, 65536, (K, bins)), axis=1).astype(np.uint16)
    cen[:, -1] = 65535
    cen_d = DeviceBuffer(cen.nbytes).upload(cen)

    # ---- (a), (b): the table form on the natural mix of turns
    T, N = args.tables, 6
    g = pokerl_amd.VecGame(T, num_players=N, seed=1)
    g.reset()
    g.rollout(37, policy=0, auto_reset=True, fused=True)
    g.sync()
    turn = g.turn
    mix = {int(t): int((turn == t).sum()) for t in range(4)}
    sets = sum(SETS[t] * n for t, n in mix.items())
    g.set_stream(stream)
    hist_d, agg_d, lab_d, st_d = DeviceBuffer(T * bins * 2), DeviceBuffer(T * 3 * 8), DeviceBuffer(T * 2), DeviceBuffer(T)
    a = time_stream(lambda: g.equity_hist_hero_d(weights_d=w_d, bins=bins, hist_d=hist_d, status_d=st_d), stream, args.samples)
    status = st_d.download(np.uint8, T)
    assert ((status == 0) == (turn > 0)).all()
    hist = hist_d.download(np.uint16, T * bins).reshape(T, bins)
    r = time_stream(lambda: g.equity_range_d(weights_d=w_d, agg_d=agg_d), stream, args.samples)
    b = time_stream(lambda: g.equity_hist_hero_d(weights_d=w_d, bins=bins, k=K, centroids_d=cen_d, label_d=lab_d), stream, args.samples)
    label = lab_d.download(np.uint16, T)
    want, _ = judger.assign_histograms(hist, cen)
    assert (label == want).all()                                     # the label-only call against assign on the rows of the hist-only call
    res["tables"] = dict(tables=T, seats=N, per_turn=mix)
    res["legs"]["table_hist"] = leg(a, T, sets)
    res["legs"]["table_range"] = dict(leg(r, T, sets), note="pk_table_equity_range_d, agg only, the same tables in the same run")
    res["legs"]["table_label"] = dict(leg(b, T, sets), K=K, note="label only: the rows stay in the work space")
    res["ratio_hist_over_range"] = round(a[0] / r[0], 3)
    res["ratio_label_over_hist"] = round(b[0] / a[0], 3)
    g.use_own_stream()
    g.close()
    for x in (hist_d, agg_d, lab_d, st_d):
        x.free()

    # ---- (c), (d): explicit full-pool flop spots; the old way on 8 of them
    m = 4096
    hero, board = np.zeros((m, 2), np.uint8), np.zeros((m, 5), np.uint8)
    for i in range(m):
        deck = rng.permutation(52)
        hero[i], board[i] = [CANON[c] for c in deck[:2]], [CANON[c] for c in deck[2:7]]
    nboard = np.full(m, 3, np.uint8)
    ins = [DeviceBuffer(x.nbytes).upload(x) for x in (hero, board, nboard)]
    hist_d, st_d = DeviceBuffer(m * bins * 2), DeviceBuffer(m)
    for name, n in (("flop_4096", m), ("flop_1", 1)):
        t = time_stream(lambda: judger.hero_histogram_d(n, ins[0].ptr, ins[1].ptr, ins[2].ptr, weights_d=w_d.ptr, bins=bins, hist_d=hist_d.ptr,
                                                        status_d=st_d.ptr, stream=stream), stream, args.samples)
        assert not st_d.download(np.uint8, n).any()
        res["legs"][name] = leg(t, n, n * SETS[1])
    judger.hero_histogram_d(m, ins[0].ptr, ins[1].ptr, ins[2].ptr, weights_d=w_d.ptr, bins=bins, hist_d=hist_d.ptr, stream=stream)
    assert hip.hipStreamSynchronize(stream) == 0
    new = hist_d.download(np.uint16, m * bins).reshape(m, bins)
    few = 8
    pub_d, pst_d = DeviceBuffer(few * H * bins * 2), DeviceBuffer(few)
    o = time_stream(lambda: judger.strength_histogram_d(few, ins[1].ptr, ins[2].ptr, weights_d=w_d.ptr, bins=bins, hist_d=pub_d.ptr, status_d=pst_d.ptr,
                                                        stream=stream), stream, args.samples)
    pub = pub_d.download(np.uint16, few * H * bins).reshape(few, H, bins)
    for i in range(few):
        assert (pub[i, judger.holding_index(int(hero[i, 0]), int(hero[i, 1]))] == new[i]).all()      # the row identity, on the timed data
    scaled = o[0] * m / few
    res["legs"]["old_way"] = dict(boards_measured=few, device_us_measured=round(o[0], 1), samples_us=o[1], scaled_to_spots=m, device_us_scaled=round(scaled, 1),
                                  note="pk_equity_hist_d on the public boards of 8 of the 4 096 spots, SCALED by 512: one row of 1 326 is wanted")
    res["ratio_old_scaled_over_new"] = round(scaled / res["legs"]["flop_4096"]["device_us"], 1)
    for x in ins + [hist_d, st_d, pub_d, pst_d, w_d, cen_d]:
        x.free()
    hip.hipStreamDestroy(stream)
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
