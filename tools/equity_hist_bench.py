#!/usr/bin/env python3
"""Timings of the strength histograms (pk_equity_hist_d) on one MI355X, printed as ONE JSON line and written to
profiles/equity_hist_bench.json (stamped with the library's source hash).  Legs: one lone flop board, one lone turn board, and batches of 8
flop and 64 turn boards, each at 10 and 32 bins.  THE YARDSTICK, in the same run beside every leg: the old way -- the same boards as
C(P, k) completed river boards each through pk_equity_rvr (the host call: its staging, its 3 x 10 608 B per river board back to the host)
plus the host binning in numpy, wall clock.  The new way is timed twice: device time of pk_equity_hist_d (a HIP event pair on the call's
stream, median of `--samples`) and the wall clock of the host call pk_equity_hist, which is what the old way's wall clock compares with.
The tool asserts that the two ways agree bit for bit on the timed data.

    python tools/equity_hist_bench.py [--samples 5]
"""
import argparse
import ctypes as C
import itertools
import json
import math
import os
import sys
import time

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
PAIR_A = np.array([a for b in range(52) for a in range(b)])
PAIR_B = np.array([b for b in range(52) for a in range(b)])


def random_boards(rng, m, nb):
    board = np.zeros((m, 5), np.uint8)
    for i in range(m):
        board[i] = [CANON[c] for c in rng.permutation(52)[:5]]
    return board, np.full(m, nb, np.uint8)


def old_way(board, nb, weights, bins):
    """One board: every completed river board through pk_equity_rvr, then the one-hot bins summed on the host."""
    index = {v: k for k, v in enumerate(CANON)}
    pool = [c for c in range(52) if c not in {index[int(x)] for x in board[:nb]}]
    combos = list(itertools.combinations(pool, 5 - nb))
    n = len(combos)
    rivers = np.zeros((n, 5), np.uint8)
    rivers[:, :nb] = board[:nb]
    live = np.zeros((n, H), bool)
    free = np.zeros(52, bool)
    free[pool] = True
    for i, comp in enumerate(combos):
        rivers[i, nb:] = [CANON[c] for c in comp]
        f = free.copy()
        f[list(comp)] = False
        live[i] = f[PAIR_A] & f[PAIR_B]
    r = judger.range_vs_range_batch(rivers, np.full(n, 5, np.uint8), None, weights)
    win, tie, tot = (np.asarray(x).astype(np.int64) for x in (r.win, r.tie, r.tot))
    b = np.minimum(bins - 1, bins * (2 * win + tie) // np.where(tot > 0, 2 * tot, 1))
    hist = np.zeros((H, bins), np.int64)
    rows, cols = np.nonzero(live & (tot > 0))
    np.add.at(hist, (cols, b[rows, cols]), 1)
    return hist.astype(np.uint16), (live & (tot == 0)).sum(axis=0).astype(np.uint16), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "equity_hist_bench.json"))
    args = ap.parse_args()
    if pokerl_amd.device_count() < 1:
        sys.exit("equity_hist_bench: no MI355X visible (no fallback)")
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    rng = np.random.default_rng(0)
    res = dict(tool="equity_hist_bench", src=L.source_hash(), samples=args.samples, legs={})
    meta = kernel_meta.kernels(L.LIB_PATH)["k_hist"]
    res["k_hist"] = dict(vgprs=meta["vgprs"], sgprs=meta["sgprs"], lds=meta["lds"], scratch=meta["private_segment"], block=512,
                         workgroups_per_cu_by_lds=163840 // meta["lds"])
    weights = rng.integers(0, 65536, H).astype(np.uint16)
    w_d = DeviceBuffer(weights.nbytes).upload(weights)
    for name, m, nb in (("flop_1", 1, 3), ("turn_1", 1, 4), ("flop_8", 8, 3), ("turn_64", 64, 4)):
        board, nboard = random_boards(rng, m, nb)
        p, k = 52 - nb, 5 - nb
        ins = [DeviceBuffer(x.nbytes).upload(x) for x in (board, nboard)]
        for bins in (10, 32):
            hist, void = DeviceBuffer(m * H * bins * 2), DeviceBuffer(m * H * 2)
            comp, status = DeviceBuffer(m * 4), DeviceBuffer(m)

            def run():
                judger.strength_histogram_d(m, ins[0].ptr, ins[1].ptr, weights_d=w_d.ptr, bins=bins, hist_d=hist.ptr, void_d=void.ptr,
                                            completions_d=comp.ptr, status_d=status.ptr, stream=stream)

            us, each, wall, odd = time_stream(run, stream, args.samples)
            assert not status.download(np.uint8, m).any() and (comp.download(np.uint32, m) == math.comb(p - 2, k)).all()
            got_h, got_v = hist.download(np.uint16, m * H * bins).reshape(m, H, bins), void.download(np.uint16, m * H).reshape(m, H)
            judger.strength_histogram_batch(board, nboard, None, weights, bins)                         # (warm)
            host = []
            for _ in range(args.samples):
                t0 = time.perf_counter()
                r = judger.strength_histogram_batch(board, nboard, None, weights, bins)
                host.append((time.perf_counter() - t0) * 1e6)
            assert (r.hist == got_h).all() and (r.void == got_v).all()
            t0 = time.perf_counter()
            rivers = 0
            for i in range(m):
                oh, ov, n = old_way(board[i], nb, weights, bins)
                rivers += n
                assert (oh == got_h[i]).all() and (ov == got_v[i]).all()                                # the identity of section 3.5, on the timed data
            old_us = (time.perf_counter() - t0) * 1e6
            evals = m * math.comb(p, k) * math.comb(p - k, 2)
            res["legs"]["%s_bins%d" % (name, bins)] = dict(
                boards=m, bins=bins, device_us=round(us, 1), samples_us=each, host_clock_us=round(wall, 1), event_anomalies=odd,
                device_us_per_board=round(us / m, 2), evals=evals, evals_per_s=round(evals / (us * 1e-6), 0),
                host_call_us=round(float(np.median(host)), 1),
                old_way=dict(us=round(old_us, 1), river_spots=rivers, bytes_to_host=rivers * 3 * H * 8,
                             note="one run, wall clock: pk_equity_rvr on every completed river board (host call) + numpy binning"),
                old_over_new_host_call=round(old_us / float(np.median(host)), 2))
            for b in (hist, void, comp, status):
                b.free()
        for b in ins:
            b.free()
    w_d.free()
    hip.hipStreamDestroy(stream)
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
