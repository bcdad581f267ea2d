#!/usr/bin/env python3
"""Timings of the histogram clustering (pk_hist_cluster_d) on one MI355X, printed as ONE JSON line and written to
profiles/hist_cluster_bench.json (stamped with the library's source hash).  One process; every figure is the median of `--samples` HIP-event
pairs on the call's stream.  TIME PER ITERATION = (a call of 1 + EXTRA iterations - a call of 1 iteration) / EXTRA: the quantisation, the
packing and the final assign cancel.  Legs: 2 000 000 synthetic rows of 32 bins at K = 1 024 and 4 096; the 1 326 x 50 rows of 50 turn boards
at 10 bins (computed by pk_equity_hist_d, never copied to the host), K = 256; one lone board, K = 16.  Beside each leg:
  old_way   the numpy assignment of tests/hist_cluster_spec.py on a slice of 20 000 rows (fewer where the leg has fewer), SCALED by n / slice
            and labelled so -- an assignment alone, so it flatters the old way;
  floor     n * K * ceil(nbins / 2) / 64 wave-instructions against the issue rate of v_sad_u16: the row `v_sad_u16 (sgpr operand) ilp8`, 8 waves
            per SIMD, of tools/microbench/valu_rates.hip when `--valu-rates <its binary>` is given, else the nominal 1 024 SIMDs x 2.4 GHz / 4.

    python tools/hist_cluster_bench.py [--samples 7] [--valu-rates /tmp/valu_rates] [--legs big1024,big4096,turn,lone]
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import pokerl_amd  # noqa: E402
from pokerl_amd import _lib as L  # noqa: E402
from pokerl_amd import hipmem, judger  # noqa: E402
from pokerl_amd.hipmem import DeviceBuffer  # noqa: E402
from equity_bench import CANON, time_stream  # noqa: E402
import hist_cluster_spec as CS  # noqa: E402
import kernel_meta  # noqa: E402

EXTRA = 2
NOMINAL = 1024 * 2.4e9 / 4            # wave-instructions per second: 1 024 SIMDs, one wave-instruction per four cycles


def sad_rate(exe):
    if not exe:
        return NOMINAL, "nominal: 1 024 SIMDs x 2.4 GHz / 4 cycles (v_sad_u16 not measured in this run)"
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=300).stdout
    row = next(ln for ln in out.splitlines() if ln.startswith("v_sad_u16 (sgpr operand)") and " ilp8 " in ln)
    return float(re.findall(r"8w/SIMD\s+[\d.]+ cyc\s+([\d.]+) Ginst/s", row)[0]) * 1e9, row.strip()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--valu-rates")
    ap.add_argument("--legs", default="big1024,big4096,turn,lone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hist_cluster_bench.json"))
    args = ap.parse_args()
    if pokerl_amd.device_count() < 1:
        sys.exit("hist_cluster_bench: no MI355X visible (no fallback)")
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    rng = np.random.default_rng(0)
    rate, rate_note = sad_rate(args.valu_rates)
    meta = kernel_meta.kernels(L.LIB_PATH)
    res = dict(tool="hist_cluster_bench", src=L.source_hash(), samples=args.samples, extra_iterations=EXTRA, sad_wave_instructions_per_s=rate,
               sad_rate_source=rate_note, legs={},
               taken=dict(workgroup=256, rows_per_lane=1, centroid_delivery="scalar loads from the packed [K][16] array", grid_max=2048,
                          note="TAKEN, not compared: no other workgroup width, rows per lane or LDS-broadcast delivery has been timed"),
               k_cl_assign={p: dict(vgprs=meta["k_cl_assign<%d>" % p]["vgprs"], sgprs=meta["k_cl_assign<%d>" % p]["sgprs"]) for p in (5, 16)})
    wanted = args.legs.split(",")
    legs = [("big1024", 2000000, 32, 1024), ("big4096", 2000000, 32, 4096), ("turn", 50 * L.EQ_HOLDINGS, 10, 256), ("lone", L.EQ_HOLDINGS, 10, 16)]
    big_d = None
    for name, n, bins, K in legs:
        if name not in wanted:
            continue
        if name.startswith("big"):
            if big_d is None:
                big_d = DeviceBuffer(n * bins * 2).upload(CS.latent_rows(rng, n, bins, mass=1081, shapes=64, empty_frac=0.1))
            hist_d = big_d
        else:
            m = n // L.EQ_HOLDINGS
            board = np.zeros((m, 5), np.uint8)
            for i in range(m):
                board[i] = [CANON[c] for c in rng.permutation(52)[:5]]
            ins = [DeviceBuffer(x.nbytes).upload(x) for x in (board, np.full(m, 4, np.uint8))]
            hist_d = DeviceBuffer(n * bins * 2)
            judger.strength_histogram_d(m, ins[0].ptr, ins[1].ptr, bins=bins, hist_d=hist_d.ptr, stream=stream)
            assert hip.hipStreamSynchronize(stream) == 0
        seeds_d, cen_d, label_d = DeviceBuffer(K * bins * 2), DeviceBuffer(K * bins * 2), DeviceBuffer(n * 2)
        in_d, ch_d = DeviceBuffer((2 + EXTRA) * 8), DeviceBuffer((1 + EXTRA) * 4)
        t0 = time.perf_counter()
        judger.seed_histogram_centroids_d(n, bins, hist_d.ptr, K, seeds_d.ptr, nonce=1, stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        seed_ms = (time.perf_counter() - t0) * 1e3

        def run(iters):
            def f():
                assert hip.hipMemcpyAsync(cen_d.ptr, seeds_d.ptr, C.c_size_t(K * bins * 2), 3, stream) == 0   # every sample starts from the seeds
                judger.cluster_histograms_d(n, bins, hist_d.ptr, K, cen_d.ptr, iters, label_d.ptr, None, in_d.ptr, ch_d.ptr, stream=stream)
            return f
        one = time_stream(run(1), stream, args.samples)
        more = time_stream(run(1 + EXTRA), stream, args.samples)
        per_iter_us = (more[0] - one[0]) / EXTRA
        inertia, changed = in_d.download(np.uint64, 2 + EXTRA), ch_d.download(np.uint32, 1 + EXTRA)
        sads = n * K * ((bins + 1) // 2) / 64.0
        floor_us = sads / rate * 1e6
        # the old way: numpy, on a slice
        cut = min(n, 20000)
        rows = DeviceBuffer.download(hist_d, np.uint16, cut * bins).reshape(cut, bins)
        cen = seeds_d.download(np.uint16, K * bins).reshape(K, bins)
        q, empty = CS.quant(rows)
        t0 = time.perf_counter()
        want_l, want_d = CS.assign(q, empty, cen)
        old_us = (time.perf_counter() - t0) * 1e6 * n / cut
        got_l = np.zeros(cut, np.uint16)
        got_d = np.zeros(cut, np.uint32)
        L.check(L.lib().pk_hist_cluster_assign(0, cut, bins, L.ptr(rows), K, L.ptr(cen), L.ptr(got_l), L.ptr(got_d)))
        assert np.array_equal(got_l, want_l) and np.array_equal(got_d, want_d)     # the timed old way and the device agree on the slice
        res["legs"][name] = dict(rows=n, bins=bins, K=K, call_1_iteration_us=round(one[0], 1), call_1_iteration_samples_us=one[1],
                                 call_more_iterations_us=round(more[0], 1), call_more_iterations_samples_us=more[1], event_anomalies=one[3] + more[3],
                                 per_iteration_us=round(per_iter_us, 1), seeding_wall_ms=round(seed_ms, 1), seeding_launches=1 + 2 * K,
                                 inertia=[int(x) for x in inertia], changed=[int(x) for x in changed],
                                 floor_us=round(floor_us, 1), fraction_of_floor_reached=round(floor_us / per_iter_us, 3) if per_iter_us > 0 else None,
                                 old_way=dict(us_scaled=round(old_us, 1), slice_rows=cut, scaled_by=round(n / cut, 2),
                                              note="numpy assignment of tests/hist_cluster_spec.py on the slice, wall clock, SCALED by rows / slice"),
                                 old_over_new=round(old_us / per_iter_us, 1) if per_iter_us > 0 else None)
        for b in (seeds_d, cen_d, label_d, in_d, ch_d):
            b.free()
        if not name.startswith("big"):
            for b in ins + [hist_d]:
                b.free()
        print(name, json.dumps(res["legs"][name]), flush=True)
    hip.hipStreamDestroy(stream)
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
