#!/usr/bin/env python3
"""Timings of the table snapshots on one MI355X, printed as ONE JSON line: for N = 6 at 65 536 and 1 048 576 tables, save (pk_save_tables_d,
no index array: asynchronous), load (pk_load_tables_d: record check + refusal word read back + scatter), a permuted clone inside one
handle (every table a source and a destination: staged through a blob), a 1 -> T fan-out from another handle, and the same fan-out with
the redeal (PK_OBSERVER_ACTIVE).  Per leg: microseconds per call (HIP events on the handle's stream around one call, warmed up, median of
`--samples`), algorithmic bytes (each record read once and written once: 278 B per table and direction at six seats, plus the 24 B of
in-flight bookkeeping a load / clone zeroes; a fan-out reads its one source record once) and their fraction of the 8 TB/s HBM roofline.

    python tools/snapshot_bench.py [--samples 9] [--tables 65536,1048576]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import pokerl_amd  # noqa: E402
from pokerl_amd import _lib as L  # noqa: E402
from pokerl_amd.hipmem import DeviceBuffer, DeviceEvent  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
N = 6
ZEROED = 4 + 4 + 8 + 8   # owed, mid, env_ctx, env_rew: written by a load / clone


def time_us(g, fn, samples, warmup=3):
    for _ in range(warmup):
        fn()
    g.sync()
    t0, t1 = DeviceEvent(), DeviceEvent()
    out = []
    for _ in range(samples):
        g.record_event(t0.handle)
        fn()
        g.record_event(t1.handle)
        out.append(DeviceEvent.elapsed_ms(t0, t1) * 1e3)
    return float(np.median(out)), [round(x, 1) for x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--tables", default="65536,1048576")
    args = ap.parse_args()
    if pokerl_amd.device_count() < 1:
        sys.exit("snapshot_bench: no MI355X visible (no fallback)")
    rec = pokerl_amd.snapshot_nbytes(N, 1 << 20) // (1 << 20)   # bytes per record (278 at six seats)
    res = dict(tool="snapshot_bench", num_players=N, record_bytes=rec, hbm_roofline_bytes_per_s=HBM_BYTES_PER_S, src=L.source_hash(), legs={})
    rng = np.random.default_rng(0)
    for T in [int(x) for x in args.tables.split(",")]:
        g = pokerl_amd.VecGame(T, num_players=N)
        g.reset()
        g.rollout(40)
        one = pokerl_amd.VecGame(1, num_players=N)
        one.reset()
        blob = DeviceBuffer(pokerl_amd.snapshot_nbytes(N, T))
        perm = DeviceBuffer(T * 4).upload(rng.permutation(T).astype(np.int32))
        zeros = DeviceBuffer(T * 4).upload(np.zeros(T, np.int32))
        g.save_d(blob)
        legs = [
            ("save", lambda: g.save_d(blob), 2 * rec * T),
            ("load", lambda: g.load_d(blob), (2 * rec + ZEROED) * T),
            ("clone_permuted", lambda: g.clone_tables_d(None, perm, T), (2 * rec + ZEROED) * T),
            ("fanout", lambda: g.clone_tables_d(None, zeros, T, src=one), rec + (rec + ZEROED) * T),
            ("fanout_redeal", lambda: g.clone_tables_d(None, zeros, T, src=one, observer="active", nonce=7), rec + (rec + ZEROED) * T),
        ]
        for name, fn, nbytes in legs:
            us, samples = time_us(g, fn, args.samples)
            res["legs"]["%s_%d" % (name, T)] = dict(us=round(us, 1), samples_us=samples, bytes=int(nbytes),
                                                    roofline_fraction=round(nbytes / HBM_BYTES_PER_S / (us * 1e-6), 3))
        for b in (blob, perm, zeros):
            b.free()
        g.close()
        one.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
