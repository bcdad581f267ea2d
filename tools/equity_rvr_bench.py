#!/usr/bin/env python3
"""Timings of range vs range (pk_equity_rvr_d / pk_table_equity_rvr_d) on one MI355X, printed as ONE JSON line and written to
profiles/equity_rvr_bench.json (stamped with the library's source hash).  Legs: 64 full-pool river boards, 64 turn boards, 8 flop boards, one
lone board of each street (latency-bound by construction: one workgroup), and the table form at 65 536 x 6 on a natural mix of turns.  THE
YARDSTICK, in the same run beside every explicit leg: the old way -- the same boards as P (P - 1) / 2 hero spots each through
pk_equity_range_d, `agg` only, DEVICE TIME ONLY, which flatters the old way (the host expansion and its upload are not counted).  And the
streaming evaluator pk_time_eval7_d at 2^28 hands, for scale, alternating with the legs.
Per leg: microseconds per call (a HIP event pair on the call's stream and the host's clock, every shape warmed up, median of `--samples`),
time per board, distinct evaluations (every holding once per completion: C(P, k) * C(P - k, 2)) and evaluations/s; per explicit leg the
ratio new / old.

    python tools/equity_rvr_bench.py [--samples 5]
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
from equity_bench import CANON, EVAL_HANDS, time_stream  # noqa: E402
import kernel_meta  # noqa: E402

H = L.EQ_HOLDINGS


def random_boards(rng, m, nb):
    board = np.zeros((m, 5), np.uint8)
    for i in range(m):
        board[i] = [CANON[c] for c in rng.permutation(52)[:5]]
    return board, np.full(m, nb, np.uint8)


def evals_of(nb):
    p, k = 52 - nb, 5 - nb
    return math.comb(p, k) * math.comb(p - k, 2)


def leg(timing, boards, evals, **more):
    us, each, wall, odd = timing
    return dict(us=round(us, 1), samples_us=each, host_clock_us=round(wall, 1), event_anomalies=odd, boards=boards,
                us_per_board=round(us / max(boards, 1), 3), evals=evals, evals_per_s=round(evals / (us * 1e-6), 0), **more)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "equity_rvr_bench.json"))
    args = ap.parse_args()
    if pokerl_amd.device_count() < 1:
        sys.exit("equity_rvr_bench: no MI355X visible (no fallback)")
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    rng = np.random.default_rng(0)
    res = dict(tool="equity_rvr_bench", src=L.source_hash(), samples=args.samples, legs={})
    meta = kernel_meta.kernels(L.LIB_PATH)["k_rvr"]
    res["k_rvr"] = dict(vgprs=meta["vgprs"], sgprs=meta["sgprs"], lds=meta["lds"], scratch=meta["private_segment"], block=512,
                        workgroups_per_cu_by_lds=163840 // meta["lds"])
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
    # ---- the explicit form, each leg beside the old way on the same boards
    for name, m, nb in (("river_64", 64, 5), ("turn_64", 64, 4), ("flop_8", 8, 3), ("river_1", 1, 5), ("turn_1", 1, 4), ("flop_1", 1, 3)):
        board, nboard = random_boards(rng, m, nb)
        p, k = 52 - nb, 5 - nb
        ins = [DeviceBuffer(x.nbytes).upload(x) for x in (board, nboard)]
        win, tie, tot = (DeviceBuffer(m * H * 8) for _ in range(3))
        boards, status = DeviceBuffer(m * 4), DeviceBuffer(m)

        def run():
            judger.range_vs_range_d(m, ins[0].ptr, ins[1].ptr, weights_d=w_d.ptr, win_d=win.ptr, tie_d=tie.ptr, tot_d=tot.ptr, boards_d=boards.ptr,
                                    status_d=status.ptr, stream=stream)

        stream_rate()
        timing = time_stream(run, stream, args.samples)
        stream_rate()
        assert not status.download(np.uint8, m).any() and (boards.download(np.uint32, m) == math.comb(p - 4, k)).all()
        new = leg(timing, m, m * evals_of(nb))
        got = np.stack([x.download(np.uint64, m * H).reshape(m, H) for x in (win, tie, tot)], axis=2)
        # the old way: every valid holding of every board as a hero spot of its own
        valid = judger.rvr_valid_holdings(board, nboard)
        bi, hi = np.nonzero(valid)
        n = len(bi)
        assert n == m * p * (p - 1) // 2
        old_ins = [DeviceBuffer(x.nbytes).upload(x) for x in (np.ascontiguousarray(judger.HOLDINGS[hi]), np.ascontiguousarray(board[bi]), np.full(n, nb, np.uint8))]
        agg, ob, os_ = DeviceBuffer(n * 24), DeviceBuffer(n * 4), DeviceBuffer(n)

        def run_old():
            judger.range_equity_d(n, *[x.ptr for x in old_ins], weights_d=w_d.ptr, agg_d=agg.ptr, boards_d=ob.ptr, status_d=os_.ptr, stream=stream)

        stream_rate()
        timing = time_stream(run_old, stream, args.samples)
        stream_rate()
        assert not os_.download(np.uint8, n).any()
        assert (agg.download(np.uint64, n * 3).reshape(n, 3) == got[bi, hi]).all()   # the identity, on the timed data
        old_evals = n * (math.comb(p - 2, k) + math.comb(p - 2, k + 2))
        old = leg(timing, m, old_evals, hero_spots=n, note="device time only: the host expansion to hero spots and their upload are not counted")
        new["old_way"] = old
        new["new_over_old_time"] = round(new["us"] / old["us"], 5)
        new["old_over_new_time"] = round(old["us"] / new["us"], 2)
        res["legs"][name] = new
        for b in ins + old_ins + [win, tie, tot, boards, status, agg, ob, os_]:
            b.free()
    # ---- the table form on a natural mix of turns
    T, n = 65536, 6
    g = pokerl_amd.VecGame(T, num_players=n)
    g.reset()
    g.rollout(37)
    turns = np.bincount(g.turn, minlength=5).tolist()
    win, tie, tot = (DeviceBuffer(T * H * 8) for _ in range(3))
    boards, status = DeviceBuffer(T * 4), DeviceBuffer(T)
    gs = C.c_void_p(g.stream)
    stream_rate()
    timing = time_stream(lambda: g.equity_rvr_d(T, None, w_d, False, win, tie, tot, boards, status), gs, args.samples)
    stream_rate()
    st = status.download(np.uint8, T)
    turn = g.turn
    assert ((st == 0) == (turn > 0)).all() and (st[turn == 0] == L.EQ_PREFLOP).all()
    nbs = np.minimum(turn[turn > 0] + 2, 5)
    res["legs"]["table_65536x6"] = leg(timing, int((turn > 0).sum()), int(sum(evals_of(int(b)) for b in nbs)), turns=turns, tables=T)
    for b in (win, tie, tot, boards, status):
        b.free()
    g.close()
    res["eval7_stream_hands_per_s"] = round(float(np.median(stream_rates)), 0)
    res["eval7_stream_samples"] = [round(x, 0) for x in stream_rates]
    hands_d.free(); out_d.free(); w_d.free()
    for v in res["legs"].values():
        v["vs_eval7_stream"] = round(v["evals_per_s"] / res["eval7_stream_hands_per_s"], 4)
    res["faster_than_old_way_on_every_explicit_leg"] = all(v["new_over_old_time"] < 1.0 for v in res["legs"].values() if "old_way" in v)
    hip.hipStreamDestroy(stream)
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
