#!/usr/bin/env python3
"""First timings of the pre-flop solver (pk_solve_preflop_d) on one MI355X, printed as ONE JSON line and written to
profiles/preflop_solver_bench.json (stamped with the library's source hash).  No threshold is set on any of them.
Legs: push_fold_tree(20) at m = 1, 64 and 1 024 spots and preflop_tree(200) at m = 256 (random ranges with zeros and 65 535s, all outputs,
`--iters` iterations).  Per leg: milliseconds per call (a HIP event pair on the call's stream and the host's clock, every shape warmed up,
median of `--samples`), spot-iterations per second and the call's work-space bytes.
The showdown mat-vec's share is an ESTIMATE from a second tree, not a counter: each push / fold leg is timed again on the same tree with the
call removed (player 1 can only fold: four nodes, two fold terminals, no showdown), and the share is 1 - that time / the push / fold time.
Beside them, host_loop: what a user ran before this entry existed -- CFR+ for ONE push / fold spot in numpy float64 on the host, calling
preflop_range_vs_range_batch once per player, showdown node and iteration with the reaches quantised to 16-bit weights -- in milliseconds
per iteration (`--host-iters` iterations, the first not counted).

    python tools/preflop_solver_bench.py [--samples 5] [--iters 64] [--host-iters 9]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import pokerl_amd  # noqa: E402
from pokerl_amd import _lib as L  # noqa: E402
from pokerl_amd import hipmem, solver  # noqa: E402
from pokerl_amd.hipmem import DeviceBuffer  # noqa: E402
from equity_bench import time_stream  # noqa: E402
import kernel_meta  # noqa: E402

H = L.EQ_HOLDINGS
NODE_BYTES = 1344 * 44      # pk::PS_NODE_BYTES: a workgroup's work space per tree node
BOARDS = L.PREFLOP_BOARDS


def random_ranges(rng, m):
    w = rng.integers(0, 65536, (m, 2, H)).astype(np.uint16)
    for row in w.reshape(-1, H):
        row[rng.integers(0, H, 200)] = 0
        row[rng.integers(0, H, 100)] = 65535
    return w


def fold_only_tree(stack):
    """push_fold_tree(stack) without the call: player 0 folds or jams, player 1 can only fold"""
    FF = solver.NO_CHILD
    return solver.RiverTree([0, 2, 1, 3], [[1, 2, FF, FF], [FF] * 4, [3, FF, FF, FF], [FF] * 4], [[1, 2], [1, 2], [stack, 2], [stack, 2]], 0)


def device_leg(tree, ranges, iters, samples, stream):
    m, D = ranges.shape[0], len(tree.decision_nodes)
    rd = DeviceBuffer(ranges.nbytes).upload(ranges)
    strategy, value, br, status = DeviceBuffer(m * D * 4 * H * 2), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m)

    def run():
        solver.solve_preflop_d(m, rd.ptr, tree, iters, strategy_d=strategy.ptr, value_d=value.ptr, br_d=br.ptr, status_d=status.ptr, stream=stream)

    us, each, wall, odd = time_stream(run, stream, samples, warmup=2)
    assert not status.download(np.uint8, m).any()
    v, b = value.download(np.int64, m * 2 * H), br.download(np.int64, m * 2 * H)
    assert (b >= v).all() and v.any()
    for x in (rd, strategy, value, br, status):
        x.free()
    return dict(m=m, iters=iters, nodes=tree.n, showdowns=int((tree.kind == solver.KIND_SHOWDOWN).sum()), ms=round(us * 1e-3, 3),
                samples_ms=[round(x * 1e-3, 3) for x in each], host_clock_ms=round(wall * 1e-3, 3), event_anomalies=odd,
                spot_iterations_per_s=round(m * iters / (us * 1e-6), 0), work_space_bytes=min(m, solver.GRID_MAX) * tree.n * NODE_BYTES)


def host_loop(ranges, stack, iters):
    """CFR+ of one push / fold spot (blinds 1 and 2) as a user of the parent commit's API writes it: float64 numpy on the host, the showdown's
    sums from preflop_range_vs_range_batch, twice per iteration (u16 weights: a reach is quantised to sixteen bits on the way in).
    -> (milliseconds per iteration, iterations timed)."""
    sb, bb = 1.0, 2.0
    w = ranges.astype(np.float64)

    def sums(x):
        """(win, tie, tot) of every holding against the reach vector x, in units of reach"""
        scale = max(float(x.max()), 1e-300) / 65535.0
        r = pokerl_amd.preflop_range_vs_range_batch(np.round(x / scale).astype(np.uint16)[None])
        return tuple(np.asarray(a[0], np.float64) * (scale / BOARDS) for a in (r.win, r.tie, r.tot))

    meet1 = sums(w[1])[2]                                                  # player 1's weight that shares no card, per holding of player 0
    R, A = [np.zeros((2, H)), np.zeros((2, H))], [np.zeros((2, H)), np.zeros((2, H))]
    per_iter = []
    for t in range(1, iters + 1):
        t0 = time.perf_counter()
        sig = []
        for p in (0, 1):
            s = R[p].sum(axis=0)
            sig.append(np.where(s > 0, R[p] / np.where(s > 0, s, 1.0), 0.5))
        jam, call = w[0] * sig[0][1], w[1] * sig[1][1]                     # the reaches at the showdown
        win_c, tie_c, tot_c = sums(call)                                   # player 0's holdings against the callers
        win_j, tie_j, tot_j = sums(jam)                                    # player 1's holdings against the jammers
        v = [[-sb * meet1, bb * (meet1 - tot_c) + stack * (win_c - (tot_c - win_c - tie_c))],
             [-bb * tot_j, stack * (win_j - (tot_j - win_j - tie_j))]]
        for p in (0, 1):
            node = sig[p][0] * v[p][0] + sig[p][1] * v[p][1]
            for a in (0, 1):
                R[p][a] = np.maximum(0.0, R[p][a] + v[p][a] - node)
                A[p][a] += t * w[p] * sig[p][a]
        per_iter.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(per_iter[1:])), len(per_iter) - 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--host-iters", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preflop_solver_bench.json"))
    args = ap.parse_args()
    assert pokerl_amd.device_count() >= 1, "no MI355X visible"
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    pokerl_amd.preflop_matchups()                                           # (the table is built before anything is timed)
    rng = np.random.default_rng(0)
    ranges = random_ranges(rng, 1024)
    meta = kernel_meta.kernels(L.LIB_PATH)["k_preflop_solve"]
    res = dict(tool="preflop_solver_bench", src=L.source_hash(), samples=args.samples,
               kernel=dict(vgprs=meta.get("vgprs"), lds=meta.get("lds"), scratch=meta.get("private_segment")), legs={})
    pf, nocall = solver.push_fold_tree(20), fold_only_tree(20)
    for m in (1, 64, 1024):
        leg = device_leg(pf, np.ascontiguousarray(ranges[:m]), args.iters, args.samples, stream)
        without = device_leg(nocall, np.ascontiguousarray(ranges[:m]), args.iters, args.samples, stream)
        leg["without_the_call_ms"] = without["ms"]
        leg["showdown_share_estimate"] = round(1.0 - without["ms"] / leg["ms"], 4)
        res["legs"]["push_fold_m_%d" % m] = leg
    res["legs"]["preflop_tree_200_m_256"] = device_leg(solver.preflop_tree(200), np.ascontiguousarray(ranges[:256]), args.iters, args.samples, stream)
    ms, n = host_loop(ranges[0], 20.0, args.host_iters)
    res["host_loop"] = dict(m=1, iterations_timed=n, ms_per_iteration=round(ms, 3), range_vs_range_calls_per_iteration=2,
                            note="numpy float64 CFR+ on the host, preflop_range_vs_range_batch per sum and iteration: the parent commit's API")
    one = res["legs"]["push_fold_m_1"]
    res["host_loop"]["device_ms_per_iteration_m_1"] = round(one["ms"] / one["iters"], 4)
    assert hip.hipStreamDestroy(stream) == 0
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
