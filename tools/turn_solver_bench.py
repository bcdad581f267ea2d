#!/usr/bin/env python3
"""Timings of the turn solver (pk_solve_turn_d) on one MI355X, printed as ONE JSON line and written to profiles/turn_solver_bench.json
(stamped with the library's source hash).  Legs: m = 256 and 1 024 full-pool turn subgames (random boards, random ranges with zeros and
65 535s), turn_tree(100, 400, (1.0,), 1), 64 iterations; outputs strategy, value, br, status (river_strategy is not asked for).  Per leg:
milliseconds per call (a HIP event pair on the call's stream and the host's clock, every shape warmed up, median of `--samples`),
microseconds per spot-iteration, the call's work-space bytes -- and the RATIO to the yardstick a user has without the turn solver:
pk_solve_river_d on the 48 x m river boards (each turn board plus each of its river cards, the same ranges) with the river subtree
river_tree(100, 400, (1.0,), 1) and the same iteration count, outputs value, br, status.  The yardstick is the cost of the inner work
alone: it has no chance node, so it computes no turn strategy.

    python tools/turn_solver_bench.py [--samples 3] [--m 256 1024] [--iters 64]

--trees K measures the tree-per-spot entry (pk_solve_turn_trees_d) instead, as tools/river_solver_bench.py --trees
does, and merges its legs into profiles/solver_trees_bench.json under "turn": the same spots through K single-tree calls (one per tree, on
its run of spots) and through ONE tree-per-spot call; K = 1 is the price of the indirection, K > 1 uses turn_tree(60 + 10 k, 400, (1.0,), 1).

    python tools/turn_solver_bench.py --trees 1 --m 256

--lock {none,one,all} measures the locked entry (pk_solve_turn_locked_d) as tools/river_solver_bench.py --lock does,
on the ordinary legs' spots and tree, and merges its legs into profiles/solver_lock_bench.json under "turn": nothing locked against
pk_solve_turn_trees_d with that one tree; player 1's rows of both levels locked to a plain solution of the same spots; every row locked
with no iteration.  river_locked takes 6.6 MB of device memory a spot.

    python tools/turn_solver_bench.py --lock none --m 256

--resolve {none,at} measures the re-solving entry (pk_solve_turn_resolve_d) as tools/river_solver_bench.py --resolve
does, and merges its legs into profiles/solver_resolve_bench.json under "turn": none of the new arguments against pk_solve_turn_locked_d
with nothing locked; the root reaches from `reach` and the node outputs at a river-level node under one river card.

    python tools/turn_solver_bench.py --resolve none --m 256
--resume {none,fresh,chain} measures the resuming entry (pk_solve_turn_resume_d) as tools/river_solver_bench.py --resume
does, and merges its legs into profiles/solver_resume_bench.json under "turn"; the state is 53 MB a spot on this tree.
    python tools/turn_solver_bench.py --resume chain --m 256
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
from pokerl_amd import hipmem, solver  # noqa: E402
from pokerl_amd.hipmem import DeviceBuffer  # noqa: E402
from equity_bench import CANON, time_stream  # noqa: E402
import kernel_meta  # noqa: E402

H = L.EQ_HOLDINGS
TABLE_BYTES, TURN_NODE_BYTES, RIVER_NODE_BYTES = 423936, 50688, 866048        # pk_turn_solver.hpp


def subgames(rng, m):
    """m turn boards, their 48 river boards each [m * 48, 5], ranges [m, 2, 1326]"""
    board, river = np.zeros((m, 4), np.uint8), np.zeros((m, 48, 5), np.uint8)
    for i in range(m):
        deck = rng.permutation(52)
        board[i] = [CANON[c] for c in deck[:4]]
        river[i, :, :4] = board[i]
        river[i, :, 4] = [CANON[c] for c in sorted(deck[4:])]
    ranges = rng.integers(0, 65536, (m, 2, H)).astype(np.uint16)
    for row in ranges.reshape(-1, H):
        row[rng.integers(0, H, 200)] = 0
        row[rng.integers(0, H, 100)] = 65535
    return board, river.reshape(m * 48, 5), ranges


def at(buf, offset):
    """a device pointer `offset` bytes into a DeviceBuffer"""
    return C.c_void_p(buf.ptr.value + offset)


def trees_legs(args, stream, res):
    """--trees K (the module's docstring)"""
    K = args.trees
    rng = np.random.default_rng(0)
    board, _, ranges = subgames(rng, max(args.m))
    trees = [solver.turn_tree(100, 400, (1.0,), 1)] if K == 1 else [solver.turn_tree(60 + 10 * k, 400, (1.0,), 1) for k in range(K)]
    D = max(len(t.decision_nodes) for t in trees)
    for m in args.m:
        tree_of = (np.arange(m) % K).astype(np.uint32)
        order = np.argsort(tree_of, kind="stable")                            # the spots grouped by tree: K runs of consecutive spots
        of = np.ascontiguousarray(tree_of[order])
        ins = [DeviceBuffer(x.nbytes).upload(x) for x in (np.ascontiguousarray(board[:m][order]), np.ascontiguousarray(ranges[:m][order]), of)]
        strategy, value, br, status = DeviceBuffer(m * D * 4 * H * 2), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m)
        starts = [int(np.searchsorted(of, k)) for k in range(K + 1)]

        def per_spot():
            solver.solve_turn_d(m, ins[0].ptr, ins[1].ptr, trees, args.iters, strategy_d=strategy.ptr, value_d=value.ptr, br_d=br.ptr, status_d=status.ptr,
                                stream=stream, tree_of=ins[2].ptr)

        def grouped():                                                        # one single-tree call per tree, on its run of spots
            for k in range(K):
                lo, n = starts[k], starts[k + 1] - starts[k]
                solver.solve_turn_d(n, at(ins[0], lo * 4), at(ins[1], lo * 2 * H * 2), trees[k], args.iters, strategy_d=at(strategy, lo * D * 4 * H * 2),
                                    value_d=at(value, lo * 2 * H * 8), br_d=at(br, lo * 2 * H * 8), status_d=at(status, lo), stream=stream)

        leg = {}
        for name, run in (("single_tree_calls", grouped), ("tree_per_spot_call", per_spot)):
            us, each, wall, odd = time_stream(run, stream, args.samples, warmup=1)
            assert not status.download(np.uint8, m).any()
            v, bb = value.download(np.int64, m * 2 * H), br.download(np.int64, m * 2 * H)
            assert (bb >= v).all() and v.any()
            leg[name] = dict(ms=round(us * 1e-3, 3), samples_ms=[round(x * 1e-3, 3) for x in each], host_clock_ms=round(wall * 1e-3, 3), event_anomalies=odd,
                             calls=K if run is grouped else 1, spot_iterations_per_s=round(m * args.iters / (us * 1e-6), 0), value_sum=int(v.sum()))
        assert leg["single_tree_calls"]["value_sum"] == leg["tree_per_spot_call"]["value_sum"]          # the same spots, the same trees: the same values
        leg["ratio_tree_per_spot_to_single"] = round(leg["tree_per_spot_call"]["ms"] / leg["single_tree_calls"]["ms"], 4)
        leg["note"] = ("single_tree_calls is THIS library's one-tree entry in the same process; the parent commit's one-tree entry is timed separately, "
                       "by this tool's ordinary legs on that commit's library")
        res["trees_%d_m_%d" % (K, m)] = dict(iters=args.iters, trees=K, tree_nodes=sorted({t.n for t in trees}), grid=solver.turn_grid(trees, m), **leg)
        for x in ins + [strategy, value, br, status]:
            x.free()


def lock_legs(args, stream, res):
    """--lock (the module's docstring)"""
    rng = np.random.default_rng(0)
    board, _, ranges = subgames(rng, max(args.m))
    tree = solver.turn_tree(100, 400, (1.0,), 1)
    Dt, Dr = len(tree.decision_nodes), len(tree.river_decision_nodes)
    t1, r1 = tree.rows_of(1)
    tf, rf = {"none": (np.zeros(Dt, bool), np.zeros(Dr, bool)), "one": (t1, r1), "all": (np.ones(Dt, bool), np.ones(Dr, bool))}[args.lock]
    iters = 0 if args.lock == "all" else args.iters
    for m in args.m:
        of = np.zeros(m, np.uint32)
        lock, rlock = (np.ascontiguousarray(np.broadcast_to(f, (m, len(f))), np.uint8) for f in (tf, rf))
        ins = [DeviceBuffer(x.nbytes).upload(x) for x in (np.ascontiguousarray(board[:m]), np.ascontiguousarray(ranges[:m]), of, lock, rlock)]
        strategy, value, br, status = DeviceBuffer(m * Dt * 4 * H * 2), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m)
        locked, rlocked = DeviceBuffer(m * Dt * 4 * H * 2), DeviceBuffer(m * Dr * 52 * 4 * H * 2)

        def plain():
            solver.solve_turn_d(m, ins[0].ptr, ins[1].ptr, [tree], args.iters, strategy_d=strategy.ptr, value_d=value.ptr, br_d=br.ptr, status_d=status.ptr,
                                stream=stream, tree_of=ins[2].ptr)

        def with_locks():
            solver.solve_turn_d(m, ins[0].ptr, ins[1].ptr, [tree], iters, strategy_d=strategy.ptr, value_d=value.ptr, br_d=br.ptr, status_d=status.ptr,
                                stream=stream, tree_of=ins[2].ptr, lock=ins[3].ptr, locked=locked.ptr, river_lock=ins[4].ptr, river_locked=rlocked.ptr)

        # what the rows are locked to: a plain solution of the same spots (device to device, behind the solve on the same stream)
        solver.solve_turn_d(m, ins[0].ptr, ins[1].ptr, [tree], 4, strategy_d=locked.ptr, river_strategy_d=rlocked.ptr, status_d=status.ptr, stream=stream,
                            tree_of=ins[2].ptr)
        assert hipmem._lib().hipStreamSynchronize(stream) == 0
        leg = {}
        for name, run in (("tree_per_spot_call", plain), ("locked_call", with_locks)) if args.lock == "none" else (("locked_call", with_locks),):
            us, each, wall, odd = time_stream(run, stream, args.samples, warmup=1)
            assert not status.download(np.uint8, m).any()
            v, bb = value.download(np.int64, m * 2 * H), br.download(np.int64, m * 2 * H)
            assert (bb >= v).all() and v.any()
            leg[name] = dict(ms=round(us * 1e-3, 3), samples_ms=[round(x * 1e-3, 3) for x in each], host_clock_ms=round(wall * 1e-3, 3), event_anomalies=odd,
                             solves_per_s=round(m / (us * 1e-6), 1), value_sum=int(v.sum()))
        if args.lock == "none":
            assert leg["tree_per_spot_call"]["value_sum"] == leg["locked_call"]["value_sum"]                # nothing locked: the same values
            leg["ratio_locked_to_tree_per_spot"] = round(leg["locked_call"]["ms"] / leg["tree_per_spot_call"]["ms"], 4)
        res["lock_%s_m_%d" % (args.lock, m)] = dict(iters=iters, locked_rows=[int(tf.sum()), int(rf.sum())], rows=[Dt, Dr], grid=solver.turn_grid([tree], m), **leg)
        for x in ins + [strategy, value, br, status, locked, rlocked]:
            x.free()


def resolve_legs(args, stream, res):
    """--resolve (the module's docstring)"""
    rng = np.random.default_rng(0)
    board, river, ranges = subgames(rng, max(args.m))
    tree = solver.turn_tree(100, 400, (1.0,), 1)
    Dt = len(tree.decision_nodes)
    node = tree.river_decision_nodes[1]
    rows = solver._TreeRows([tree], solver.TURN_MAX_NODES)
    for m in args.m:
        b, r = np.ascontiguousarray(board[:m]), np.ascontiguousarray(ranges[:m])
        cards = np.ascontiguousarray(river.reshape(-1, 48, 5)[:m, 24, 4])     # a river card from the middle of each spot's pool
        ins = [DeviceBuffer(x.nbytes).upload(x) for x in (b, r, r.astype(np.uint32) << 1, np.full(m, node, np.uint8), cards)]
        strategy, value, br, status = DeviceBuffer(m * Dt * 4 * H * 2), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m)
        nreach, nvalue, nbr = DeviceBuffer(m * 2 * H * 4), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m * 2 * H * 8)

        def call(ranges_d=None, reach=None, at_d=None, card_d=None, nodes=(None, None, None)):
            L.check(L.lib().pk_solve_turn_resolve_d(0, m, ins[0].ptr, None, ranges_d, *rows.args(), None, args.iters, None, None, None, None, reach, at_d, card_d,
                                                    strategy.ptr, None, value.ptr, br.ptr, *nodes, status.ptr, stream))

        def locked_entry():
            solver.solve_turn_d(m, ins[0].ptr, ins[1].ptr, tree, args.iters, strategy_d=strategy.ptr, value_d=value.ptr, br_d=br.ptr, status_d=status.ptr,
                                stream=stream, lock=None, locked=nvalue.ptr)             # (locked without lock: not looked at; the locked entry point)

        runs = {"none": (("locked_call", locked_entry), ("resolve_call", lambda: call(ranges_d=ins[1].ptr))),
                "at": (("resolve_call", lambda: call(reach=ins[2].ptr, at_d=ins[3].ptr, card_d=ins[4].ptr, nodes=(nreach.ptr, nvalue.ptr, nbr.ptr))),)}[args.resolve]
        leg = {}
        for name, run in runs:
            us, each, wall, odd = time_stream(run, stream, args.samples, warmup=1)
            assert not status.download(np.uint8, m).any()
            v, bb = value.download(np.int64, m * 2 * H), br.download(np.int64, m * 2 * H)
            assert (bb >= v).all() and v.any()
            leg[name] = dict(ms=round(us * 1e-3, 3), samples_ms=[round(x * 1e-3, 3) for x in each], host_clock_ms=round(wall * 1e-3, 3), event_anomalies=odd,
                             solves_per_s=round(m / (us * 1e-6), 1), value_sum=int(v.sum()))
        if args.resolve == "none":
            assert leg["locked_call"]["value_sum"] == leg["resolve_call"]["value_sum"]                      # nothing new used: the same values
            leg["ratio_resolve_to_locked"] = round(leg["resolve_call"]["ms"] / leg["locked_call"]["ms"], 4)
        else:
            assert nvalue.download(np.int64, m * 2 * H).any() and nreach.download(np.uint32, m * 2 * H).any()
        res["resolve_%s_m_%d" % (args.resolve, m)] = dict(iters=args.iters, at=node if args.resolve == "at" else None, grid=solver.turn_grid([tree], m), **leg)
        for x in ins + [strategy, value, br, status, nreach, nvalue, nbr]:
            x.free()


def resume_legs(args, stream, res):
    """--resume (the module's docstring)"""
    rng = np.random.default_rng(0)
    board, river, ranges = subgames(rng, max(args.m))
    tree = solver.turn_tree(100, 400, (1.0,), 1)
    Dt, Dr = len(tree.decision_nodes), len(tree.river_decision_nodes)
    rows = solver._TreeRows([tree], solver.TURN_MAX_NODES)
    q = args.iters // 4
    for m in args.m:
        b, r = np.ascontiguousarray(board[:m]), np.ascontiguousarray(ranges[:m])
        ins = [DeviceBuffer(x.nbytes).upload(x) for x in (b, r)]
        t0s = [DeviceBuffer(m * 4).upload(np.full(m, k * q, np.uint32)) for k in range(4)]
        strategy, value, br, status = DeviceBuffer(m * Dt * 4 * H * 2), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m)
        state = [DeviceBuffer(m * Dt * 4 * H * 8), DeviceBuffer(m * Dt * 4 * H * 8), DeviceBuffer(m * Dr * 52 * 4 * H * 8), DeviceBuffer(m * Dr * 52 * 4 * H * 8)]

        def resolve_entry():
            L.check(L.lib().pk_solve_turn_resolve_d(0, m, ins[0].ptr, None, ins[1].ptr, *rows.args(), None, args.iters, None, None, None, None, None, None, None,
                                                    strategy.ptr, None, value.ptr, br.ptr, None, None, None, status.ptr, stream))

        def resume_entry(iters=args.iters, t0=None, with_state=True):
            L.check(L.lib().pk_solve_turn_resume_d(0, m, ins[0].ptr, None, ins[1].ptr, *rows.args(), None, iters, None, None, None, None, None, None, None, t0,
                                                   *[x.ptr if with_state else None for x in state], strategy.ptr, None, value.ptr, br.ptr, None, None, None,
                                                   status.ptr, stream))

        def chain():
            for k in range(4):
                resume_entry(q, t0s[k].ptr)
        runs = {"none": (("resolve_call", resolve_entry), ("resume_call", lambda: resume_entry(with_state=False))),
                "fresh": (("resolve_call", resolve_entry), ("resume_call", resume_entry)),
                "chain": (("one_call", resume_entry), ("four_calls", chain))}[args.resume]
        leg = {}
        for name, run in runs:
            us, each, wall, odd = time_stream(run, stream, args.samples, warmup=1)
            assert not status.download(np.uint8, m).any()
            v, bb = value.download(np.int64, m * 2 * H), br.download(np.int64, m * 2 * H)
            assert (bb >= v).all() and v.any()
            leg[name] = dict(ms=round(us * 1e-3, 3), samples_ms=[round(x * 1e-3, 3) for x in each], host_clock_ms=round(wall * 1e-3, 3), event_anomalies=odd,
                             solves_per_s=round(m / (us * 1e-6), 1), value_sum=int(v.sum()))
        a, b2 = [n for n, _ in runs]
        assert leg[a]["value_sum"] == leg[b2]["value_sum"] and q * 4 == args.iters                        # the same solve either way
        leg["ratio_%s_to_%s" % (b2, a)] = round(leg[b2]["ms"] / leg[a]["ms"], 4)
        res["resume_%s_m_%d" % (args.resume, m)] = dict(iters=args.iters, grid=solver.turn_grid([tree], m), state_bytes=solver.solver_state_bytes(tree, m), **leg)
        for x in ins + t0s + state + [strategy, value, br, status]:
            x.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--m", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--trees", type=int, default=0, help="K: measure the tree-per-spot entry with K trees (1: the indirection alone)")
    ap.add_argument("--lock", choices=("none", "one", "all"), default=None, help="measure the locked entry: nothing, player 1 or every row locked")
    ap.add_argument("--resolve", choices=("none", "at"), default=None, help="measure the re-solving entry: nothing new, or node outputs at a river-level node")
    ap.add_argument("--resume", choices=("none", "fresh", "chain"), default=None, help="measure the resuming entry: no state, state from nothing, a solve in four calls")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "solver_resume_bench.json" if args.resume else "solver_resolve_bench.json" if args.resolve else "solver_lock_bench.json" if args.lock else "solver_trees_bench.json" if args.trees else "turn_solver_bench.json")
    if pokerl_amd.device_count() < 1:
        sys.exit("turn_solver_bench: no MI355X visible (no fallback)")
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    if args.resume:
        from river_solver_bench import merge_into
        ks = kernel_meta.kernels(L.LIB_PATH)
        res = dict(tool="turn_solver_bench --resume", src=L.source_hash(), samples=args.samples)
        for name in ("k_resolve_turn_solve", "k_resume_turn_solve"):
            res[name] = dict(vgprs=ks[name]["vgprs"], sgprs=ks[name]["sgprs"], lds=ks[name]["lds"], scratch=ks[name]["private_segment"])
        resume_legs(args, stream, res)
        hip.hipStreamDestroy(stream)
        merge_into(args.out, "turn", res)
        print(json.dumps(res))
        return
    if args.resolve:
        from river_solver_bench import merge_into
        ks = kernel_meta.kernels(L.LIB_PATH)
        res = dict(tool="turn_solver_bench --resolve", src=L.source_hash(), samples=args.samples)
        for name in ("k_lock_turn_solve", "k_resolve_turn_solve"):
            res[name] = dict(vgprs=ks[name]["vgprs"], sgprs=ks[name]["sgprs"], lds=ks[name]["lds"], scratch=ks[name]["private_segment"])
        resolve_legs(args, stream, res)
        hip.hipStreamDestroy(stream)
        merge_into(args.out, "turn", res)
        print(json.dumps(res))
        return
    if args.lock:
        from river_solver_bench import merge_into
        ks = kernel_meta.kernels(L.LIB_PATH)
        res = dict(tool="turn_solver_bench --lock", src=L.source_hash(), samples=args.samples)
        for name in ("k_trees_turn_solve", "k_lock_turn_solve"):
            res[name] = dict(vgprs=ks[name]["vgprs"], sgprs=ks[name]["sgprs"], lds=ks[name]["lds"], scratch=ks[name]["private_segment"])
        lock_legs(args, stream, res)
        hip.hipStreamDestroy(stream)
        merge_into(args.out, "turn", res)
        print(json.dumps(res))
        return
    if args.trees:
        from river_solver_bench import merge_into
        ks = kernel_meta.kernels(L.LIB_PATH)
        res = dict(tool="turn_solver_bench --trees", src=L.source_hash(), samples=args.samples)
        for name in ("k_turn_solve", "k_trees_turn_solve"):
            res[name] = dict(vgprs=ks[name]["vgprs"], sgprs=ks[name]["sgprs"], lds=ks[name]["lds"], scratch=ks[name]["private_segment"])
        trees_legs(args, stream, res)
        hip.hipStreamDestroy(stream)
        merge_into(args.out, "turn", res)
        print(json.dumps(res))
        return
    rng = np.random.default_rng(0)
    tree, rtree = solver.turn_tree(100, 400, (1.0,), 1), solver.river_tree(100, 400, (1.0,), 1)
    Dt = len(tree.decision_nodes)
    nr = int(tree.river_level.sum())
    meta = kernel_meta.kernels(L.LIB_PATH)["k_turn_solve"]
    res = dict(tool="turn_solver_bench", src=L.source_hash(), samples=args.samples, iters=args.iters, tree_nodes=tree.n, turn_level_nodes=tree.n - nr,
               river_level_nodes=nr, yardstick_tree_nodes=rtree.n, legs={},
               k_turn_solve=dict(vgprs=meta["vgprs"], sgprs=meta["sgprs"], lds=meta["lds"], scratch=meta["private_segment"], block=512))
    board, river, ranges = subgames(rng, max(args.m))
    for m in args.m:
        grid = solver.turn_grid(tree, m)
        ins = [DeviceBuffer(x.nbytes).upload(x) for x in (np.ascontiguousarray(board[:m]), np.ascontiguousarray(ranges[:m]))]
        strategy, value, br, status = DeviceBuffer(m * Dt * 4 * H * 2), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m)

        def run():
            solver.solve_turn_d(m, ins[0].ptr, ins[1].ptr, tree, args.iters, strategy_d=strategy.ptr, value_d=value.ptr, br_d=br.ptr, status_d=status.ptr,
                                stream=stream)

        us, each, wall, odd = time_stream(run, stream, args.samples, warmup=1)
        assert not status.download(np.uint8, m).any()
        v, b = value.download(np.int64, m * 2 * H), br.download(np.int64, m * 2 * H)
        assert (b >= v).all() and v.any()
        for x in ins + [strategy, value, br, status]:
            x.free()
        # the yardstick: 48 m river subgames, each spot's ranges repeated for its 48 river boards
        M = 48 * m
        rins = [DeviceBuffer(x.nbytes).upload(x) for x in (np.ascontiguousarray(river[:M]), np.ascontiguousarray(np.repeat(ranges[:m], 48, axis=0)))]
        rvalue, rbr, rstatus = DeviceBuffer(M * 2 * H * 8), DeviceBuffer(M * 2 * H * 8), DeviceBuffer(M)

        def run_river():
            solver.solve_river_d(M, rins[0].ptr, rins[1].ptr, rtree, args.iters, value_d=rvalue.ptr, br_d=rbr.ptr, status_d=rstatus.ptr, stream=stream)

        rus, reach, rwall, rodd = time_stream(run_river, stream, args.samples, warmup=1)
        assert not rstatus.download(np.uint8, M).any()
        for x in rins + [rvalue, rbr, rstatus]:
            x.free()
        res["legs"]["m_%d" % m] = dict(ms_per_call=round(us * 1e-3, 3), samples_ms=[round(x * 1e-3, 3) for x in each], host_clock_ms=round(wall * 1e-3, 3),
                                       event_anomalies=odd + rodd, grid=grid, us_per_spot_iteration=round(us / (m * args.iters), 3),
                                       work_space_bytes=((m * 24 + 255) & ~255) + grid * (TABLE_BYTES + (tree.n - nr) * TURN_NODE_BYTES + nr * RIVER_NODE_BYTES),
                                       yardstick_ms_per_call=round(rus * 1e-3, 3), yardstick_samples_ms=[round(x * 1e-3, 3) for x in reach],
                                       ratio_to_yardstick=round(us / rus, 3))
    hip.hipStreamDestroy(stream)
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
