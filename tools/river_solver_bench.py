#!/usr/bin/env python3
"""Timings of the river solver (pk_solve_river_d) on one MI355X, printed as ONE JSON line and written to profiles/river_solver_bench.json
(stamped with the library's source hash).  Legs: m = 512 and 4 096 full-pool river subgames (random boards, random ranges with zeros and
65 535s), the default tree river_tree(100, 400), 256 iterations, all outputs.  Per leg: milliseconds per call (a HIP event pair on the
call's stream and the host's clock, every shape warmed up, median of `--samples`), solves per second, and the call's work-space bytes
(the descriptors plus one slice per resident workgroup).  For scale, --spec-iters N times N iterations of the numpy restatement
(tests/river_solver_spec.py) of ONE of the same subgames on the host and reports seconds per iteration.

    python tools/river_solver_bench.py [--samples 3] [--m 512 4096] [--iters 256] [--spec-iters 4]

--trees K measures the tree-per-spot entry (pk_solve_river_trees_d) instead, and merges its legs into
profiles/solver_trees_bench.json under "river".  K = 1, the price of the indirection: the same spots and the same tree through
pk_solve_river_d and through pk_solve_river_trees_d with that one tree, one after the other in the same process.  K > 1, a heterogeneous
batch: m spots over K distinct pots (river_tree(60 + 10 k, 400), spot i has pot i % K) in ONE tree-per-spot call, against the same spots
grouped by pot into K single-tree calls queued back to back on the stream; spot-iterations per second of both.

    python tools/river_solver_bench.py --trees 1 --m 512
    python tools/river_solver_bench.py --trees 64 --m 1024 --iters 64

--lock {none,one,all} measures the locked entry (pk_solve_river_locked_d) on the ordinary legs' spots and tree, and
merges its legs into profiles/solver_lock_bench.json under "river".  none: nothing locked, against pk_solve_river_trees_d with that one tree
in the same process -- the price of the LOCK instantiation.  one: player 1's rows locked to a plain solution of the same spots, CFR+ for
player 0.  all: every row locked, no iteration -- evaluations of a supplied strategy per second.

    python tools/river_solver_bench.py --lock none --m 512

--resolve {none,at,gadget} measures the re-solving entry (pk_solve_river_resolve_d) on the ordinary legs' spots and
tree, and merges its legs into profiles/solver_resolve_bench.json under "river".  none: none of the new arguments, against
pk_solve_river_locked_d with nothing locked in the same process (k_lock_river_solve: the kernel tools/isa_diff.py shows identical to the
parent commit's) -- the price of the RESOLVE instantiation.  at: the root reaches from `reach` and the three node outputs at the node after
player 0's first bet.  gadget: the subtree below that node re-solved through gadget_tree from the node_reach and node_br of a first solve.

    python tools/river_solver_bench.py --resolve none --m 512
--resume {none,fresh,chain} measures the resuming entry (pk_solve_river_resume_d) on the ordinary legs' spots and tree,
and merges its legs into profiles/solver_resume_bench.json under "river".  none: the new entry without state -- by its definition the
re-solving call -- against pk_solve_river_resolve_d.  fresh: state given, t0 = 0 (k_resume_river_solve: the instantiation, the zero fill and
one store of the state), against the re-solving entry.  chain: four calls of a quarter of the iterations, t0 = 0, q, 2q, 3q, against one call
with state: the price of stopping, one load and one store of the state per call.
    python tools/river_solver_bench.py --resume chain --m 512
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
from equity_bench import CANON, time_stream  # noqa: E402
import kernel_meta  # noqa: E402

H = L.EQ_HOLDINGS
NODE_BYTES = 1088 * 44      # pk::RS_NODE_BYTES: a workgroup's work space per tree node


def work_bytes(m, n):
    """pk::rs_work_bytes"""
    return ((m * 24 + 255) & ~255) + min(m, solver.GRID_MAX) * n * NODE_BYTES


def subgames(rng, m):
    board = np.zeros((m, 5), np.uint8)
    for i in range(m):
        board[i] = [CANON[c] for c in rng.permutation(52)[:5]]
    ranges = rng.integers(0, 65536, (m, 2, H)).astype(np.uint16)
    for row in ranges.reshape(-1, H):
        row[rng.integers(0, H, 200)] = 0
        row[rng.integers(0, H, 100)] = 65535
    return board, ranges


def merge_into(path, key, res):
    """profiles/solver_trees_bench.json holds the river and the turn tool's legs side by side"""
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc.setdefault(key, {}).update(res)
    with open(path, "w") as f:
        f.write(json.dumps(doc) + "\n")


def at(buf, offset):
    """a device pointer `offset` bytes into a DeviceBuffer"""
    return C.c_void_p(buf.ptr.value + offset)


def trees_legs(args, stream, res):
    """--trees K (the module's docstring)"""
    K = args.trees
    rng = np.random.default_rng(0)
    board, ranges = subgames(rng, max(args.m))
    trees = [solver.river_tree(100, 400)] if K == 1 else [solver.river_tree(60 + 10 * k, 400) for k in range(K)]
    D = max(len(t.decision_nodes) for t in trees)
    for m in args.m:
        tree_of = (np.arange(m) % K).astype(np.uint32)
        order = np.argsort(tree_of, kind="stable")                            # the spots grouped by tree: K runs of consecutive spots
        b, r = np.ascontiguousarray(board[:m][order]), np.ascontiguousarray(ranges[:m][order])
        of = np.ascontiguousarray(tree_of[order])
        ins = [DeviceBuffer(x.nbytes).upload(x) for x in (b, r, of)]
        strategy, value, br, status = DeviceBuffer(m * D * 4 * H * 2), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m)
        starts = [int(np.searchsorted(of, k)) for k in range(K + 1)]

        def per_spot():
            solver.solve_river_d(m, ins[0].ptr, ins[1].ptr, trees, args.iters, strategy_d=strategy.ptr, value_d=value.ptr, br_d=br.ptr, status_d=status.ptr,
                                 stream=stream, tree_of=ins[2].ptr)

        def grouped():                                                        # one single-tree call per tree, on its run of spots
            for k in range(K):
                lo, n = starts[k], starts[k + 1] - starts[k]
                solver.solve_river_d(n, at(ins[0], lo * 5), at(ins[1], lo * 2 * H * 2), trees[k], args.iters, strategy_d=at(strategy, lo * D * 4 * H * 2),
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
        res["trees_%d_m_%d" % (K, m)] = dict(iters=args.iters, trees=K, tree_nodes=sorted({t.n for t in trees}), **leg)
        for x in ins + [strategy, value, br, status]:
            x.free()


def lock_legs(args, stream, res):
    """--lock (the module's docstring)"""
    rng = np.random.default_rng(0)
    board, ranges = subgames(rng, max(args.m))
    tree = solver.river_tree(100, 400)
    D = len(tree.decision_nodes)
    flags = {"none": np.zeros(D, bool), "one": tree.rows_of(1), "all": np.ones(D, bool)}[args.lock]
    iters = 0 if args.lock == "all" else args.iters
    for m in args.m:
        of = np.zeros(m, np.uint32)
        lock = np.ascontiguousarray(np.broadcast_to(flags, (m, D)), np.uint8)
        ins = [DeviceBuffer(x.nbytes).upload(x) for x in (np.ascontiguousarray(board[:m]), np.ascontiguousarray(ranges[:m]), of, lock)]
        strategy, value, br, status = DeviceBuffer(m * D * 4 * H * 2), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m)
        locked = DeviceBuffer(m * D * 4 * H * 2)

        def plain():
            solver.solve_river_d(m, ins[0].ptr, ins[1].ptr, [tree], args.iters, strategy_d=strategy.ptr, value_d=value.ptr, br_d=br.ptr, status_d=status.ptr,
                                 stream=stream, tree_of=ins[2].ptr)

        def with_locks():
            solver.solve_river_d(m, ins[0].ptr, ins[1].ptr, [tree], iters, strategy_d=strategy.ptr, value_d=value.ptr, br_d=br.ptr, status_d=status.ptr,
                                 stream=stream, tree_of=ins[2].ptr, lock=ins[3].ptr, locked=locked.ptr)

        # what the rows are locked to: a plain solution of the same spots (device to device, behind the solve on the same stream)
        solver.solve_river_d(m, ins[0].ptr, ins[1].ptr, [tree], 16, strategy_d=locked.ptr, status_d=status.ptr, stream=stream, tree_of=ins[2].ptr)
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
        res["lock_%s_m_%d" % (args.lock, m)] = dict(iters=iters, locked_rows=int(flags.sum()), rows=D, **leg)
        for x in ins + [strategy, value, br, status, locked]:
            x.free()


def resolve_legs(args, stream, res):
    """--resolve (the module's docstring)"""
    rng = np.random.default_rng(0)
    board, ranges = subgames(rng, max(args.m))
    tree = solver.river_tree(100, 400)
    node = int(tree.child[0][1])
    sub, _ = tree.subtree(node)
    gadget = solver.gadget_tree(sub, 1)
    used = gadget if args.resolve == "gadget" else tree
    D = len(used.decision_nodes)
    rows = solver._TreeRows([used], solver.MAX_NODES)
    for m in args.m:
        b, r = np.ascontiguousarray(board[:m]), np.ascontiguousarray(ranges[:m])
        ins = [DeviceBuffer(x.nbytes).upload(x) for x in (b, r, r.astype(np.uint32) << 4, np.full(m, node, np.uint8))]
        strategy, value, br, status = DeviceBuffer(m * D * 4 * H * 2), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m)
        nreach, nvalue, nbr = DeviceBuffer(m * 2 * H * 4), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m * 2 * H * 8)

        def call(ranges_d=None, reach=None, given=None, at_d=None, nodes=(None, None, None)):
            L.check(L.lib().pk_solve_river_resolve_d(0, m, ins[0].ptr, None, ranges_d, *rows.args(), None, args.iters, None, None, reach, given, at_d, strategy.ptr,
                                                     value.ptr, br.ptr, *nodes, status.ptr, stream))

        def locked_entry():
            solver.solve_river_d(m, ins[0].ptr, ins[1].ptr, tree, args.iters, strategy_d=strategy.ptr, value_d=value.ptr, br_d=br.ptr, status_d=status.ptr,
                                 stream=stream, lock=None, locked=nvalue.ptr)            # (locked without lock: not looked at; the locked entry point)

        runs = {"none": (("locked_call", locked_entry), ("resolve_call", lambda: call(ranges_d=ins[1].ptr))),
                "at": (("resolve_call", lambda: call(reach=ins[2].ptr, at_d=ins[3].ptr, nodes=(nreach.ptr, nvalue.ptr, nbr.ptr))),),
                "gadget": (("resolve_call", lambda: call(reach=nreach.ptr, given=nbr.ptr)),)}[args.resolve]
        if args.resolve == "gadget":                                          # the first solve: its node_reach and node_br stay on the device
            solver.solve_river_d(m, ins[0].ptr, ins[1].ptr, tree, args.iters, status_d=status.ptr, stream=stream, at=ins[3].ptr, node_reach_d=nreach.ptr,
                                 node_br_d=nbr.ptr)
            assert hipmem._lib().hipStreamSynchronize(stream) == 0 and not status.download(np.uint8, m).any()
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
        if args.resolve == "at":
            assert nvalue.download(np.int64, m * 2 * H).any() and nreach.download(np.uint32, m * 2 * H).any()
        res["resolve_%s_m_%d" % (args.resolve, m)] = dict(iters=args.iters, tree_nodes=used.n, at=node if args.resolve == "at" else None, **leg)
        for x in ins + [strategy, value, br, status, nreach, nvalue, nbr]:
            x.free()


def resume_legs(args, stream, res):
    """--resume (the module's docstring)"""
    rng = np.random.default_rng(0)
    board, ranges = subgames(rng, max(args.m))
    tree = solver.river_tree(100, 400)
    D = len(tree.decision_nodes)
    rows = solver._TreeRows([tree], solver.MAX_NODES)
    q = args.iters // 4
    for m in args.m:
        b, r = np.ascontiguousarray(board[:m]), np.ascontiguousarray(ranges[:m])
        ins = [DeviceBuffer(x.nbytes).upload(x) for x in (b, r)]
        t0s = [DeviceBuffer(m * 4).upload(np.full(m, k * q, np.uint32)) for k in range(4)]
        strategy, value, br, status = DeviceBuffer(m * D * 4 * H * 2), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m)
        regret, average = DeviceBuffer(m * D * 4 * H * 8), DeviceBuffer(m * D * 4 * H * 8)

        def resolve_entry():
            L.check(L.lib().pk_solve_river_resolve_d(0, m, ins[0].ptr, None, ins[1].ptr, *rows.args(), None, args.iters, None, None, None, None, None, strategy.ptr,
                                                     value.ptr, br.ptr, None, None, None, status.ptr, stream))

        def resume_entry(iters=args.iters, t0=None, state=True):
            L.check(L.lib().pk_solve_river_resume_d(0, m, ins[0].ptr, None, ins[1].ptr, *rows.args(), None, iters, None, None, None, None, None, t0,
                                                    regret.ptr if state else None, average.ptr if state else None, strategy.ptr, value.ptr, br.ptr, None, None,
                                                    None, status.ptr, stream))

        def chain():
            for k in range(4):
                resume_entry(q, t0s[k].ptr)
        runs = {"none": (("resolve_call", resolve_entry), ("resume_call", lambda: resume_entry(state=False))),
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
        res["resume_%s_m_%d" % (args.resume, m)] = dict(iters=args.iters, tree_nodes=tree.n, state_bytes=2 * m * D * 4 * H * 8, **leg)
        for x in ins + t0s + [strategy, value, br, status, regret, average]:
            x.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--m", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--iters", type=int, default=256)
    ap.add_argument("--spec-iters", type=int, default=0)
    ap.add_argument("--trees", type=int, default=0, help="K: measure the tree-per-spot entry with K trees (1: the indirection alone)")
    ap.add_argument("--lock", choices=("none", "one", "all"), default=None, help="measure the locked entry: nothing, player 1 or every row locked")
    ap.add_argument("--resolve", choices=("none", "at", "gadget"), default=None, help="measure the re-solving entry: nothing new, node outputs, a gadget solve")
    ap.add_argument("--resume", choices=("none", "fresh", "chain"), default=None, help="measure the resuming entry: no state, state from nothing, a solve in four calls")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "solver_resume_bench.json" if args.resume else "solver_resolve_bench.json" if args.resolve else "solver_lock_bench.json" if args.lock else "solver_trees_bench.json" if args.trees else "river_solver_bench.json")
    if pokerl_amd.device_count() < 1:
        sys.exit("river_solver_bench: no MI355X visible (no fallback)")
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    if args.resume:
        ks = kernel_meta.kernels(L.LIB_PATH)
        res = dict(tool="river_solver_bench --resume", src=L.source_hash(), samples=args.samples)
        for name in ("k_resolve_river_solve", "k_resume_river_solve"):
            res[name] = dict(vgprs=ks[name]["vgprs"], sgprs=ks[name]["sgprs"], lds=ks[name]["lds"], scratch=ks[name]["private_segment"])
        resume_legs(args, stream, res)
        hip.hipStreamDestroy(stream)
        merge_into(args.out, "river", res)
        print(json.dumps(res))
        return
    if args.resolve:
        ks = kernel_meta.kernels(L.LIB_PATH)
        res = dict(tool="river_solver_bench --resolve", src=L.source_hash(), samples=args.samples)
        for name in ("k_lock_river_solve", "k_resolve_river_solve"):
            res[name] = dict(vgprs=ks[name]["vgprs"], sgprs=ks[name]["sgprs"], lds=ks[name]["lds"], scratch=ks[name]["private_segment"])
        resolve_legs(args, stream, res)
        hip.hipStreamDestroy(stream)
        merge_into(args.out, "river", res)
        print(json.dumps(res))
        return
    if args.lock:
        ks = kernel_meta.kernels(L.LIB_PATH)
        res = dict(tool="river_solver_bench --lock", src=L.source_hash(), samples=args.samples)
        for name in ("k_trees_river_solve", "k_lock_river_solve"):
            res[name] = dict(vgprs=ks[name]["vgprs"], sgprs=ks[name]["sgprs"], lds=ks[name]["lds"], scratch=ks[name]["private_segment"])
        lock_legs(args, stream, res)
        hip.hipStreamDestroy(stream)
        merge_into(args.out, "river", res)
        print(json.dumps(res))
        return
    if args.trees:
        ks = kernel_meta.kernels(L.LIB_PATH)
        res = dict(tool="river_solver_bench --trees", src=L.source_hash(), samples=args.samples)
        for name in ("k_river_solve", "k_trees_river_solve"):
            res[name] = dict(vgprs=ks[name]["vgprs"], sgprs=ks[name]["sgprs"], lds=ks[name]["lds"], scratch=ks[name]["private_segment"])
        trees_legs(args, stream, res)
        hip.hipStreamDestroy(stream)
        merge_into(args.out, "river", res)
        print(json.dumps(res))
        return
    rng = np.random.default_rng(0)
    tree = solver.river_tree(100, 400)
    D = len(tree.decision_nodes)
    meta = kernel_meta.kernels(L.LIB_PATH)["k_river_solve"]
    res = dict(tool="river_solver_bench", src=L.source_hash(), samples=args.samples, iters=args.iters, tree_nodes=tree.n, decision_nodes=D, legs={},
               k_river_solve=dict(vgprs=meta["vgprs"], sgprs=meta["sgprs"], lds=meta["lds"], scratch=meta["private_segment"], block=512, grid_max=solver.GRID_MAX))
    board, ranges = subgames(rng, max(args.m))
    for m in args.m:
        ins = [DeviceBuffer(x.nbytes).upload(x) for x in (np.ascontiguousarray(board[:m]), np.ascontiguousarray(ranges[:m]))]
        strategy, value, br, status = DeviceBuffer(m * D * 4 * H * 2), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m * 2 * H * 8), DeviceBuffer(m)

        def run():
            solver.solve_river_d(m, ins[0].ptr, ins[1].ptr, tree, args.iters, strategy_d=strategy.ptr, value_d=value.ptr, br_d=br.ptr, status_d=status.ptr,
                                 stream=stream)

        us, each, wall, odd = time_stream(run, stream, args.samples, warmup=1)
        assert not status.download(np.uint8, m).any()
        v, b = value.download(np.int64, m * 2 * H), br.download(np.int64, m * 2 * H)
        assert (b >= v).all() and v.any()
        res["legs"]["m_%d" % m] = dict(ms_per_call=round(us * 1e-3, 3), samples_ms=[round(x * 1e-3, 3) for x in each], host_clock_ms=round(wall * 1e-3, 3),
                                       event_anomalies=odd, solves_per_s=round(m / (us * 1e-6), 1), iterations_per_s=round(m * args.iters / (us * 1e-6), 0),
                                       work_space_bytes=work_bytes(m, tree.n))
        for x in ins + [strategy, value, br, status]:
            x.free()
    if args.spec_iters > 0:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import river_solver_spec as RS
        RS.solve_spot([int(x) for x in board[0]], ranges[0], tree, 1)                       # (warm: the pairwise matrices' code paths)
        t0 = time.perf_counter()
        RS.solve_spot([int(x) for x in board[0]], ranges[0], tree, 1)
        t1 = time.perf_counter()
        RS.solve_spot([int(x) for x in board[0]], ranges[0], tree, 1 + args.spec_iters)
        t2 = time.perf_counter()
        per_iter = ((t2 - t1) - (t1 - t0)) / args.spec_iters
        res["numpy_spec_on_the_host"] = dict(seconds_per_iteration=round(per_iter, 4), seconds_per_solve_extrapolated=round(per_iter * args.iters + (t1 - t0), 2),
                                             note="one subgame, int64 numpy on one host core; not the device's yardstick, only a sense of scale")
    hip.hipStreamDestroy(stream)
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
