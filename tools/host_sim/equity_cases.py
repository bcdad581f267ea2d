#!/usr/bin/env python3
"""Dev-only: the cases of tools/host_sim/equity_sim.cpp -- the equity kernels run on the CPU as 8-wave workgroups (wg_shim.h) -- and their
expected values.  This module writes a case file, runs the driver on it, reads every output array back and compares it, by exact integer
equality, with the numpy specs of tests/ (equity_spec, equity_sampled_spec, equity_range_spec, rvr_spec, hist_spec: themselves pinned to the
reference's fixtures by the host tests).  Nothing expected comes from a kernel.  tests/test_equity_sim_host.py runs the cases marked quick on a
plain build; tools/host_sim/sanitize_equity.sh runs all of them on the ASan + UBSan and the TSan build.

The shapes are the smallest at which each mechanism of the kernels can break (docs/history.md lists them with their reasons):
  k_rvr / k_hist   nh = C(P, 2) pool holdings: P = 11|12, 16|17, 23|24, 32|33, 45|46 lie across each size of the sort (npad 64 .. 2048; 32|33 and
                   45|46 also give a lane its second and third holding), 47 is the full river pool, k + 4 the smallest; river and turn spots
                   (1 and P completions), flop spots at P = 6, 7 (the pair-order walk); every weight form, a dead range, a range dead on some
                   completions; bins 1, 7, 32; each output NULL in turn; a grid of 1 with spots of falling size (stale LDS); a refused spot
                   between good ones;
  k_eqr            nb = 3, 4, 5; the smallest pool; sets below 512 and no multiple of 512; a grid of 1 (the counters cleared for the next spot);
                   agg NULL and not; every weight form; a refused spot in between;
  k_equity<N>      N = 2, 3, 9, 16; nb = 0 .. 5; folded seats, a lone live seat; grids of 1 and 2 with more tasks than waves; 64+ one-task
                   spots on a grid of 1 (take = 4); refused spots inside the batch;
  k_eqs<N>         N = 2, 6, 16; hidden hole cards up to 37 draws (three Philox blocks); samples 1, 63, 64, 65 and several tasks per spot; two nonces;
  k_eqw<N, RC>     (ranged_cases, run beside all_cases by this program and by tests/test_equity_ranged_sim_host.py) N = 2, 3, 6, 16; the three LDS
                   size classes (R = 0, 4, 16); H = 1 .. 16 hidden seats (1 .. 9 Philox blocks); dense, sparse, one-holding and dead ranges; attempts
                   1, 65 and several tasks per spot on a grid of 1; a refused spot between good ones; the three new refusals; the table form;
  k_ev<N>          (ev_cases, run beside all_cases by this program and by tests/test_equity_ev_sim_host.py) N = 2, 3, 5, 9, 16; a grid of 1 with
                   spots of falling size and different levels (stale LDS, stale level tables); a refused spot (a bad bet, a bad card) between
                   valid ones; five live seats on a ladder -- four levels to compare, the smallest spot that needs a second group of levels;
                   ladders at 9 and 16 seats; dead money, a live seat with bet 0, one live seat, all bets 0; each output NULL in turn; the
                   table form with bets + pending_bets.  f64 arrays travel as their bit patterns: amount and ev are compared bit for bit;
  k_cl_*           (cluster_cases, run beside all_cases by this program and by tests/test_hist_cluster_sim_host.py) quantise / assign / update /
                   finalise / seed as pk::cl_*_launch queues them; 1, 2, 7, 10 and 32 bins; a grid of 1 (every workgroup strides), an unaligned
                   histogram pointer, empty rows as whole waves, constructed ties, both update kernels, seeding over several chunks and tiles.
  k_hero_hist      (hero_hist_cases, run beside all_cases by this program and by tests/test_hero_hist_sim_host.py) k_eqr's shapes: nb = 3, 4, 5;
                   the smallest pool; sets below 512 and no multiple of 512; a river spot (one completion); a grid of 1 with spots of falling
                   size (the counters cleared for the next spot, stale LDS); every weight form, a dead range (every completion void); bins 1,
                   7, 10, 32; each output NULL in turn; a refused spot between good ones; the table form.
  preparation      every status bit, the explicit and the table form; table indices -1, T and 2^31 - 1 (nothing is read: ASan's to check).

  equity_cases.py --exe <equity_sim> [--exe <another build>] [--quick] [--only <substring>] [--list] [--keep <dir>]
"""
import argparse
import hashlib
import math
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import equity_range_spec as RS          # noqa: E402
import equity_ranged_spec as WS         # noqa: E402
import equity_sampled_spec as SS        # noqa: E402
import equity_spec as ES                # noqa: E402
import ev_spec as EV                    # noqa: E402
import hero_hist_spec as HHS             # noqa: E402
import hist_cluster_spec as CS          # noqa: E402
import hist_spec as HS                  # noqa: E402
import preflop_spec as PS               # noqa: E402
import preflop_solver_spec as PFS       # noqa: E402
import river_solver_spec as RVS         # noqa: E402
import resolve_spec as RZS              # noqa: E402
import resume_spec as RMS               # noqa: E402
import solver_resume_util as SMU        # noqa: E402
import solver_lock_spec as SLS           # noqa: E402
import solver_trees_util as STU         # noqa: E402
import turn_solver_spec as TSS          # noqa: E402
import ranged_ev_spec as XS             # noqa: E402
import rvr_spec as VS                   # noqa: E402
from oracle import rng_spec as R        # noqa: E402

HOLDINGS = 1326
IN_FLIGHT, BAD_TABLE = 16, 32
DTYPES = {"u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64, "i32": np.int32}
OUTPUTS = {"equity": ("win", "tie", "share", "boards", "status"), "sampled": ("win", "tie", "share", "samples", "status"),
           "range": ("agg", "win", "tie", "boards", "status"), "rvr": ("win", "tie", "tot", "boards", "status"),
           "hist": ("hist", "void", "completions", "status"), "ranged": ("win", "tie", "share", "accepted", "status"),
           "ev": ("share", "level_seat", "amount", "ev", "boards", "status"),
           "rangedev": ("share", "level_seat", "amount", "ev", "accepted", "status"),
           "cluster": ("centroids_out", "label", "dist", "inertia", "changed"),
           "herohist": ("hist", "void", "completions", "status"), "preflop": ("win", "tie"),
           "pfhero": ("agg", "win", "tie", "boards", "status"), "pfrvr": ("win", "tie", "tot"),
           "riversolve": ("strategy", "value", "br", "status"), "turnsolve": ("strategy", "river_strategy", "value", "br", "status"),
           "rivertrees": ("strategy", "value", "br", "status"), "turntrees": ("strategy", "river_strategy", "value", "br", "status"),
           "pfsolve": ("strategy", "value", "br", "status"),
           "riverlock": ("strategy", "value", "br", "status"), "turnlock": ("strategy", "river_strategy", "value", "br", "status"),
           "riverresolve": ("strategy", "value", "br", "node_reach", "node_value", "node_br", "status"),
           "turnresolve": ("strategy", "river_strategy", "value", "br", "node_reach", "node_value", "node_br", "status"),
           "riverresume": ("strategy", "value", "br", "node_reach", "node_value", "node_br", "status", "regret", "average"),
           "turnresume": ("strategy", "river_strategy", "value", "br", "node_reach", "node_value", "node_br", "status", "regret", "average", "river_regret",
                          "river_average")}


class Case:
    """name, family, the driver's input arrays {name: (dtype, values)}, the outputs wanted, expect() -> {output: array}, quick."""

    def __init__(self, name, family, arrays, expect, outputs=None, quick=False):
        self.name, self.family, self.arrays, self.expect, self.quick = name, family, arrays, expect, quick
        self.outputs = tuple(OUTPUTS[family] if outputs is None else outputs)
        self._want = None

    def expected(self):
        if self._want is None:                                        # (once, however many builds run the case)
            self._want = self.expect()
        return self._want

    def write(self, path):
        with open(path, "w") as f:
            f.write("family %s\noutputs %s\n" % (self.family, " ".join(self.outputs)))
            for key, (dt, val) in self.arrays.items():
                if val is None:
                    continue
                v = np.asarray(val).astype(DTYPES[dt]).reshape(-1)
                f.write("%s %s %d\n%s\n" % (key, dt, v.size, " ".join(str(int(x)) for x in v.tolist())))


def read_outputs(path):
    out = {}
    with open(path) as f:
        while True:
            head = f.readline().split()
            if not head:
                return out
            vals = f.readline().split()
            assert len(vals) == int(head[2]), (head, len(vals))
            out[head[0]] = np.array([int(x) for x in vals], dtype=np.uint64).astype(DTYPES[head[1]])


def run_case(exe, case, workdir, timeout=1800):
    """Runs the driver on one case -> (list of mismatch strings, seconds of the driver, its stdout + stderr)."""
    cpath, opath = os.path.join(workdir, case.name + ".case"), os.path.join(workdir, case.name + ".out")
    case.write(cpath)
    if os.path.exists(opath):
        os.remove(opath)
    t0 = time.time()
    r = subprocess.run([exe, cpath, opath], capture_output=True, text=True, timeout=timeout)
    sec = time.time() - t0
    log = r.stdout + r.stderr
    if r.returncode != 0:
        return ["the driver exited with status %d" % r.returncode], sec, log
    got, want, bad = read_outputs(opath), case.expected(), []
    if sorted(got) != sorted(case.outputs):
        bad.append("outputs written: %s, wanted: %s" % (sorted(got), sorted(case.outputs)))
    for key in case.outputs:
        if key not in got:
            continue
        g = got[key]
        if isinstance(want[key], str):                                # a fixture that holds the array's SHA-256 only
            if hashlib.sha256(np.ascontiguousarray(g).tobytes()).hexdigest() != want[key]:
                bad.append("%s: the SHA-256 of the %d entries is not the fixture's" % (key, g.size))
            continue
        w = np.asarray(want[key]).reshape(-1)
        if g.size != w.size:
            bad.append("%s: %d entries, the spec has %d" % (key, g.size, w.size))
            continue
        ne = np.nonzero(g.astype(np.uint64) != w.astype(np.uint64))[0]
        if ne.size:
            i = int(ne[0])
            bad.append("%s: %d of %d entries differ, the first at %d: kernel %d, spec %d" % (key, ne.size, g.size, i, int(g[i]), int(w[i])))
    return bad, sec, log


# ---------------------------------------------------------------------------------------------------------------- spots
def card(c):
    return ES.CANON[c]


def dead_mask(cards):
    m = 0
    for c in cards:
        m |= 1 << int(c)
    return m


def board_spots(seed, shapes):
    """[(nb, P)] -> board [m, 5], nboard [m], dead [m]: random valid spots whose pool has P cards."""
    rng = np.random.default_rng(seed)
    bs, ns, ds = [], [], []
    for nb, pool in shapes:
        b, n, d = VS.random_boards(rng, 1, nb, pool=pool)
        bs.append(b[0]); ns.append(n[0]); ds.append(d[0])
    return np.array(bs, np.uint8), np.array(ns, np.uint8), np.array(ds, np.uint64)


def hero_spots(seed, shapes):
    rng = np.random.default_rng(seed)
    hs, bs, ns, ds = [], [], [], []
    for nb, pool in shapes:
        h, b, n, d = RS.random_spots(rng, 1, nb, pool=pool)
        hs.append(h[0]); bs.append(b[0]); ns.append(n[0]); ds.append(d[0])
    return np.array(hs, np.uint8), np.array(bs, np.uint8), np.array(ns, np.uint8), np.array(ds, np.uint64)


def weights_for(seed, m, form):
    """form: None, 'shared' [1326], 'spot' [m, 1326], 'zero' (shared, all zero); a third of the entries zero, the largest 65 535."""
    if form is None:
        return None, 0
    if form == "zero":
        return np.zeros(HOLDINGS, np.uint16), 0
    rng = np.random.default_rng(seed)
    shape = (m, HOLDINGS) if form == "spot" else (HOLDINGS,)
    w = rng.integers(0, 200, shape).astype(np.uint16)
    w[rng.random(shape) < 0.33] = 0
    w.reshape(-1)[::97] = 65535
    return w, 1 if form == "spot" else 0


def pack_tables(deck, turn, active, states, inflight):
    """A handle's arrays by hand: deck uint8 [T, 5 + 2N], turn / active [T], states [T, N] (PlayerState: 0 folded 1 active 2 called 3 all in),
    inflight [T] (the step-in-flight bits of the cursor) -> cards [W][T] words, cursors [T], seat_states [T]."""
    deck = np.asarray(deck, np.uint8)
    t, k = deck.shape
    w = (k + 3) // 4
    padded = np.full((t, 4 * w), 0xFF, np.uint32)
    padded[:, :k] = deck
    words = (padded[:, 0::4] | (padded[:, 1::4] << 8) | (padded[:, 2::4] << 16) | (padded[:, 3::4] << 24)).astype(np.uint32)   # [T, W]
    n = states.shape[1]
    cursors = np.array([int(active[i]) | (0 << 4) | (((0 + 1) % n) << 8) | (((0 + 2) % n) << 12) | (int(turn[i]) << 16) | (int(inflight[i]) << 20) for i in range(t)], np.uint32)
    ss = np.zeros(t, np.uint64)
    for i in range(t):
        v = 0
        for p in range(n):
            if states[i, p] in (1, 2, 3):
                v |= 1 << (16 * (int(states[i, p]) - 1) + p)
        ss[i] = v
    return words.T.copy(), cursors, ss


def table_world(seed, n, t, turns=(1, 2, 3, 0)):
    """t hand-built tables of n seats: the betting rounds `turns` in turn, one step in flight (table 2), folded seats, -> dict."""
    rng = np.random.default_rng(seed)
    deck = np.array([[card(c) for c in rng.permutation(52)[:5 + 2 * n]] for _ in range(t)], np.uint8)
    turn = np.array([turns[i % len(turns)] for i in range(t)])        # (1 2 3 0: flop, turn, river, pre-flop)
    active = np.array([i % n for i in range(t)])
    states = np.ones((t, n), np.int64)
    for i in range(t):
        states[i, (i + 1) % n] = (0, 2, 3)[i % 3]                     # a folded, a called, an all-in seat
    inflight = np.zeros(t, np.int64)
    inflight[2 % t] = 0x13
    cards, cursors, ss = pack_tables(deck, turn, active, states, inflight)
    # the spots: every table once, and the three indices no table has
    tables = np.array(list(range(t)) + [-1, t, 2 ** 31 - 1, 0], np.int32)
    return dict(deck=deck, turn=turn, active=active, states=states, inflight=inflight, cards=cards, cursors=cursors, ss=ss, tables=tables, T=t, N=n)


def table_arrays(w):
    return {"T": ("u32", [w["T"]]), "N": ("u32", [w["N"]]), "cards": ("u32", w["cards"]), "cursors": ("u32", w["cursors"]),
            "seat_states": ("u64", w["ss"]), "tables": ("i32", w["tables"])}


def table_expect(w, per_table, zero_keys, count_key):
    """The table form's expected outputs from per_table (the spec's batch result over ALL T tables, as explicit spots): spot i is table
    tables[i]; a bad index is BAD_TABLE alone and zeros; a step in flight adds IN_FLIGHT and zeroes the spot's results."""
    tabs = w["tables"]
    out = {}
    for key, arr in per_table.items():
        out[key] = np.zeros((len(tabs),) + arr.shape[1:], arr.dtype)
    for i, t in enumerate(tabs.tolist()):
        if t < 0 or t >= w["T"]:
            out["status"][i] = BAD_TABLE
            continue
        for key in per_table:
            out[key][i] = per_table[key][t]
        if w["inflight"][t]:
            out["status"][i] |= IN_FLIGHT
            for key in zero_keys + (count_key,):
                out[key][i] = 0
    return out


# ---------------------------------------------------------------------------------------------------------------- rvr / hist
def rvr_like(name, family, shapes, seed, grid, wform=None, bins=None, outputs=None, quick=False, edit=None, wedit=None):
    board, nboard, dead = board_spots(seed, shapes)
    if edit:
        edit(board, nboard, dead)
    m = len(shapes)
    w, per_spot = weights_for(seed + 1, m, wform)
    if wedit:
        w = wedit(w, board, nboard, dead)
    arrays = {"m": ("u32", [m]), "grid": ("u32", [grid]), "board": ("u8", board), "nboard": ("u8", nboard), "dead": ("u64", dead),
              "weights": ("u16", w), "per_spot": ("u32", [per_spot])}
    if family == "hist":
        arrays["bins"] = ("u32", [bins])

    def expect():
        if family == "rvr":
            return VS.batch_rvr(board, nboard, dead, w)
        r = HS.batch_hist(board, nboard, dead, w, bins)
        return dict(r, void=r["void"])
    return Case(name, family, arrays, expect, outputs, quick)


def range_dead_on_some(w, board, nboard, dead):
    """Shared weights that live on ONE holding only: every completion that holds one of its cards leaves the range dead (hist: void)."""
    gone = VS.check_spot([int(x) for x in board[0]], int(nboard[0]), int(dead[0]))[1]
    pool = [c for c in range(52) if c not in gone]
    a, b = pool[1], pool[3]
    w = np.zeros(HOLDINGS, np.uint16)
    w[b * (b - 1) // 2 + a] = 7
    return w


def break_middle(board, nboard, dead):
    board[1, 1] = board[1, 0]                                         # the spot in the middle: a card twice -> refused


RIVER_DOWN = [(5, p) for p in (47, 46, 45, 33, 32, 24, 23, 17, 16, 12, 11, 4)]
TURN_SMALL = [(4, p) for p in (24, 23, 17, 16, 12, 11, 5)]


def rvr_hist_cases():
    cs = []
    for fam, bins in (("rvr", None), ("hist", 7)):
        # every boundary of the sort on river spots, the largest first on ONE workgroup: each spot starts from the LDS the larger one left
        cs.append(rvr_like(fam + "-river-bounds-grid1", fam, RIVER_DOWN, 11, 1, None, bins, quick=True))
        cs.append(rvr_like(fam + "-river-bounds-shared-w", fam, RIVER_DOWN[::-1], 12, 3, "shared", bins))
        # turn spots (P completions each) across npad 64|128, 128|256, 256|512 and the smallest pool, falling sizes on one workgroup
        cs.append(rvr_like(fam + "-turn-small-grid1-spot-w", fam, TURN_SMALL, 13, 1, "spot", bins, quick=True))
        cs.append(rvr_like(fam + "-turn-32-33", fam, [(4, 33), (4, 32)], 14, 1, "shared", bins))
        cs.append(rvr_like(fam + "-turn-45-46-47", fam, [(4, 47), (4, 46), (4, 45)], 15, 3, "spot", bins))
        # flop spots: the pair-order walk of ci / cj, 15 and 21 completions
        cs.append(rvr_like(fam + "-flop-6-7", fam, [(3, 7), (3, 6)], 16, 1, "shared", bins, quick=True))
        cs.append(rvr_like(fam + "-zero-weights", fam, [(4, 12), (5, 17)], 17, 2, "zero", bins))
        cs.append(rvr_like(fam + "-range-dies", fam, [(4, 12)], 18, 1, "shared", bins, wedit=range_dead_on_some, quick=True))
        cs.append(rvr_like(fam + "-refused-between", fam, [(5, 24), (4, 12), (5, 11)], 19, 1, None, bins, edit=break_middle, quick=True))
        for o in OUTPUTS[fam]:
            cs.append(rvr_like(fam + "-no-" + o, fam, [(5, 12), (4, 11)], 20, 1, "shared", bins, outputs=[x for x in OUTPUTS[fam] if x != o]))
        cs.append(status_case(fam, bins))
        cs.append(table_case(fam, bins))
    cs.append(rvr_like("hist-bins1", "hist", [(5, 33), (4, 12), (3, 6)], 21, 1, "shared", 1, quick=True))
    cs.append(rvr_like("hist-bins32", "hist", [(5, 33), (4, 12), (3, 6)], 22, 1, "spot", 32, quick=True))
    return cs


def status_case(fam, bins):
    """Every status bit of k_rvr_prep's explicit form, with a good spot at each end (boards / status / completions AND the rows: zeros)."""
    shapes = [(5, 12), (5, 12), (5, 12), (5, 12), (2, 20), (4, 12), (5, 12), (3, 12), (5, 11)]

    def edit(board, nboard, dead):
        board[1, 2] = 0x0D                                            # rank nibble 13: no card
        board[2, 3] = board[2, 0]                                     # a card twice
        nboard[3] = 6                                                 # no board size
        # [4]: nb = 2, pre-flop
        dead[5] = np.uint64(dead_mask([c for c in range(52) if card(c) not in [int(x) for x in board[5, :4]]][:44]))   # P = 4 < k + 4 = 5
        dead[6] = np.uint64(int(dead[6]) | (1 << 52))                 # a bit no card has
        dead[7] = np.uint64(int(dead[7]) | (1 << VS.canon_index(int(board[7, 0]))))   # a board card is also `dead`
    return rvr_like(fam + "-status-bits", fam, shapes, 23, 2, None, bins, edit=edit, quick=True)


def table_case(fam, bins):
    w = table_world(24, 2, 5, turns=(3, 0, 3))                        # river and pre-flop tables (a full-pool flop is 1 176 completions)
    arrays = dict(table_arrays(w), m=("u32", [len(w["tables"])]), grid=("u32", [2]))
    if fam == "hist":
        arrays["bins"] = ("u32", [bins])

    def expect():
        board, nboard = VS.table_boards(w["deck"], w["turn"])
        if fam == "rvr":
            r = VS.batch_rvr(board, nboard)
            return table_expect(w, {k: r[k] for k in OUTPUTS["rvr"]}, ("win", "tie", "tot"), "boards")
        r = HS.batch_hist(board, nboard, None, None, bins)
        return table_expect(w, {k: r[k] for k in OUTPUTS["hist"]}, ("hist", "void"), "completions")
    return Case(fam + "-table-form", fam, arrays, expect, quick=(fam == "rvr"))


# ---------------------------------------------------------------------------------------------------------------- range
def range_case(name, shapes, seed, grid, wform=None, outputs=None, quick=False, edit=None):
    hero, board, nboard, dead = hero_spots(seed, shapes)
    if edit:
        edit(hero, board, nboard, dead)
    m = len(shapes)
    w, per_spot = weights_for(seed + 1, m, wform)
    arrays = {"m": ("u32", [m]), "grid": ("u32", [grid]), "hero": ("u8", hero), "board": ("u8", board), "nboard": ("u8", nboard),
              "dead": ("u64", dead), "weights": ("u16", w), "per_spot": ("u32", [per_spot])}
    return Case(name, "range", arrays, lambda: RS.batch_range(hero, board, nboard, dead, w), outputs, quick)


def range_cases():
    cs = []
    # nb = 5, 4, 3 at the smallest pool (k + 2), k + 4, sets below 512 (C(12, 4) = 495) and no multiple of 512 (C(20, 3) = 1140, C(33, 2) = 528)
    small = [(5, 33), (5, 6), (5, 4), (5, 2), (4, 20), (4, 7), (4, 5), (4, 3), (3, 20), (3, 12), (3, 8), (3, 6), (3, 4)]
    cs.append(range_case("range-bounds-grid1", small, 31, 1, None, quick=True))
    cs.append(range_case("range-bounds-shared-w", small[::-1], 32, 3, "shared"))
    cs.append(range_case("range-full-pools", [(3, 47), (4, 46), (5, 45)], 33, 2, "spot"))
    # one workgroup, three spots, the largest first: the counters cleared for the next spot; without agg, and with per-spot weights
    cs.append(range_case("range-grid1-no-agg", [(4, 30), (3, 12), (5, 20)], 34, 1, "shared", outputs=("win", "tie", "boards", "status"), quick=True))
    cs.append(range_case("range-grid1-spot-w", [(4, 30), (3, 12), (5, 20)], 35, 1, "spot", quick=True))
    cs.append(range_case("range-agg-only", [(4, 12), (5, 20)], 36, 1, "shared", outputs=("agg",)))

    def middle(hero, board, nboard, dead):
        hero[1, 1] = board[1, 0]                                      # the hero holds a board card -> refused
    cs.append(range_case("range-refused-between", [(4, 20), (4, 12), (5, 11)], 37, 1, "shared", edit=middle, quick=True))

    def bits(hero, board, nboard, dead):
        hero[1, 0] = 0x4A                                             # suit 4: no card
        board[2, 2] = hero[2, 0]
        nboard[3] = 7
        # [4]: nb = 0, pre-flop
        used = [VS.canon_index(int(x)) for x in list(hero[5]) + list(board[5, :3])]
        dead[5] = np.uint64(dead_mask([c for c in range(52) if c not in used][:44]))      # P = 3 < k + 2 = 4
        dead[6] = np.uint64(1 << 63)
    cs.append(range_case("range-status-bits", [(5, 12), (5, 12), (5, 12), (5, 12), (0, 30), (3, 12), (5, 12), (4, 11)], 38, 2, None, edit=bits, quick=True))
    for observer, who in ((1, lambda w: np.full(w["T"], 1)), (-2, lambda w: w["active"])):
        w = table_world(39, 3, 5)
        arrays = dict(table_arrays(w), m=("u32", [len(w["tables"])]), grid=("u32", [2]), observer=("i32", [observer]))

        def expect(w=w, who=who):
            hero, board, nboard = RS.table_spots(w["deck"], w["turn"], who(w))
            r = RS.batch_range(hero, board, nboard)
            return table_expect(w, {k: r[k] for k in OUTPUTS["range"]}, ("agg", "win", "tie"), "boards")
        cs.append(Case("range-table-form-observer%d" % observer, "range", arrays, expect, quick=(observer == -2)))
    return cs


# ---------------------------------------------------------------------------------------------------------------- equity / sampled
def eq_lpt(m):
    return 16 if m < 16 else (64 if m < 256 else 1024)               # pk::eq_lpt


def seat_spots(seed, n, specs):
    """specs: [(nb, live mask or None = every seat, seats whose cards are unknown)] -> holes [m, n, 2], board, nboard, live."""
    rng = np.random.default_rng(seed)
    m = len(specs)
    holes, board = np.zeros((m, n, 2), np.uint8), np.zeros((m, 5), np.uint8)
    nboard, live = np.zeros(m, np.uint8), np.zeros(m, np.uint16)
    for i, (nb, lv, unknown) in enumerate(specs):
        vals = np.array([card(c) for c in rng.permutation(52)], np.uint8)
        board[i], holes[i], nboard[i] = vals[:5], vals[5:5 + 2 * n].reshape(n, 2), nb
        live[i] = (1 << n) - 1 if lv is None else lv
        for p in unknown:
            holes[i, p] = ES.UNKNOWN
    return holes, board, nboard, live


def equity_case(name, n, specs, seed, grid, outputs=None, quick=False, edit=None):
    holes, board, nboard, live = seat_spots(seed, n, specs)
    if edit:
        edit(holes, board, nboard, live)
    m = len(specs)
    arrays = {"N": ("u32", [n]), "m": ("u32", [m]), "grid": ("u32", [grid]), "lpt": ("u32", [eq_lpt(m)]), "pool_max": ("u32", [50]),
              "holes": ("u8", holes), "board": ("u8", board), "nboard": ("u8", nboard), "live": ("u16", live)}
    return Case(name, "equity", arrays, lambda: ES.batch_equity(holes, board, nboard, live), outputs, quick)


def equity_cases():
    cs = []
    # N = 2: nb = 2 is a spot of 15 tasks (C(46, 3) = 15 180 boards, 1 024 per task): more tasks than the 8 or 16 waves -> the counter path;
    # a folded seat with unknown cards, a lone live seat
    two = [(2, None, ()), (3, None, ()), (4, None, ()), (5, None, ()), (2, 0b01, (1,)), (3, 0b10, ()), (5, 0b10, (0,))]
    cs.append(equity_case("equity-N2-grid1", 2, two, 41, 1, quick=True))
    cs.append(equity_case("equity-N2-grid2", 2, two, 42, 2))
    cs.append(equity_case("equity-N3", 3, [(2, None, ()), (3, 0b101, (1,)), (4, 0b110, ()), (5, None, ()), (4, 0b010, (0, 2))], 43, 1, quick=True))
    cs.append(equity_case("equity-N9", 9, [(1, None, ()), (3, 0b101010101, (1, 3)), (5, None, ()), (4, 0b000010000, ()), (2, 0b111000111, ())], 44, 2))
    cs.append(equity_case("equity-N16", 16, [(0, None, ()), (1, 0xF0F0, ()), (2, None, ()), (5, 0x8001, ()), (3, 0x0100, ())], 45, 2))
    cs.append(equity_case("equity-N16-quick", 16, [(2, None, ()), (5, 0x8001, ()), (1, 0xF0F0, ())], 46, 1, quick=True))

    # 72 river spots of one task each on one workgroup: 68 tasks >= 8 per wave -> runs of four; four refused spots inside the batch
    def some_bad(holes, board, nboard, live):
        holes[5, 0, 0] = board[5, 1]
        live[20] = 0
        nboard[41] = 9
        holes[63, 1, 1] = 0x3D
    cs.append(equity_case("equity-take4", 2, [(5, None, ())] * 72, 47, 1, edit=some_bad, quick=True))
    cs.append(equity_case("equity-take4-N3-turn", 3, [(4, None, ())] * 70, 48, 1))
    for o in ("win", "tie", "share", "boards", "status"):
        cs.append(equity_case("equity-no-" + o, 3, [(4, None, ()), (5, 0b011, (2,))], 49, 1, outputs=[x for x in OUTPUTS["equity"] if x != o]))

    def bits(holes, board, nboard, live):
        holes[1, 0, 0] = 0x1F                                         # rank nibble 15
        holes[2, 1, 1] = board[2, 2]
        live[3] = 0
        nboard[4] = 6
        holes[5, 1] = ES.UNKNOWN                                      # a LIVE seat's cards must be known
    cs.append(equity_case("equity-status-bits", 2, [(5, None, ())] * 7, 50, 1, edit=bits, quick=True))
    for n in (2, 9):
        w = table_world(51 + n, n, 5, turns=(1, 2, 3, 0) if n == 9 else (1, 2, 3))   # (pre-flop at two seats is 1.7 million boards)
        arrays = dict(table_arrays(w), m=("u32", [len(w["tables"])]), grid=("u32", [2]), lpt=("u32", [16]), pool_max=("u32", [52 - 2 * n]))

        def expect(w=w):
            holes, board, nboard, live = ES.table_spots(w["deck"], w["states"], w["turn"])
            r = ES.batch_equity(holes, board, nboard, live)
            return table_expect(w, {k: r[k] for k in OUTPUTS["equity"]}, ("win", "tie", "share"), "boards")
        cs.append(Case("equity-table-form-N%d" % n, "equity", arrays, expect, quick=(n == 2)))
    return cs


def sampled_case(name, n, specs, seed, grid, samples, nonce=0, ids=None, lpt=None, quick=False, edit=None):
    holes, board, nboard, live = seat_spots(seed, n, specs)
    if edit:
        edit(holes, board, nboard, live)
    m = len(specs)
    key = R.seed_key(SS.DEFAULT_SEED + seed)
    arrays = {"N": ("u32", [n]), "m": ("u32", [m]), "grid": ("u32", [grid]), "samples": ("u32", [samples]), "nonce": ("u32", [nonce]),
              "key0": ("u32", [key[0]]), "key1": ("u32", [key[1]]), "ids": ("u32", ids), "lpt": ("u32", None if lpt is None else [lpt]),
              "holes": ("u8", holes), "board": ("u8", board), "nboard": ("u8", nboard), "live": ("u16", live)}
    return Case(name, "sampled", arrays, lambda: SS.batch_equity(holes, board, nboard, live, samples, nonce=nonce, ids=ids, key=key), None, quick)


def sampled_cases():
    cs = []
    # hidden hole cards: a seat's both, one byte, nobody's; a folded seat whose cards are simply in the pool
    two = [(3, None, (1,)), (0, None, (0, 1)), (5, None, ()), (4, 0b01, (1,)), (2, None, ())]

    def one_byte(holes, board, nboard, live):
        holes[4, 0, 1] = ES.UNKNOWN
    for s in (1, 63, 64, 65):
        cs.append(sampled_case("sampled-N2-S%d" % s, 2, two, 61, 1, s, edit=one_byte, quick=(s in (1, 65))))
    # several tasks per spot (512 samples per task at the smallest lpt), more tasks than waves on one workgroup; two nonces over the same spots
    for nonce in (0, 1):
        cs.append(sampled_case("sampled-N2-S1200-nonce%d" % nonce, 2, two, 61, 1, 1200, nonce=nonce, ids=[7, 7, 9, 2 ** 32 - 1, 0], edit=one_byte, quick=(nonce == 1)))
    six = [(3, None, (1, 2, 3, 4, 5)), (0, 0b101101, (0, 1, 2, 3, 4, 5)), (5, None, (2,)), (4, 0b000100, (2,))]
    cs.append(sampled_case("sampled-N6", 6, six, 62, 2, 200, quick=True))
    # 16 seats, everything hidden: 32 + k draws -- pre-flop 37, the third Philox block; the flop 34, the second
    all16 = tuple(range(16))
    cs.append(sampled_case("sampled-N16", 16, [(0, None, all16), (3, None, all16), (5, 0x00FF, all16), (4, None, ())], 63, 1, 130, quick=True))

    def bits(holes, board, nboard, live):
        holes[1, 0, 0] = 0x0E
        holes[2, 1, 1] = board[2, 2]
        live[3] = 0
        nboard[4] = 6
    cs.append(sampled_case("sampled-status-bits", 2, [(5, None, ())] * 6, 64, 1, 64, edit=bits, quick=True))
    for observer in (-1, -2, 1):
        w = table_world(65, 6, 5)
        key = R.seed_key(SS.DEFAULT_SEED)
        arrays = dict(table_arrays(w), m=("u32", [len(w["tables"])]), grid=("u32", [1]), samples=("u32", [65]), nonce=("u32", [3]), key0=("u32", [key[0]]),
                      key1=("u32", [key[1]]), id_base=("u32", [1000]), observer=("i32", [observer]))

        def expect(w=w, observer=observer, key=key):
            holes, board, nboard, live = SS.table_spots(w["deck"], w["states"], w["turn"], w["active"], observer)
            r = SS.batch_equity(holes, board, nboard, live, 65, nonce=3, ids=[1000 + t for t in range(w["T"])], key=key)
            return table_expect(w, {k: r[k] for k in OUTPUTS["sampled"]}, ("win", "tie", "share"), "samples")
        cs.append(Case("sampled-table-form-observer%d" % observer, "sampled", arrays, expect, quick=(observer == -2)))
    return cs


# ---------------------------------------------------------------------------------------------------------------- ranged
def ranged_case(name, n, specs, seed, grid, samples, weights=None, range_of=None, nonce=0, ids=None, lpt=None, quick=False, edit=None):
    """specs as seat_spots; range_of [m, n] (None: every hidden seat uniform); weights [R, 1326] or None."""
    holes, board, nboard, live = seat_spots(seed, n, specs)
    m = len(specs)
    ro = None if range_of is None else np.array(range_of, np.uint16).reshape(m, n)
    if edit:
        edit(holes, board, nboard, live, ro)
    key = R.seed_key(WS.DEFAULT_SEED + seed)
    w = None if weights is None else np.asarray(weights, np.uint16).reshape(-1, HOLDINGS)
    arrays = {"N": ("u32", [n]), "m": ("u32", [m]), "grid": ("u32", [grid]), "samples": ("u32", [samples]), "nonce": ("u32", [nonce]),
              "key0": ("u32", [key[0]]), "key1": ("u32", [key[1]]), "ids": ("u32", ids), "lpt": ("u32", None if lpt is None else [lpt]),
              "R": ("u32", [0 if w is None else len(w)]), "weights": ("u16", w), "range_of": ("u16", ro),
              "holes": ("u8", holes), "board": ("u8", board), "nboard": ("u8", nboard), "live": ("u16", live)}
    return Case(name, "ranged", arrays,
                lambda: WS.batch_equity(holes, board, nboard, live, samples, w, ro, per_spot=True, nonce=nonce, ids=ids, key=key), None, quick)


def ranged_cases():
    """The cases of k_eqw_cdf / k_eqw_prep / k_eqw<N, RC>; NOT part of all_cases() (tests/test_equity_sim_host.py pins that set)."""
    cs = []
    rng = np.random.default_rng(71)
    four = WS.random_ranges(rng)                                      # dense, ~40 holdings, one holding, all zero
    U = WS.UNIFORM
    # two seats: hero against one hidden hand on every street, each row and the uniform one; a dead range (accepted 0, status 0); nothing
    # hidden; a folded hidden seat (its 0xFF is simply in the pool)
    two = [(4, None, (1,)), (0, None, (1,)), (3, None, (1,)), (5, None, (0,)), (5, None, (1,)), (2, None, ()), (4, 0b01, (1,)), (0, None, (0, 1))]
    ro2 = [[U, 0], [U, 1], [U, U], [2, U], [U, 3], [0, 0], [0, 9], [1, 0]]
    for s in (1, 65):
        cs.append(ranged_case("ranged-N2-S%d-grid1" % s, 2, two, 72, 1, s, four, ro2, quick=True))
    # several tasks per spot (512 attempts per task at the smallest lpt) on ONE workgroup, whose LDS the tasks before have used; two nonces
    for nonce in (0, 1):
        cs.append(ranged_case("ranged-N2-S1200-grid1-nonce%d" % nonce, 2, two[:4], 72, 1, 1200, four, ro2[:4], nonce=nonce, ids=[7, 7, 9, 2 ** 32 - 1],
                              quick=(nonce == 0)))
    # R = 0: no cumulative row in LDS at all (size class 0), range_of NULL
    cs.append(ranged_case("ranged-N3-R0", 3, [(0, None, (1, 2)), (3, None, (0, 1, 2)), (5, 0b011, (1,))], 73, 1, 100, quick=True))
    # six seats, the observer shown: H = 5, a mix of rows; a refused spot between good ones (a card twice)
    six = [(0, None, (1, 2, 3, 4, 5)), (3, None, (1, 2, 3, 4, 5)), (4, 0b101101, (0, 2, 3, 5)), (5, None, (2,))]
    ro6 = [[U, 0, 1, U, 0, 1], [U, 0, 0, 0, 0, 0], [1, U, 0, 0, U, U], [U, U, 1, U, U, U]]

    def twice(holes, board, nboard, live, ro):
        holes[1, 0, 1] = board[1, 0]
    cs.append(ranged_case("ranged-N6", 6, six, 74, 2, 200, four, ro6, quick=True))
    cs.append(ranged_case("ranged-N6-refused-between", 6, six[:3], 74, 1, 70, four, ro6[:3], edit=twice, quick=True))
    # sixteen seats, everything hidden: H = 16, 17 words, 9 Philox blocks; sixteen rows, every one used (size class 16).  Row r lives on the
    # three holdings among the cards 3r .. 3r + 2, so sixteen holdings never collide and pre-flop every attempt is accepted; with the rows
    # handed out the other way round as well, with board cards dead (some rows lose holdings), and H = 15 with dense rows (nearly all rejected)
    sixteen = np.zeros((16, HOLDINGS), np.uint16)
    for r in range(16):
        for a, b in ((3 * r, 3 * r + 1), (3 * r, 3 * r + 2), (3 * r + 1, 3 * r + 2)):
            sixteen[r, b * (b - 1) // 2 + a] = int(rng.integers(1, 65536))
    all16 = tuple(range(16))
    cs.append(ranged_case("ranged-N16-H16-R16", 16, [(0, None, all16), (0, None, all16), (3, None, all16), (5, 0x00FF, all16)], 75, 1, 130, sixteen,
                          [list(range(16)), list(range(15, -1, -1)), list(range(16)), [U] * 8 + list(range(8))], quick=True))
    dense = np.zeros((9, HOLDINGS), np.uint16)
    for r in range(9):
        dense[r] = rng.integers(0, 300, HOLDINGS) * (rng.random(HOLDINGS) < 0.6)
    cs.append(ranged_case("ranged-N16-H15-R9-dense", 16, [(3, None, all16[1:])], 78, 1, 70, dense, [[r % 9 for r in range(16)]]))

    # the refusals: a half-hidden live seat, a row >= R at a hidden seat (and the same entry at a shown seat: ignored), a card twice, nb = 6, no
    # live seat, a byte that is no card -- good spots at both ends
    def bits(holes, board, nboard, live, ro):
        holes[1, 1, 1] = ES.UNKNOWN                                   # seat 1 shows one card
        ro[2, 1] = 4                                                  # R = 4: no such row, seat 1 hidden
        ro[3, 0] = 4                                                  # ... seat 0 shown: not read
        holes[4, 0, 1] = board[4, 2]
        nboard[5] = 6
        live[6] = 0
        holes[7, 0, 0] = 0x0E
    status_specs = [(5, None, (1,)), (5, None, ()), (4, None, (1,)), (4, None, (1,)), (5, None, (1,)), (5, None, (1,)), (5, None, (1,)), (3, None, (1,)), (5, None, (1,))]
    cs.append(ranged_case("ranged-status-bits", 2, status_specs, 76, 1, 64, four, [[U, 0]] * 9, edit=bits, quick=True))
    for observer, per in ((-2, 0), (1, 1)):
        w = table_world(77, 6, 5)
        key = R.seed_key(WS.DEFAULT_SEED)
        m = len(w["tables"])
        ro = np.array([[0, 1, U, 0, 1, 2]] * (m if per else 1), np.uint16)
        if per:
            ro[1] = [1, 1, 1, 1, 1, 1]
        arrays = dict(table_arrays(w), m=("u32", [m]), grid=("u32", [1]), samples=("u32", [65]), nonce=("u32", [3]), key0=("u32", [key[0]]),
                      key1=("u32", [key[1]]), id_base=("u32", [1000]), observer=("i32", [observer]), R=("u32", [4]), weights=("u16", four),
                      range_of=("u16", ro), per_spot=("u32", [per]))

        def expect(w=w, observer=observer, key=key, ro=ro, per=per):
            holes, board, nboard, live = WS.table_spots(w["deck"], w["states"], w["turn"], w["active"], observer)
            tabs = w["tables"].tolist()
            # range_of goes by SPOT: evaluate per spot, then pick (a shared vector: by table is the same)
            if not per:
                r = WS.batch_equity(holes, board, nboard, live, 65, four, ro[0], nonce=3, ids=[1000 + t for t in range(w["T"])], key=key)
                return table_expect(w, {k: r[k] for k in OUTPUTS["ranged"]}, ("win", "tie", "share"), "accepted")
            good = [(i, t) for i, t in enumerate(tabs) if 0 <= t < w["T"]]
            idx = [t for _, t in good]
            r = WS.batch_equity(holes[idx], board[idx], nboard[idx], live[idx], 65, four, ro[[i for i, _ in good]], per_spot=True, nonce=3,
                                ids=[1000 + t for t in idx], key=key)
            out = {k: np.zeros((len(tabs),) + r[k].shape[1:], r[k].dtype) for k in OUTPUTS["ranged"]}
            for i, t in enumerate(tabs):
                if not 0 <= t < w["T"]:
                    out["status"][i] = BAD_TABLE
            for j, (i, t) in enumerate(good):
                for k in out:
                    out[k][i] = r[k][j]
                if w["inflight"][t]:
                    out["status"][i] |= IN_FLIGHT
                    for k in ("win", "tie", "share", "accepted"):
                        out[k][i] = 0
            return out
        cs.append(Case("ranged-table-form-observer%d" % observer, "ranged", arrays, expect, quick=True))
    assert len({c.name for c in cs}) == len(cs)
    return cs


# ---------------------------------------------------------------------------------------------------------------- ev
def f64_bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def ev_expect(r):
    return dict(r, amount=f64_bits(r["amount"]), ev=f64_bits(r["ev"]))


def ev_case(name, n, specs, bets, seed, grid, outputs=None, quick=False, edit=None):
    """specs as seat_spots; bets [m][n] (a short row is padded with its last value)."""
    holes, board, nboard, live = seat_spots(seed, n, specs)
    m = len(specs)
    b = np.array([list(row) + [row[-1]] * (n - len(row)) for row in bets], np.float64)
    assert b.shape == (m, n)
    if edit:
        edit(holes, board, nboard, live, b)
    arrays = {"N": ("u32", [n]), "m": ("u32", [m]), "grid": ("u32", [grid]), "lpt": ("u32", [eq_lpt(m)]), "pool_max": ("u32", [50]),
              "holes": ("u8", holes), "board": ("u8", board), "nboard": ("u8", nboard), "live": ("u16", live), "bets": ("u64", f64_bits(b))}
    return Case(name, "ev", arrays, lambda: ev_expect(EV.batch_ev(holes, board, nboard, live, b)), outputs, quick)


def ev_cases():
    cs = []
    ladder = lambda n: [5.0 * (p + 1) for p in range(n)]
    # a grid of 1, spots of falling size with different levels: what a spot leaves in LDS and in the level table must not reach the next
    two = [(2, None, ()), (3, None, ()), (4, None, ()), (5, None, ()), (3, 0b01, (1,)), (5, 0b10, (0,)), (4, None, ())]
    cs.append(ev_case("ev-N2-grid1", 2, two, [[10, 37], [20, 20], [50, 5], [0, 10], [10, 37], [5, 5], [0, 0]], 71, 1, quick=True))
    cs.append(ev_case("ev-N2-grid2", 2, two, [[10, 37], [20, 20], [50, 5], [0, 10], [10, 37], [5, 5], [0, 0]], 72, 2))
    three = [(3, None, ()), (4, 0b101, (1,)), (5, None, ()), (4, None, ()), (5, 0b010, (0, 2)), (4, 0b110, ())]
    cs.append(ev_case("ev-N3-grid1", 3, three, [[30, 10, 20], [10, 50, 10], [10, 10, 10], [0, 10, 10], [5, 7, 9], [50, 20, 20]], 73, 1, quick=True))

    # a refused spot between two valid ones: a bad bet, a duplicate card, no live seat, a NaN, an infinity
    def refuse(holes, board, nboard, live, b):
        b[1, 2] = -1.0
        holes[3, 0, 0] = board[3, 1]
        live[5] = 0
        b[7, 0] = np.nan
        b[7, 1] = np.inf
    cs.append(ev_case("ev-N3-refused-between", 3, [(4, None, ())] * 9, [ladder(3)] * 9, 74, 1, edit=refuse, quick=True))
    # five live seats on a ladder: four levels to compare = two groups of three; then fewer levels in the same slots
    five = [(4, None, ()), (5, None, ()), (4, 0b10111, ()), (5, 0b00100, ()), (4, None, ())]
    cs.append(ev_case("ev-N5-two-groups", 5, five, [ladder(5), ladder(5)[::-1], [50, 5, 5, 50, 20], ladder(5), [10] * 5], 75, 1, quick=True))
    cs.append(ev_case("ev-N9-ladder", 9, [(3, None, ()), (5, 0b101010101, (1, 3)), (4, None, ())], [ladder(9), ladder(9), [0, 5, 5, 37, 37, 50, 10, 20, 20]], 76, 2))
    cs.append(ev_case("ev-N16-ladder", 16, [(3, None, ()), (5, 0x8001, ()), (4, 0xF0F0, ())], [ladder(16)] * 3, 77, 2))
    cs.append(ev_case("ev-N16-quick", 16, [(4, None, ()), (5, 0xF0F0, ())], [ladder(16), ladder(16)[::-1]], 78, 1, quick=True))
    # 72 river spots of one task each on one workgroup: runs of four
    cs.append(ev_case("ev-take4", 2, [(5, None, ())] * 72, [[10, 37], [5, 5], [20, 0]] * 24, 79, 1, quick=True))
    for o in ("share", "level_seat", "amount", "ev", "boards"):
        cs.append(ev_case("ev-no-" + o, 3, [(4, None, ()), (5, 0b011, (2,))], [[30, 10, 20], [10, 5, 50]], 80, 1, outputs=[x for x in OUTPUTS["ev"] if x != o], quick=(o == "share")))
    for n in (3, 9):
        w = table_world(81 + n, n, 5, turns=(1, 2, 3))
        rng = np.random.default_rng(90 + n)
        tb = rng.choice([0.0, 5.0, 10.0, 20.0, 37.5], (w["T"], n))
        tp = rng.choice([0.0, 0.0, 2.5, 10.0], (w["T"], n))
        arrays = dict(table_arrays(w), m=("u32", [len(w["tables"])]), grid=("u32", [2]), lpt=("u32", [16]), pool_max=("u32", [52 - 2 * n]),
                      bets=("u64", f64_bits(tb.T.copy())), pending=("u64", f64_bits(tp.T.copy())))

        def expect(w=w, tb=tb, tp=tp):
            holes, board, nboard, live = ES.table_spots(w["deck"], w["states"], w["turn"])
            r = EV.batch_ev(holes, board, nboard, live, tb + tp)
            out = table_expect(w, {k: r[k] for k in OUTPUTS["ev"]}, ("share", "amount", "ev", "level_seat"), "boards")
            out["level_seat"][out["status"] != 0] = EV.NO_LEVEL
            return ev_expect(out)
        cs.append(Case("ev-table-form-N%d" % n, "ev", arrays, expect, quick=(n == 3)))
    assert len({c.name for c in cs}) == len(cs)
    return cs


# ---------------------------------------------------------------------------------------------------------------- ranged ev
def ranged_ev_case(name, n, specs, bets, seed, grid, samples, weights=None, range_of=None, nonce=0, ids=None, lpt=None, outputs=None, quick=False,
                   edit=None):
    """specs as seat_spots; bets [m][n] (a short row is padded with its last value); range_of [m, n] (None: every hidden seat uniform);
    weights [R, 1326] or None."""
    holes, board, nboard, live = seat_spots(seed, n, specs)
    m = len(specs)
    b = np.array([list(row) + [row[-1]] * (n - len(row)) for row in bets], np.float64)
    assert b.shape == (m, n)
    ro = None if range_of is None else np.array(range_of, np.uint16).reshape(m, n)
    if edit:
        edit(holes, board, nboard, live, ro, b)
    key = R.seed_key(WS.DEFAULT_SEED + seed)
    w = None if weights is None else np.asarray(weights, np.uint16).reshape(-1, HOLDINGS)
    arrays = {"N": ("u32", [n]), "m": ("u32", [m]), "grid": ("u32", [grid]), "samples": ("u32", [samples]), "nonce": ("u32", [nonce]),
              "key0": ("u32", [key[0]]), "key1": ("u32", [key[1]]), "ids": ("u32", ids), "lpt": ("u32", None if lpt is None else [lpt]),
              "R": ("u32", [0 if w is None else len(w)]), "weights": ("u16", w), "range_of": ("u16", ro),
              "holes": ("u8", holes), "board": ("u8", board), "nboard": ("u8", nboard), "live": ("u16", live), "bets": ("u64", f64_bits(b))}
    return Case(name, "rangedev", arrays,
                lambda: ev_expect(XS.batch_ev(holes, board, nboard, live, b, samples, w, ro, per_spot=True, nonce=nonce, ids=ids, key=key)), outputs, quick)


def ranged_ev_cases():
    """The cases of k_evw_prep<N, TABLE> / k_evw<N, RC> / k_evw_finish (family "rangedev", names evw-...: `--only ranged` and `--only ev-` do not
    pick them up); NOT part of all_cases()."""
    cs = []
    rng = np.random.default_rng(71)
    four = WS.random_ranges(rng)                                      # dense, ~40 holdings, one holding, all zero
    U = WS.UNIFORM
    ladder = lambda n: [5.0 * (p + 1) for p in range(n)]
    # a grid of 1, spots with different levels after each other: what a spot leaves in LDS and in the level table must not reach the next;
    # every street, each row and the uniform one, nothing hidden, a folded hidden seat, all bets zero
    two = [(4, None, (1,)), (0, None, (1,)), (3, None, (1,)), (5, None, (0,)), (5, None, (1,)), (2, None, ()), (4, 0b01, (1,)), (0, None, (0, 1))]
    ro2 = [[U, 0], [U, 1], [U, U], [2, U], [U, 3], [0, 0], [0, 9], [1, 0]]
    bets2 = [[10, 37], [20, 20], [50, 5], [0, 10], [10, 37], [5, 5], [10, 37], [0, 0]]
    cs.append(ranged_ev_case("evw-N2-S65-grid1", 2, two, bets2, 72, 1, 65, four, ro2, quick=True))
    three = [(3, None, (1, 2)), (4, 0b101, (1, 2)), (5, None, (2,)), (0, None, (0, 1, 2)), (5, 0b010, (0, 2)), (4, 0b110, (1, 2))]
    ro3 = [[U, 0, 1], [U, 0, 0], [U, U, 1], [0, U, 1], [U, 0, U], [1, 0, U]]
    cs.append(ranged_ev_case("evw-N3-grid1", 3, three, [[30, 10, 20], [10, 50, 10], [10, 10, 10], [0, 10, 10], [5, 7, 9], [50, 20, 20]], 73, 1, 100, four, ro3,
                             quick=True))
    # S = 200: one chunk, a ragged run of lanes; S = 1 200: several chunks (512 attempts a chunk at the smallest lpt) on ONE workgroup, two nonces
    cs.append(ranged_ev_case("evw-N3-S200", 3, three[:3], [[30, 10, 20], [10, 50, 10], [20, 20, 5]], 73, 2, 200, four, ro3[:3], quick=True))
    for nonce in (0, 1):
        cs.append(ranged_ev_case("evw-N3-S1200-grid1-nonce%d" % nonce, 3, three[:3], [[30, 10, 20], [10, 50, 10], [20, 20, 5]], 73, 1, 1200, four, ro3[:3],
                                 nonce=nonce, ids=[7, 7, 2 ** 32 - 1], quick=(nonce == 0)))
    # R = 0: no cumulative row in LDS at all (size class 0), range_of NULL
    cs.append(ranged_ev_case("evw-N3-R0", 3, [(0, None, (1, 2)), (3, None, (0, 1, 2)), (5, 0b011, (1,))], [[30, 10, 20], [5, 5, 5], [10, 50, 10]], 74, 1, 100,
                             quick=True))
    # an all-zero range at a hidden seat: accepted 0, status 0 -- group 0 still runs, nothing is evaluated; the levels are still reported
    cs.append(ranged_ev_case("evw-N3-dead-range", 3, [(4, None, (1, 2)), (4, None, (1, 2)), (4, None, (1, 2))], [[30, 10, 20]] * 3, 75, 1, 70, four,
                             [[U, 0, 1], [U, 3, 0], [U, 0, 1]], quick=True))

    # a refused spot between valid ones: a bad bet, a half-hidden live seat (BAD_CARD), a NaN with an infinity, no live seat
    def refuse(holes, board, nboard, live, ro, b):
        b[1, 2] = -1.0
        holes[3, 1, 1] = [c for c in ES.CANON if c not in set(holes[3].reshape(-1).tolist()) | set(board[3].tolist())][0]
        live[5] = 0
        b[7, 0] = np.nan
        b[7, 1] = np.inf
        b[8, 0] = -0.0                                                # -0.0 is a zero
    cs.append(ranged_ev_case("evw-N3-refused-between", 3, [(4, None, (1, 2))] * 9, [ladder(3)] * 9, 76, 1, 70, four, [[U, 0, 1]] * 9, edit=refuse, quick=True))
    # five live seats on a ladder with two hidden seats: four levels to compare = two groups of three; then fewer levels in the same slots
    five = [(4, None, (1, 3)), (5, None, (0, 4)), (4, 0b10111, (1, 2)), (5, 0b00100, (2,)), (3, None, (1, 3))]
    ro5 = [[U, 0, U, 1, U], [1, U, U, U, 0], [U, 0, U, U, U], [U, U, 1, U, U], [U, 0, U, 0, U]]
    cs.append(ranged_ev_case("evw-N5-two-groups", 5, five, [ladder(5), ladder(5)[::-1], [50, 5, 5, 50, 20], ladder(5), [10] * 5], 77, 1, 100, four, ro5, quick=True))
    # nine seats with size class 16, sixteen seats on a ladder: two-level groups, four and eight of them.  Row r lives on the three holdings among
    # the cards 3r .. 3r + 2, so the drawn holdings never collide with each other
    sixteen = np.zeros((16, HOLDINGS), np.uint16)
    for r in range(16):
        for a, b in ((3 * r, 3 * r + 1), (3 * r, 3 * r + 2), (3 * r + 1, 3 * r + 2)):
            sixteen[r, b * (b - 1) // 2 + a] = int(rng.integers(1, 65536))
    all9, all16 = tuple(range(9)), tuple(range(16))
    cs.append(ranged_ev_case("evw-N9-R16", 9, [(0, None, all9), (3, 0b101010111, all9)], [ladder(9), [0, 5, 5, 37, 37, 50, 10, 20, 20]], 78, 1, 66, sixteen,
                             [list(range(9)), [15, 14, 13, U, 11, 10, 9, 8, 7]], quick=True))
    cs.append(ranged_ev_case("evw-N16-ladder", 16, [(0, None, all16), (3, 0xF0F7, all16)], [ladder(16), ladder(16)[::-1]], 79, 1, 66, sixteen,
                             [list(range(16)), list(range(15, -1, -1))], quick=True))
    cs.append(ranged_ev_case("evw-N16-ladder-grid2", 16, [(0, None, all16), (4, None, all16), (5, 0x8001, all16)], [ladder(16)] * 3, 80, 2, 130, sixteen,
                             [list(range(16))] * 3))
    for o in ("share", "level_seat", "amount", "ev", "accepted"):
        cs.append(ranged_ev_case("evw-no-" + o, 3, three[:2], [[30, 10, 20], [10, 5, 50]], 81, 1, 70, four, ro3[:2],
                                 outputs=[x for x in OUTPUTS["rangedev"] if x != o], quick=(o in ("share", "accepted"))))
    for observer, per in ((-2, 0), (1, 1)):
        w = table_world(82, 3, 5)
        key = R.seed_key(WS.DEFAULT_SEED)
        m = len(w["tables"])
        ro = np.array([[0, 1, U]] * (m if per else 1), np.uint16)
        if per:
            ro[1] = [1, 1, 1]
        trng = np.random.default_rng(90)
        tb = trng.choice([0.0, 5.0, 10.0, 20.0, 37.5], (w["T"], 3))
        tp = trng.choice([0.0, 0.0, 2.5, 10.0], (w["T"], 3))
        arrays = dict(table_arrays(w), m=("u32", [m]), grid=("u32", [1]), samples=("u32", [65]), nonce=("u32", [3]), key0=("u32", [key[0]]),
                      key1=("u32", [key[1]]), id_base=("u32", [1000]), observer=("i32", [observer]), R=("u32", [4]), weights=("u16", four),
                      range_of=("u16", ro), per_spot=("u32", [per]), bets=("u64", f64_bits(tb.T.copy())), pending=("u64", f64_bits(tp.T.copy())))

        def expect(w=w, observer=observer, key=key, ro=ro, per=per, tb=tb, tp=tp):
            holes, board, nboard, live, bets = XS.table_spots(w["deck"], w["states"], w["turn"], w["active"], observer, tb, tp)
            tabs = w["tables"].tolist()
            good = [(i, t) for i, t in enumerate(tabs) if 0 <= t < w["T"]]      # range_of goes by SPOT: evaluate per spot
            idx = [t for _, t in good]
            rows = ro[[i for i, _ in good]] if per else np.tile(ro[0], (len(good), 1))
            r = XS.batch_ev(holes[idx], board[idx], nboard[idx], live[idx], bets[idx], 65, four, rows, per_spot=True, nonce=3,
                            ids=[1000 + t for t in idx], key=key)
            out = {k: np.zeros((len(tabs),) + r[k].shape[1:], r[k].dtype) for k in OUTPUTS["rangedev"]}
            out["level_seat"][:] = XS.NO_LEVEL
            for i, t in enumerate(tabs):
                if not 0 <= t < w["T"]:
                    out["status"][i] = BAD_TABLE
            for j, (i, t) in enumerate(good):
                for k in out:
                    out[k][i] = r[k][j]
                if w["inflight"][t]:
                    out["status"][i] |= IN_FLIGHT
                    for k in ("share", "amount", "ev", "accepted"):
                        out[k][i] = 0
                    out["level_seat"][i] = XS.NO_LEVEL
            return ev_expect(out)
        cs.append(Case("evw-table-form-observer%d" % observer, "rangedev", arrays, expect, quick=True))
    assert len({c.name for c in cs}) == len(cs) and all(c.name.startswith("evw-") for c in cs)
    return cs


# ---------------------------------------------------------------------------------------------------------------- histogram clustering
def cluster_case(name, op, hist, K, grid, centroids=None, iters=None, seed=None, nonce=0, chunk=None, lds=None, skew=0, quick=False):
    """op 0: seeding -> centroids; 1: assign -> label, dist; 2: `iters` iterations and the final assign.  Expected: tests/hist_cluster_spec.py."""
    hist = np.ascontiguousarray(hist, np.uint16)
    n, nbins = hist.shape
    arrays = {"n": ("u32", [n]), "nbins": ("u32", [nbins]), "K": ("u32", [K]), "op": ("u32", [op]), "grid": ("u32", [grid]),
              "skew": ("u32", [skew]), "hist": ("u16", np.concatenate([np.full(skew, 0xABCD, np.uint16), hist.reshape(-1)]))}
    if chunk is not None:
        arrays["chunk"] = ("u32", [chunk])
    if lds is not None:
        arrays["lds"] = ("u32", [lds])
    if op == 0:
        arrays.update(key0=("u32", [seed & 0xFFFFFFFF]), key1=("u32", [seed >> 32]), nonce=("u32", [nonce]))

        def expect():
            q, empty = CS.quant(hist)
            return {"centroids": CS.seed(q, empty, K, seed, nonce)[0]}
        return Case(name, "cluster", arrays, expect, ("centroids",), quick)
    centroids = np.ascontiguousarray(centroids, np.uint16)
    assert centroids.shape == (K, nbins)
    arrays["centroids"] = ("u16", centroids)
    if op == 1:
        def expect():
            q, empty = CS.quant(hist)
            label, dist = CS.assign(q, empty, centroids)
            return {"label": label, "dist": dist}
        return Case(name, "cluster", arrays, expect, ("label", "dist"), quick)
    arrays["iters"] = ("u32", [iters])

    def expect():
        q, empty = CS.quant(hist)
        r = CS.iterate(q, empty, centroids, iters)
        return {"centroids_out": r["centroids"], "label": r["labels"], "dist": r["dist"], "inertia": r["inertia"], "changed": r["changed"]}
    return Case(name, "cluster", arrays, expect, None, quick)


def cluster_rows(seed, n, nbins, empties=()):
    rng = np.random.default_rng(seed)
    hist = CS.latent_rows(rng, n, nbins, mass=46, shapes=5, empty_frac=0.1)
    for a, b in empties:
        hist[a:b] = 0
    return hist


def cluster_centroids(seed, hist, K):
    """K centroids near the data: the q of random non-empty rows, some nudged (kept non-decreasing)."""
    rng = np.random.default_rng(seed)
    q, empty = CS.quant(hist)
    C = q[rng.choice(np.flatnonzero(~empty), K)].astype(np.int64)
    C[::2] = np.sort(np.clip(C[::2] + rng.integers(-900, 900, C[::2].shape), 0, 65535), axis=1)
    return C.astype(np.uint16)


def cluster_cases():
    cs = []
    for nbins in (1, 2, 7, 10, 32):
        # 300 rows = two workgroups' worth on a grid of 1: the workgroup strides; empty rows first, last and as a whole wave; an unaligned pointer
        hist = cluster_rows(200 + nbins, 300, nbins, empties=((0, 3), (64, 128), (297, 300)))
        cs.append(cluster_case("cluster-assign-b%d" % nbins, 1, hist, 5, 1, centroids=cluster_centroids(1, hist, 5), skew=(nbins % 3), quick=True))
        cs.append(cluster_case("cluster-iterate-b%d" % nbins, 2, hist, 6, 2, centroids=cluster_centroids(2, hist, 6), iters=3, quick=nbins in (7, 32)))
    # assign takes any K: one row and 63 rows against 2, 3 (one more than the kernel's unroll of two) and more centroids than rows
    wide = cluster_rows(209, 400, 10)
    for n, K in ((1, 2), (1, 3), (1, 70), (63, 2), (63, 3), (63, 70)):
        few = wide[wide.any(axis=1)][:n] if n == 1 else wide[:n]
        cs.append(cluster_case("cluster-assign-n%d-K%d" % (n, K), 1, few, K, 1, centroids=cluster_centroids(10 + K, wide, K), quick=True))
    hist = cluster_rows(210, 700, 7, empties=((640, 700),))
    cs.append(cluster_case("cluster-iterate-global-sums", 2, hist, 9, 2, centroids=cluster_centroids(3, hist, 9), iters=2, lds=0, quick=True))
    cs.append(cluster_case("cluster-iterate-K1", 2, hist[:65], 1, 1, centroids=cluster_centroids(4, hist, 1), iters=2, quick=True))
    # ties: duplicated rows, two identical centroids (the smaller index wins, the larger stays empty and keeps its centroid), a row midway
    t = np.zeros((70, 4), np.uint16)
    t[:, 3] = 4
    t[::3] = [4, 0, 0, 0]
    t[1::3] = [0, 0, 0, 4]
    t[2::3] = [2, 0, 0, 2]                                            # q = (32767, 32767, 32767, 65535): between the two below
    t[5] = 0
    tc = np.array([[65535, 65535, 65535, 65535], [0, 0, 0, 65535], [0, 0, 0, 65535], [65534, 65535, 65535, 65535]], np.uint16)
    cs.append(cluster_case("cluster-ties-assign", 1, t, 4, 1, centroids=tc, quick=True))
    cs.append(cluster_case("cluster-ties-iterate", 2, t, 4, 1, centroids=tc, iters=2, quick=True))
    # seeding: three chunks of one tile, two chunks of two tiles, one row; K = 1, 2, 33
    for K, chunk in ((1, 256), (2, 256), (33, 256), (5, 512)):
        cs.append(cluster_case("cluster-seed-K%d-chunk%d" % (K, chunk), 0, hist, K, 2, seed=R.DEFAULT_SEED + K, nonce=K, chunk=chunk, quick=K != 2))
    cs.append(cluster_case("cluster-seed-one-row", 0, hist[:1], 1, 1, seed=7, quick=True))
    same = np.zeros((300, 10), np.uint16)
    same[:] = [1, 0, 3, 0, 0, 9, 0, 0, 2, 1]
    same[:70] = 0
    same[200:264] = 0
    cs.append(cluster_case("cluster-seed-identical-rows", 0, same, 3, 1, seed=11, nonce=2, quick=True))   # W = 0 from round 1 on
    cs.append(cluster_case("cluster-iterate-identical-rows", 2, same, 3, 1, centroids=np.tile(CS.quant(same)[0][70], (3, 1)), iters=1, quick=True))
    assert len({c.name for c in cs}) == len(cs) and all(c.name.startswith("cluster-") for c in cs)
    return cs


# ---------------------------------------------------------------------------------------------------------------- hero histograms
def hero_hist_case(name, shapes, seed, grid, bins, wform=None, outputs=None, quick=False, edit=None):
    hero, board, nboard, dead = hero_spots(seed, shapes)
    if edit:
        edit(hero, board, nboard, dead)
    m = len(shapes)
    w, per_spot = weights_for(seed + 1, m, wform)
    arrays = {"m": ("u32", [m]), "grid": ("u32", [grid]), "bins": ("u32", [bins]), "hero": ("u8", hero), "board": ("u8", board), "nboard": ("u8", nboard),
              "dead": ("u64", dead), "weights": ("u16", w), "per_spot": ("u32", [per_spot])}
    return Case(name, "herohist", arrays, lambda: HHS.batch_hero_hist(hero, board, nboard, dead, w, bins), outputs, quick)


def hero_hist_cases():
    """The cases of k_hero_hist: a list of its own (all_cases() and cluster_cases() are counted by their tests)."""
    cs = []
    # nb = 5, 4, 3 at the smallest pool (k + 2), sets below 512 (C(12, 4) = 495) and no multiple of 512 (C(20, 3) = 1140, C(33, 2) = 528), river spots
    # (one completion); ONE workgroup, the largest first: the counters cleared for the next spot
    small = [(5, 33), (5, 6), (5, 2), (4, 20), (4, 7), (4, 3), (3, 12), (3, 8), (3, 4)]
    cs.append(hero_hist_case("herohist-bounds-grid1", small, 51, 1, 7, None, quick=True))
    cs.append(hero_hist_case("herohist-bounds-shared-w", small[::-1], 52, 3, 10, "shared"))
    cs.append(hero_hist_case("herohist-full-pools", [(3, 47), (4, 46), (5, 45)], 53, 2, 10, "spot"))
    cs.append(hero_hist_case("herohist-grid1-spot-w", [(4, 30), (3, 12), (5, 20)], 54, 1, 10, "spot", quick=True))
    cs.append(hero_hist_case("herohist-two-spots-grid1", [(3, 10), (3, 9)], 55, 1, 32, "shared", quick=True))
    cs.append(hero_hist_case("herohist-river-alone", [(5, 47)], 56, 1, 2, "shared", quick=True))
    cs.append(hero_hist_case("herohist-zero-weights", [(4, 12), (5, 17), (3, 7)], 57, 2, 7, "zero", quick=True))
    cs.append(hero_hist_case("herohist-bins1", [(5, 33), (4, 12), (3, 6)], 58, 1, 1, "shared", quick=True))

    def middle(hero, board, nboard, dead):
        hero[1, 1] = board[1, 0]                                      # the hero holds a board card -> refused
    cs.append(hero_hist_case("herohist-refused-between", [(4, 20), (4, 12), (5, 11)], 59, 1, 7, "shared", edit=middle, quick=True))
    for o in OUTPUTS["herohist"]:
        cs.append(hero_hist_case("herohist-no-" + o, [(5, 12), (4, 11)], 60, 1, 7, "shared", outputs=[x for x in OUTPUTS["herohist"] if x != o]))

    def bits(hero, board, nboard, dead):
        hero[1, 0] = 0x4A                                             # suit 4: no card
        board[2, 2] = hero[2, 0]
        nboard[3] = 7
        # [4]: nb = 0, pre-flop
        used = [VS.canon_index(int(x)) for x in list(hero[5]) + list(board[5, :3])]
        dead[5] = np.uint64(dead_mask([c for c in range(52) if c not in used][:44]))      # P = 3 < k + 2 = 4
        dead[6] = np.uint64(1 << 63)
    cs.append(hero_hist_case("herohist-status-bits", [(5, 12), (5, 12), (5, 12), (5, 12), (0, 30), (3, 12), (5, 12), (4, 11)], 61, 2, 7, None, edit=bits, quick=True))
    for observer, who in ((1, lambda w: np.full(w["T"], 1)), (-2, lambda w: w["active"])):
        w = table_world(62, 3, 5, turns=(3, 0, 2))                    # river, pre-flop and turn tables (a full-pool flop is 178 365 sets)
        arrays = dict(table_arrays(w), m=("u32", [len(w["tables"])]), grid=("u32", [2]), bins=("u32", [10]), observer=("i32", [observer]))

        def expect(w=w, who=who):
            hero, board, nboard = RS.table_spots(w["deck"], w["turn"], who(w))
            r = HHS.batch_hero_hist(hero, board, nboard, None, None, 10)
            return table_expect(w, {k: r[k] for k in OUTPUTS["herohist"]}, ("hist", "void"), "completions")
        cs.append(Case("herohist-table-form-observer%d" % observer, "herohist", arrays, expect, quick=(observer == -2)))
    assert len({c.name for c in cs}) == len(cs)
    return cs


# ---------------------------------------------------------------------------------------------------------------- pre-flop partial counts
OUT_FILL = 0xA5A5A5A5       # what the driver's output arrays hold before the launch


def preflop_case(name, first, n, chunk, accumulate=0, outputs=None, quick=False):
    arrays = {"first": ("u32", [first]), "n": ("u32", [n]), "chunk": ("u32", [chunk]), "accumulate": ("u32", [accumulate])}

    def expect():
        win, tie = PS.counts(first, n)
        if accumulate:                                                # (added to what the arrays held, modulo 2^32)
            win, tie = win + np.uint32(OUT_FILL), tie + np.uint32(OUT_FILL)
        return {"win": win, "tie": tie}
    return Case(name, "preflop", arrays, expect, outputs, quick)


def preflop_cases():
    """The cases of k_pfm_rank + k_pfm_count: a list of its own.  Boards from rank 1 000 000 on hold middling cards; from 0 on, the lowest."""
    cs = [preflop_case("preflop-one-board-first", 0, 1, 64, quick=True),
          preflop_case("preflop-one-board-last", PS.ALL_BOARDS - 1, 1, 64, quick=True),
          # 100 boards in chunks of 40: a storing launch of one slice (32 boards), then 40 and a ragged 28; two slices per chunk, the second ragged
          preflop_case("preflop-100-boards-chunk40", 1000003, 100, 40, quick=True),
          preflop_case("preflop-accumulate-33-boards", 17, 33, 32, accumulate=1, quick=True),
          preflop_case("preflop-win-alone", 2000000, 5, 64, outputs=("win",)),
          preflop_case("preflop-tie-alone", 2000000, 5, 64, outputs=("tie",)),
          # a chunk below one run of boards: the storing launch is capped at the chunk (the key work space holds exactly one chunk)
          preflop_case("preflop-40-boards-chunk5", 1234567, 40, 5, quick=True),
          preflop_case("preflop-accumulate-chunk1", 99, 3, 1, accumulate=1),
          preflop_case("preflop-300-boards-chunk128", 2598960 - 300, 300, 128)]
    cs += preflop_reader_cases()
    assert len({c.name for c in cs}) == len(cs)
    return cs


_pf_table = []


def preflop_table():
    """The table the driver hands the readers (equity_sim.cpp fill_table): a fixed pattern, win and tie uint32 [1326, 1326]."""
    if not _pf_table:
        i = np.arange(HOLDINGS * HOLDINGS, dtype=np.uint64)
        win = (((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(11)).astype(np.uint32)
        tie = (((i * np.uint64(40503) + np.uint64(7)) & np.uint64(0xFFFFFFFF)) & np.uint64(1023)).astype(np.uint32)
        _pf_table.append((win.reshape(HOLDINGS, HOLDINGS), tie.reshape(HOLDINGS, HOLDINGS)))
    return _pf_table[0]


def pf_hero_expect(hero, w, per_spot):
    win, tie = preflop_table()
    m = len(hero)
    out = dict(agg=np.zeros((m, 3), np.uint64), win=np.zeros((m, HOLDINGS), np.uint32), tie=np.zeros((m, HOLDINGS), np.uint32),
               boards=np.zeros(m, np.uint32), status=np.zeros(m, np.uint8))
    for i in range(m):
        r = PS.hero_equity(win, tie, hero[i], None if w is None else (w[i] if per_spot else w))
        for k in out:
            out[k][i] = r[k]
    return out


def pf_hero_case(name, m, seed, grid, wform=None, outputs=None, quick=False, edit=None):
    rng = np.random.default_rng(seed)
    hero = np.array([[card(c) for c in rng.permutation(52)[:2]] for _ in range(m)], np.uint8)
    if edit:
        edit(hero)
    w, per_spot = weights_for(seed + 1, m, wform)
    arrays = {"m": ("u32", [m]), "grid": ("u32", [grid]), "hero": ("u8", hero), "weights": ("u16", w), "per_spot": ("u32", [per_spot])}
    return Case(name, "pfhero", arrays, lambda: pf_hero_expect(hero, w, per_spot), outputs, quick)


def preflop_reader_cases():
    """k_pfm_prep + k_pfm_hero (family pfhero) and k_pfm_rvr (family pfrvr) on the fixed table."""
    cs = []

    def ends(hero):
        hero[0], hero[1] = [card(0), card(1)], [card(51), card(50)]      # holdings 0 and 1325

    def bits(hero):
        hero[1] = [0x4A, 0x01]                                        # suit 4: no card
        hero[2] = [0x05, 0xFF]
        hero[4] = [0x21, 0x21]                                        # the same card twice
    # ONE workgroup takes every spot in turn: the sums of the spot before are read before the next one's are written
    cs.append(pf_hero_case("pfhero-grid1-five-spots", 5, 71, 1, "shared", quick=True, edit=ends))
    cs.append(pf_hero_case("pfhero-spot-weights-grid2", 5, 72, 2, "spot", quick=True))
    cs.append(pf_hero_case("pfhero-no-weights-refused-between", 6, 73, 4, None, quick=True, edit=bits))
    cs.append(pf_hero_case("pfhero-zero-weights", 2, 74, 2, "zero"))
    cs.append(pf_hero_case("pfhero-status-alone", 6, 73, 4, None, outputs=("status",), quick=True, edit=bits))
    for o in OUTPUTS["pfhero"]:
        cs.append(pf_hero_case("pfhero-no-" + o, 3, 75, 1, "shared", outputs=[x for x in OUTPUTS["pfhero"] if x != o]))
    for observer, who in ((1, lambda w: np.full(w["T"], 1)), (-2, lambda w: w["active"])):
        w = table_world(76, 3, 6)                                     # tables at every turn: the board is not read
        arrays = dict(table_arrays(w), m=("u32", [len(w["tables"])]), grid=("u32", [2]), observer=("i32", [observer]))

        def expect(w=w, who=who):
            seat = np.asarray(who(w), np.int64)
            rows = np.arange(w["T"])
            hero = np.stack([w["deck"][rows, 5 + 2 * seat], w["deck"][rows, 6 + 2 * seat]], axis=1)
            return table_expect(w, pf_hero_expect(hero, None, 0), ("agg", "win", "tie"), "boards")
        cs.append(Case("pfhero-table-form-observer%d" % observer, "pfhero", arrays, expect, quick=(observer == -2)))
    for name, m, wform, quick in (("pfrvr-two-rows", 2, "spot", True), ("pfrvr-no-weights", 1, None, False)):
        w, _ = weights_for(77, m, wform)
        arrays = {"m": ("u32", [m]), "weights": ("u16", w)}

        def expect(w=w, m=m):
            win, tie = preflop_table()
            rw, rt, tot = PS.rvr(win, tie, np.ones((m, HOLDINGS), np.uint16) if w is None else w)
            return {"win": rw, "tie": rt, "tot": tot}
        cs.append(Case(name, "pfrvr", arrays, expect, quick=quick))
    return cs


# ---------------------------------------------------------------------------------------------------------------- river solver
def river_case(name, pools, tree, iters, seed, grid=1, outputs=None, quick=True, edit=None, redit=None):
    """k_rs_prep + k_river_solve against tests/river_solver_spec.py; int64 value / br are compared as their bit patterns."""
    board, _, dead = board_spots(seed, [(5, p) for p in pools])
    m = len(pools)
    rng = np.random.default_rng(seed + 1)
    ranges = rng.integers(0, 65536, (m, 2, HOLDINGS)).astype(np.uint16)
    for row in ranges.reshape(-1, HOLDINGS):
        row[rng.integers(0, HOLDINGS, 200)] = 0
        row[rng.integers(0, HOLDINGS, 100)] = 65535
    if edit:
        edit(board, dead)
    if redit:
        redit(ranges)
    arrays = {"m": ("u32", [m]), "grid": ("u32", [grid]), "iters": ("u32", [iters]), "n": ("u32", [tree.n]), "pot": ("u32", [tree.pot]),
              "kind": ("u8", tree.kind), "child": ("u8", tree.child), "put": ("u32", tree.put), "board": ("u8", board), "dead": ("u64", dead),
              "ranges": ("u16", ranges)}

    def expect():
        r = RVS.solve_batch(board, ranges, tree, iters, dead)
        return dict(strategy=r["strategy"], value=r["value"].view(np.uint64), br=r["br"].view(np.uint64), status=r["status"])
    return Case(name, "riversolve", arrays, expect, outputs, quick)


def river_cases():
    """Every case at a grid of 1: one workgroup takes the spots in turn, so stale LDS or work space of the spot before would show."""
    from pokerl_amd.solver import RiverTree, river_tree
    small, default = river_tree(100, 50), river_tree(100, 400)
    FF = 0xFF
    forced = RiverTree([0, 1, 4], [[1, FF, FF, FF], [2, FF, FF, FF], [FF] * 4], [[0, 0]] * 3, 77)
    four = RiverTree([0, 4, 1, 1, 1, 3, 4, 3, 4, 3, 4], [[1, 2, 3, 4], [FF] * 4, [5, 6, FF, FF], [7, 8, FF, FF], [9, 10, FF, FF]] + [[FF] * 4] * 6,
                     [[0, 0], [0, 0], [50, 0], [100, 0], [200, 0], [50, 0], [50, 50], [100, 0], [100, 100], [200, 0], [200, 200]], 100)

    def royal_board(board, dead):                                     # ten to ace of one suit, the rest of that suit dead: the board plays
        board[:] = np.array([8, 9, 10, 11, 12], np.uint8)             # for everyone, every pair of holdings ties
        for i in range(len(dead)):
            d = (int(dead[i]) & ~sum(1 << (r * 4) for r in range(8, 13))) | sum(1 << (r * 4) for r in range(8))
            dead[i] = np.uint64(d)

    def break_middle_board(board, dead):
        board[1, 1] = board[1, 0]

    def zero_one(ranges):
        ranges[0, 1] = 0
        ranges[1, 0] = 0
    cs = [river_case("rsolve-pools-grid1", (4, 9, 33, 46), small, 2, 31),
          river_case("rsolve-default-tree-iters1", (9, 12), default, 1, 32),
          river_case("rsolve-default-tree-iters3", (6, 17), default, 3, 33),
          river_case("rsolve-forced-and-four", (5, 24), forced, 2, 34),
          river_case("rsolve-four-actions", (11, 32), four, 2, 35),
          river_case("rsolve-refused-between", (12, 9, 11), small, 2, 36, edit=break_middle_board),
          river_case("rsolve-all-ties", (10, 14), small, 3, 37, edit=royal_board),
          river_case("rsolve-one-range-zero", (12, 16), default, 2, 38, redit=zero_one),
          river_case("rsolve-grid2-status-only", (9, 9, 9), small, 1, 39, grid=2, outputs=("status",), edit=break_middle_board),
          river_case("rsolve-no-strategy", (7, 8), small, 2, 40, outputs=("value", "br", "status"))]
    assert len({c.name for c in cs}) == len(cs)
    return cs


# ---------------------------------------------------------------------------------------------------------------- turn solver
def turn_case(name, pools, tree, iters, seed, outputs=None, quick=True, edit=None, redit=None, fixture=None):
    """k_ts_prep + k_turn_solve against tests/turn_solver_spec.py at a grid of 1; int64 value / br are compared as their bit patterns.
    fixture: the spot and the expected values come from tests/golden/turn_solver/<fixture>.npz (written by the spec: make.py there)."""
    m = len(pools)
    if fixture:
        fx = np.load(os.path.join(ROOT, "tests", "golden", "turn_solver", fixture + ".npz"))
        board, dead, ranges = fx["board"][None].copy(), np.array([fx["dead"]], np.uint64), fx["ranges"][None].copy()
    else:
        board, _, dead = board_spots(seed, [(4, p) for p in pools])
        board = np.ascontiguousarray(board[:, :4])
        rng = np.random.default_rng(seed + 1)
        ranges = rng.integers(0, 65536, (m, 2, HOLDINGS)).astype(np.uint16)
        for row in ranges.reshape(-1, HOLDINGS):
            row[rng.integers(0, HOLDINGS, 200)] = 0
            row[rng.integers(0, HOLDINGS, 100)] = 65535
    if edit:
        edit(board, dead)
    if redit:
        redit(ranges)
    arrays = {"m": ("u32", [m]), "grid": ("u32", [1]), "iters": ("u32", [iters]), "n": ("u32", [tree.n]), "pot": ("u32", [tree.pot]),
              "kind": ("u8", tree.kind), "child": ("u8", tree.child), "put": ("u32", tree.put), "board": ("u8", board), "dead": ("u64", dead),
              "ranges": ("u16", ranges)}

    def expect():
        if fixture:
            return dict(strategy=fx["strategy"][None], value=fx["value"][None].view(np.uint64), br=fx["br"][None].view(np.uint64), status=fx["status"][None])
        r = TSS.solve_batch(board, ranges, tree, iters, dead)
        return dict(strategy=r["strategy"], river_strategy=r["river_strategy"], value=r["value"].view(np.uint64), br=r["br"].view(np.uint64), status=r["status"])
    return Case(name, "turnsolve", arrays, expect, outputs, quick)


def turn_feature_tree():
    """A hand-made tree with a four-action root, a forced node, turn-level folds, river-level folds and an all-in chance -> showdown."""
    from pokerl_amd.solver import TurnTree
    FF = 0xFF
    nodes = [(0, [1, 2, 3, 4], (0, 0)), (1, [5], (0, 0)), (1, [6, 7], (50, 0)), (1, [8, 9], (300, 0)), (1, [10, 11], (100, 0)),
             (5, [12], (0, 0)), (3, [], (50, 0)), (5, [13], (50, 50)), (3, [], (300, 0)), (5, [14], (300, 300)), (3, [], (100, 0)), (5, [15], (100, 100)),
             (0, [16, 17], (0, 0)), (4, [], (50, 50)), (4, [], (300, 300)), (0, [18, 19], (100, 100)), (4, [], (0, 0)), (1, [20, 21], (100, 0)),
             (1, [22, 23, 24], (200, 100)), (4, [], (100, 100)), (3, [], (100, 0)), (4, [], (100, 100)), (3, [], (200, 100)), (4, [], (200, 200)),
             (0, [25, 26], (200, 300)), (2, [], (200, 300)), (4, [], (300, 300))]
    return TurnTree([k for k, _, _ in nodes], [ch + [FF] * (4 - len(ch)) for _, ch, _ in nodes], [list(p) for _, _, p in nodes], 100)


def turn_cases():
    """The turn solver's cases (names tsolve-...), every one at a grid of 1: one workgroup takes the spots in turn, so stale LDS or work
    space of the spot before would show.  NOT part of all_cases()."""
    from pokerl_amd.solver import turn_tree
    small, feature = turn_tree(100, 50, (0.5,), 1), turn_feature_tree()

    def straight_flush_board(board, dead):                            # four of the river solver's royal_board, the rest of that suit dead:
        board[:] = np.array([8, 9, 10, 11], np.uint8)                  # the fifth on the river makes the board play for everyone
        for i in range(len(dead)):
            dead[i] = np.uint64((int(dead[i]) & ~sum(1 << (r * 4) for r in range(8, 13))) | sum(1 << (r * 4) for r in range(8)))

    def break_middle_board(board, dead):
        board[1, 1] = board[1, 0]

    def zero_one(ranges):
        ranges[0, 1] = 0
        ranges[1, 0] = 0
    cs = [turn_case("tsolve-pools-grid1", (5, 9, 20, 33), small, 2, 51),
          turn_case("tsolve-feature-tree-iters1", (8, 12), feature, 1, 52),
          turn_case("tsolve-feature-tree-iters3", (6, 10), feature, 3, 53),
          turn_case("tsolve-refused-between", (9, 8, 7), small, 2, 54, edit=break_middle_board),
          turn_case("tsolve-board-plays", (14, 16), small, 2, 55, edit=straight_flush_board),
          turn_case("tsolve-one-range-zero", (10, 12), feature, 2, 56, redit=zero_one),
          turn_case("tsolve-no-strategy", (7, 8), small, 2, 57, outputs=("value", "br", "status")),
          turn_case("tsolve-status-only", (9, 9, 9), small, 1, 58, outputs=("status",), edit=break_middle_board),
          turn_case("tsolve-p48-fixture", (48,), turn_tree(100, 400, (1.0,), 1), 2, 59, outputs=("strategy", "value", "br", "status"), quick=False, fixture="p48")]
    assert len({c.name for c in cs}) == len(cs)
    return cs


# ---------------------------------------------------------------------------------------------------------------- a tree per spot
def tree_rows(trees, rows):
    """The trees as the tree-per-spot calls take them: tree k is row k of every array, `rows` nodes a row"""
    K = len(trees)
    kind, child, put = np.zeros((K, rows), np.uint8), np.full((K, rows, 4), 0xFF, np.uint8), np.zeros((K, rows, 2), np.uint32)
    for k, t in enumerate(trees):
        kind[k, :t.n], child[k, :t.n], put[k, :t.n] = t.kind, t.child, t.put
    return {"ntrees": ("u32", [K]), "n": ("u32", [t.n for t in trees]), "pot": ("u32", [t.pot for t in trees]), "kind": ("u8", kind),
            "child": ("u8", child), "put": ("u32", put)}


def trees_case(name, street, pools, trees, tree_of, iters, seed, outputs=None, quick=True, edit=None):
    """k_rs_prep / k_ts_prep + k_trees_prep + k_trees_river_solve / k_trees_turn_solve at a grid of 1 against the spec run ONE SPOT AT A
    TIME with that spot's tree (tests/solver_trees_util.py); street: 5 (river) or 4 (turn) board cards."""
    m = len(pools)
    board, _, dead = board_spots(seed, [(street, p) for p in pools])
    board = np.ascontiguousarray(board[:, :street])
    rng = np.random.default_rng(seed + 1)
    ranges = rng.integers(0, 65536, (m, 2, HOLDINGS)).astype(np.uint16)
    for row in ranges.reshape(-1, HOLDINGS):
        row[rng.integers(0, HOLDINGS, 200)] = 0
        row[rng.integers(0, HOLDINGS, 100)] = 65535
    if edit:
        edit(board, dead)
    tree_of = np.asarray(tree_of, np.uint32)
    assert tree_of.shape == (m,)
    arrays = {"m": ("u32", [m]), "grid": ("u32", [1]), "iters": ("u32", [iters]), **tree_rows(trees, 64 if street == 5 else 128),
              "tree_of": ("u32", tree_of), "board": ("u8", board), "dead": ("u64", dead), "ranges": ("u16", ranges)}

    def expect():
        r = (STU.river_expect if street == 5 else STU.turn_expect)(board, ranges, trees, tree_of, iters, dead)
        return {k: (r[k].view(np.uint64) if k in ("value", "br") else r[k]) for k in OUTPUTS["rivertrees" if street == 5 else "turntrees"]}
    return Case(name, "rivertrees" if street == 5 else "turntrees", arrays, expect, outputs, quick)


def break_second_board(board, dead):
    board[1, 1] = board[1, 0]


def river_trees_cases():
    """The river solver with a tree per spot (names rtrees-...), every case at a grid of 1: ONE workgroup takes the spots in turn, so a stale
    tree, stale regrets or stale LDS of the spot before would show.  NOT part of all_cases()."""
    from pokerl_amd.solver import river_tree
    forced, four, chain = STU.forced_river_tree(), STU.four_action_river_tree(), STU.chain_river_tree()
    small, default = river_tree(100, 50), river_tree(100, 400)
    cs = [trees_case("rtrees-big-after-small-and-back", 5, (9, 7, 12, 6, 10, 8), [forced, default, four, chain], [0, 1, 0, 3, 2, 1], 2, 71),
          trees_case("rtrees-refused-and-bad-tree-between", 5, (9, 8, 10, 7, 9, 6), [small, default], [1, 0, 2, 0, 0xFFFFFFFF, 1], 2, 72, edit=break_second_board),
          trees_case("rtrees-one-tree-repeated", 5, (6, 17, 9), [small], [0, 0, 0], 3, 73),
          trees_case("rtrees-unreferenced-tree-sets-the-stride", 5, (8, 11), [forced, chain, four], [0, 2], 2, 74),
          trees_case("rtrees-pools-fall-trees-grow", 5, (33, 12, 5), [forced, small, default], [0, 1, 2], 1, 75),
          trees_case("rtrees-no-strategy", 5, (7, 8), [default, forced], [0, 1], 2, 76, outputs=("value", "br", "status")),
          trees_case("rtrees-status-only", 5, (9, 9, 9), [small, forced], [0, 1, 5], 1, 77, outputs=("status",), edit=break_second_board)]
    assert len({c.name for c in cs}) == len(cs)
    return cs


def turn_trees_cases():
    """The turn solver with a tree per spot (names ttrees-...), every case at a grid of 1.  NOT part of all_cases()."""
    from pokerl_amd.solver import turn_tree
    allin, small, wide = STU.allin_turn_tree(), turn_tree(30, 20, (1.0,), 1), turn_tree(100, 400, (1.0,), 1)
    cs = [trees_case("ttrees-big-after-small-and-back", 4, (7, 6, 8, 6, 9), [allin, wide, small], [0, 1, 0, 2, 1], 2, 81),
          trees_case("ttrees-refused-and-bad-tree-between", 4, (8, 7, 9, 6, 7, 6), [small, allin], [1, 0, 2, 0, 0xFFFFFFFF, 1], 2, 82, edit=break_second_board),
          trees_case("ttrees-one-tree-repeated", 4, (6, 10, 7), [small], [0, 0, 0], 2, 83),
          trees_case("ttrees-unreferenced-tree-sets-the-strides", 4, (7, 8), [allin, wide], [0, 0], 1, 84),
          trees_case("ttrees-no-river-strategy", 4, (9, 7), [wide, allin], [0, 1], 2, 85, outputs=("strategy", "value", "br", "status")),
          trees_case("ttrees-status-only", 4, (9, 9, 9), [small, allin], [0, 1, 7], 1, 86, outputs=("status",), edit=break_second_board)]
    assert len({c.name for c in cs}) == len(cs)
    return cs


# ---------------------------------------------------------------------------------------------------------------- locked nodes
def lock_arrays(seed, trees, tree_of, patterns, river=False):
    """(lock uint8 [m, Dmax], locked uint16 [m, Dmax, (52,) 4, 1326]) for one level of a call.  patterns[i]: "none", "all", "p1" (the rows
    player 1 acts at), "zero" (every row locked to all-zero weights: the uniform row), "ffff" (a refused spot: every flag set, every weight
    0xFFFF) or a list of rows.  The weights are random with zeros among them.  What the definition says is NOT READ is 0xFFFF wherever this
    function knows it: rows past the spot's own D (their flags set), rows whose flag is 0, and action slots from nact on."""
    rng = np.random.default_rng(seed)
    m = len(patterns)
    rows_of = lambda t: (t.river_decision_nodes if river else t.decision_nodes)
    Dmax = max(len(rows_of(t)) for t in trees)
    mid = (52,) if river else ()
    lock = np.zeros((m, Dmax), np.uint8)
    locked = rng.integers(0, 65536, (m, Dmax) + mid + (4, HOLDINGS)).astype(np.uint16)
    locked[rng.random(locked.shape) < 0.1] = 0
    for i, pat in enumerate(patterns):
        k = int(tree_of[i]) if tree_of is not None else 0
        if pat == "ffff" or k >= len(trees):
            lock[i], locked[i] = 0xFF, 0xFFFF
            continue
        t = trees[k]
        nodes = rows_of(t)
        D = len(nodes)
        if pat == "none":
            rows = []
        elif pat in ("all", "zero"):
            rows = list(range(D))
        elif pat == "p1":
            rows = [r for r, v in enumerate(nodes) if int(t.kind[v]) == 1]
        else:
            rows = [r for r in pat if r < D]
        lock[i, rows] = 1
        if pat == "zero":
            locked[i, :D] = 0
        lock[i, D:], locked[i, D:] = 1, 0xFFFF
        for r, v in enumerate(nodes):
            if not lock[i, r]:
                locked[i, r] = 0xFFFF
            locked[i, r, ..., t.num_actions(v):, :] = 0xFFFF
    return lock, locked


def lock_case(name, street, pools, trees, tree_of, iters, seed, patterns, river_patterns=None, outputs=None, quick=True, edit=None, no_lock=False, fixture=None):
    """k_rs_prep / k_ts_prep (+ k_trees_prep where tree_of is given) + k_lock_river_solve / k_lock_turn_solve at a grid of 1 against
    tests/solver_lock_spec.py; street: 5 (river) or 4 (turn) board cards.  tree_of None: one tree, no tree_of array.  no_lock: the lock
    arrays are left out of the call (nothing is locked).  fixture: the expected outputs come from tests/golden/solver_lock/<fixture>.npz
    (written by the spec alone: make.py there, which also holds the recipe of the inputs)."""
    m = len(pools)
    if fixture:
        import importlib.util
        mk = importlib.util.spec_from_file_location("solver_lock_make", os.path.join(ROOT, "tests", "golden", "solver_lock", "make.py"))
        LOCKFX = importlib.util.module_from_spec(mk)
        mk.loader.exec_module(LOCKFX)
        x = LOCKFX.inputs(fixture)
        board, dead, ranges, trees, tree_of = x["board"], x["dead"], x["ranges"], [x["tree"]], None
        lock, locked, rlock, rlocked = x["lock"], x["locked"], x["river_lock"], x["river_locked"]
        iters = x["iters"]
    else:
        board, _, dead = board_spots(seed, [(street, p) for p in pools])
        board = np.ascontiguousarray(board[:, :street])
        rng = np.random.default_rng(seed + 1)
        ranges = rng.integers(0, 65536, (m, 2, HOLDINGS)).astype(np.uint16)
        for row in ranges.reshape(-1, HOLDINGS):
            row[rng.integers(0, HOLDINGS, 200)] = 0
            row[rng.integers(0, HOLDINGS, 100)] = 65535
        if edit:
            edit(board, dead)
        lock, locked = lock_arrays(seed + 2, trees, tree_of, patterns)
        rlock, rlocked = lock_arrays(seed + 3, trees, tree_of, river_patterns or patterns, river=True) if street == 4 else (None, None)
    if tree_of is not None:
        tree_of = np.asarray(tree_of, np.uint32)
        assert tree_of.shape == (m,)
    arrays = {"m": ("u32", [m]), "grid": ("u32", [1]), "iters": ("u32", [iters]), **tree_rows(trees, 64 if street == 5 else 128),
              "tree_of": ("u32", tree_of), "board": ("u8", board), "dead": ("u64", dead), "ranges": ("u16", ranges)}
    if not no_lock:
        arrays.update({"lock": ("u8", lock), "locked": ("u16", locked)})
        if street == 4:
            arrays.update({"river_lock": ("u8", rlock), "river_locked": ("u16", rlocked)})
    family = "riverlock" if street == 5 else "turnlock"

    def expect():
        of = np.zeros(m, np.uint32) if tree_of is None else tree_of
        if fixture:
            fx = np.load(os.path.join(ROOT, "tests", "golden", "solver_lock", fixture + ".npz"))
            return dict(strategy=fx["strategy"][None], value=fx["value"][None].view(np.uint64), br=fx["br"][None].view(np.uint64), status=fx["status"][None])
        if street == 5:
            r = SLS.solve_river_batch(board, ranges, trees, of, iters, None if no_lock else lock, locked, dead)
        else:
            r = SLS.solve_turn_batch(board, ranges, trees, of, iters, None if no_lock else lock, locked, None if no_lock else rlock, rlocked, dead)
        return {k: (r[k].view(np.uint64) if k in ("value", "br") else r[k]) for k in OUTPUTS[family]}
    return Case(name, family, arrays, expect, outputs, quick)


def river_lock_cases():
    """The river solver with locked nodes (names rlock-...), every case at a grid of 1: ONE workgroup takes the spots in turn, so a stale
    sigma or stale flags of the spot before would show.  NOT part of all_cases()."""
    from pokerl_amd.solver import river_tree
    forced, four, chain = STU.forced_river_tree(), STU.four_action_river_tree(), STU.chain_river_tree()
    small, default = river_tree(100, 50), river_tree(100, 400)
    cs = [lock_case("rlock-free-all-p1-all-free", 5, (9, 7, 12, 6, 10), [default], None, 2, 91, ["none", "all", "p1", "all", "none"]),
          lock_case("rlock-refused-with-ffff-between", 5, (9, 8, 10, 7, 9), [small, four], [1, 0, 2, 0, 1], 2, 92, ["p1", "ffff", "ffff", "all", "none"],
                    edit=break_second_board),
          lock_case("rlock-all-zero-rows-are-uniform", 5, (8, 11), [four], None, 2, 93, ["zero", [0]]),
          lock_case("rlock-iters0", 5, (10, 6, 9), [default, four], [0, 1, 0], 0, 94, ["all", "p1", "none"]),
          lock_case("rlock-pools-4-9-33", 5, (4, 9, 33), [small], [0, 0, 0], 2, 95, ["p1", [1, 2], "all"]),
          lock_case("rlock-large-after-small-locks-past-its-rows", 5, (8, 7, 9, 6), [forced, chain, small], [0, 1, 2, 1], 1, 96, [[0, 1, 5, 20], [3, 20, 31], "none", "all"]),
          lock_case("rlock-lock-null", 5, (7, 9), [default], None, 2, 97, ["all", "all"], no_lock=True),
          lock_case("rlock-status-only", 5, (9, 9, 9), [small, forced], [0, 1, 5], 1, 98, ["all", "ffff", "all"], outputs=("status",), edit=break_second_board)]
    assert len({c.name for c in cs}) == len(cs)
    return cs


def turn_lock_cases():
    """The turn solver with locked nodes (names tlock-...), every case at a grid of 1: stale packed regret words of the spot before would
    show too.  NOT part of all_cases()."""
    from pokerl_amd.solver import turn_tree
    allin, small = STU.allin_turn_tree(), turn_tree(30, 20, (1.0,), 1)
    cs = [lock_case("tlock-free-all-p1-all-free", 4, (7, 6, 8, 6, 7), [small], None, 2, 101, ["none", "all", "p1", "all", "none"]),
          lock_case("tlock-refused-with-ffff-between", 4, (8, 7, 9, 6, 7), [small, allin], [1, 0, 2, 0, 1], 2, 102, ["p1", "ffff", "ffff", "all", "none"],
                    edit=break_second_board),
          lock_case("tlock-all-zero-rows-are-uniform", 4, (7, 8), [small], None, 2, 103, ["zero", [0]], ["zero", [1]]),
          lock_case("tlock-iters0", 4, (8, 6, 7), [small, allin], [0, 1, 0], 0, 104, ["all", "p1", "none"]),
          lock_case("tlock-pools-5-9-20", 4, (5, 9, 20), [small], [0, 0, 0], 2, 105, ["p1", [1], "all"], ["none", [0, 2], "p1"]),
          lock_case("tlock-large-after-small-locks-past-its-rows", 4, (7, 6, 8), [allin, small], [0, 1, 0], 1, 106, [[0, 3], [1, 3], "none"], [[1, 3], [0, 3], "all"]),
          lock_case("tlock-turn-level-only-and-river-level-only", 4, (7, 8), [small], None, 2, 107, ["all", "none"], ["none", "all"]),
          lock_case("tlock-lock-null", 4, (7, 6), [small], None, 2, 108, ["all", "all"], no_lock=True),
          lock_case("tlock-p48-fixture", 4, (48,), None, None, None, 109, None, outputs=("strategy", "value", "br", "status"), quick=False, fixture="turn_p48")]
    assert len({c.name for c in cs}) == len(cs)
    return cs


# ---------------------------------------------------------------------------------------------------------------- re-solving
def resolve_reach(seed, board, street, dead, limit, over=(), refused=()):
    """reach uint32 [m, 2, 1326]: random up to `limit` with zeros among them; the spots in `over` also hold entries ABOVE the limit (the
    kernel takes the minimum); what the definition says is not read -- invalid holdings, every entry of a spot in `refused` -- is
    0xFFFFFFFF."""
    rng = np.random.default_rng(seed)
    m = board.shape[0]
    reach = rng.integers(0, limit + 1, (m, 2, HOLDINGS)).astype(np.uint32)
    reach[rng.random(reach.shape) < 0.15] = 0
    reach[rng.random(reach.shape) < 0.05] = limit
    for i in range(m):
        if i in over:
            pick = rng.random((2, HOLDINGS))
            reach[i][pick < 0.1] = limit + 1
            reach[i][pick > 0.9] = 0xFFFFFFFF
        status, gone = VS.check_spot([int(x) for x in board[i]], street, int(dead[i]))
        if i in refused:
            reach[i] = 0xFFFFFFFF
        elif not status & ~VS.PREFLOP:
            reach[i][:, [h for h in range(HOLDINGS) if VS.PAIR_A[h] in gone or VS.PAIR_B[h] in gone]] = 0xFFFFFFFF
    return reach


def resolve_given(seed, trees, tree_of, m, beyond=()):
    """given int64 [m, 2, 1326]: random within +- 2^40; the spots in `beyond` also hold values past the clamp, the extremes of int64 among
    them; a spot whose tree has no given node (or no tree): all ones, which the kernel never reads."""
    rng = np.random.default_rng(seed)
    given = rng.integers(-(1 << 40), 1 << 40, (m, 2, HOLDINGS)).astype(np.int64)
    for i in range(m):
        k = int(tree_of[i]) if tree_of is not None else 0
        if k >= len(trees) or RZS.GIVEN not in [int(x) for x in trees[k].kind]:
            given[i] = -1
        elif i in beyond:
            pick = rng.random((2, HOLDINGS))
            given[i][pick < 0.05] = (1 << 45)
            given[i][(pick >= 0.05) & (pick < 0.1)] = -(1 << 45)
            given[i][pick > 0.97] = np.iinfo(np.int64).max
            given[i][(pick > 0.94) & (pick <= 0.97)] = np.iinfo(np.int64).min
    return given


def resolve_case(name, street, pools, trees, tree_of, iters, seed, at=None, at_card=None, patterns=None, use_reach=True, use_ranges=False, over=(),
                 beyond=(), refused=None, outputs=None, quick=True, edit=None, fixture=None):
    """k_rs_prep / k_ts_prep (+ k_trees_prep) + k_resolve_prep + k_resolve_river_solve / k_resolve_turn_solve at a grid of 1 against
    tests/resolve_spec.py.  at: per spot a node index, "root", "last", "leaf" (the tree's first terminal) or None for the whole call;
    at_card (turn): per spot a card code, "first" / "last" (the pool's first / last card), "board" (a board card: no card of the pool) or 0xFF.  refused: {spot: True} for the spots
    whose reach holds 0xFFFFFFFF throughout (refused by their board, their tree_of, their at or their at_card).  fixture: the expected
    outputs come from tests/golden/resolve/<fixture>.npz (written by the spec alone: make.py there)."""
    m = len(pools)
    family = "riverresolve" if street == 5 else "turnresolve"
    if fixture:
        import importlib.util
        mk = importlib.util.spec_from_file_location("resolve_make", os.path.join(ROOT, "tests", "golden", "resolve", "make.py"))
        FX = importlib.util.module_from_spec(mk)
        mk.loader.exec_module(FX)
        x = FX.inputs(fixture)
        arrays = {"m": ("u32", [1]), "grid": ("u32", [1]), "iters": ("u32", [x["iters"]]), **tree_rows([x["tree"]], 64 if street == 5 else 128),
                  "board": ("u8", x["board"]), "dead": ("u64", x["dead"]), "reach": ("u32", x["reach"]), "at": ("u8", x["at"])}
        if street == 4:
            arrays["at_card"] = ("u8", x["at_card"])

        def expect_fx():
            fx = np.load(os.path.join(ROOT, "tests", "golden", "resolve", fixture + ".npz"))
            return {k: (fx[k][None].view(np.uint64) if fx[k].dtype == np.int64 else fx[k][None]) for k in OUTPUTS[family] if k in fx}
        return Case(name, family, arrays, expect_fx, outputs, quick)
    board, _, dead = board_spots(seed, [(street, p) for p in pools])
    board = np.ascontiguousarray(board[:, :street])
    rng = np.random.default_rng(seed + 1)
    ranges = rng.integers(0, 65536, (m, 2, HOLDINGS)).astype(np.uint16)
    if edit:
        edit(board, dead)
    if tree_of is not None:
        tree_of = np.asarray(tree_of, np.uint32)
    tree_at = lambda i: trees[min(int(tree_of[i]) if tree_of is not None else 0, len(trees) - 1)]
    ats = None
    if at is not None:
        ats = np.zeros(m, np.uint8)
        for i, a in enumerate(at):
            t = tree_at(i)
            ats[i] = {"root": 0, "last": t.n - 1, "leaf": next(v for v in range(t.n) if t.kind[v] > 1 and t.kind[v] != 5)}.get(a, a)
    cards = None
    if at_card is not None:
        cards = np.zeros(m, np.uint8)
        for i, c in enumerate(at_card):
            _, gone = VS.check_spot([int(x) for x in board[i]], street, int(dead[i]))
            pool = [k for k in range(52) if k not in gone]
            cards[i] = {"first": int(VS.CANON[pool[0]]), "last": int(VS.CANON[pool[-1]]), "board": int(board[i, 0])}.get(c, c)
    limit = RZS.RIVER_LIM if street == 5 else RZS.TURN_LIM
    reach = resolve_reach(seed + 4, board, street, dead, limit, over, refused or {}) if use_reach else None
    has_given = street == 5 and any(RZS.GIVEN in [int(x) for x in t.kind] for t in trees)
    given = resolve_given(seed + 5, trees, tree_of, m, beyond) if has_given else None
    lock = locked = rlock = rlocked = None
    if patterns is not None:
        lock, locked = lock_arrays(seed + 2, trees, tree_of, patterns)
        if street == 4:
            rlock, rlocked = lock_arrays(seed + 3, trees, tree_of, patterns, river=True)
    arrays = {"m": ("u32", [m]), "grid": ("u32", [1]), "iters": ("u32", [iters]), **tree_rows(trees, 64 if street == 5 else 128),
              "tree_of": ("u32", tree_of), "board": ("u8", board), "dead": ("u64", dead),
              "ranges": ("u16", ranges if use_ranges or not use_reach else None), "reach": ("u32", reach),
              "given": ("u64", None if given is None else given.view(np.uint64)), "at": ("u8", ats), "at_card": ("u8", cards),
              "lock": ("u8", lock), "locked": ("u16", locked), "river_lock": ("u8", rlock), "river_locked": ("u16", rlocked)}
    if outputs is None and ats is None:
        outputs = tuple(k for k in OUTPUTS[family] if not k.startswith("node_"))

    def expect():
        if street == 5:
            r = RZS.solve_river_batch(board, ranges, trees, tree_of, iters, lock, locked, dead, reach, given, ats)
        else:
            r = RZS.solve_turn_batch(board, ranges, trees, tree_of, iters, lock, locked, rlock, rlocked, dead, reach, ats, cards)
        return {k: (r[k].view(np.uint64) if r[k].dtype == np.int64 else r[k]) for k in OUTPUTS[family]}
    return Case(name, family, arrays, expect, outputs, quick)


def gadget_of(tree, opponent):
    from pokerl_amd.solver import gadget_tree
    return gadget_tree(tree, opponent)


def river_resolve_cases():
    """The river solver's re-solving call (names rres-...), every case at a grid of 1: ONE workgroup takes the spots in turn, so stale node
    outputs, stale given values or stale LDS of the spot before would show.  NOT part of all_cases()."""
    from pokerl_amd.solver import river_tree
    forced, four, chain = STU.forced_river_tree(), STU.four_action_river_tree(), STU.chain_river_tree()
    small, default = river_tree(100, 50), river_tree(100, 400)
    gsmall, gfour = gadget_of(small, 1), gadget_of(four, 0)
    cs = [resolve_case("rres-at-after-no-given-and-back", 5, (9, 7, 10, 6, 8), [small, gsmall, gfour], [0, 1, 0, 2, 0], 2, 111, at=[3, 2, "root", 1, "last"], beyond=(1,)),
          resolve_case("rres-refused-bad-at-between", 5, (9, 8, 10, 7, 9, 8), [small, gfour], [1, 0, 2, 0, 0, 1], 2, 112, at=[0, 1, 0, 200, small.n, 4],
                       refused={1: True, 2: True, 3: True, 4: True}, edit=break_second_board),
          resolve_case("rres-at-root-leaf-last", 5, (8, 11, 7), [default], None, 2, 113, at=["root", "leaf", "last"]),
          resolve_case("rres-reach-above-the-limit", 5, (9, 6), [small], None, 2, 114, at=[1, 0], over=(0, 1)),
          resolve_case("rres-given-beyond-the-clamp", 5, (8, 10), [gsmall], None, 3, 115, at=[1, 0], beyond=(0, 1)),
          resolve_case("rres-large-after-small", 5, (8, 7, 9, 6), [forced, chain, gsmall], [0, 1, 2, 1], 1, 116, at=["last", "last", 1, 5]),
          resolve_case("rres-iters0-all-locked", 5, (10, 6, 9), [default, gfour], [0, 1, 0], 0, 117, at=[2, "last", "leaf"], patterns=["all", "p1", "none"]),
          resolve_case("rres-pools-4-9-33", 5, (4, 9, 33), [gsmall], [0, 0, 0], 2, 118, at=[2, 3, "last"]),
          resolve_case("rres-ranges-no-reach-no-at", 5, (7, 9), [gsmall], None, 2, 119, use_reach=False),
          resolve_case("rres-ranges-beside-reach-are-not-read", 5, (7, 9), [small], None, 2, 120, at=[0, 2], use_ranges=True),
          resolve_case("rres-status-only", 5, (9, 9, 9), [small, forced], [0, 1, 5], 1, 121, refused={1: True, 2: True}, outputs=("status",), edit=break_second_board)]
    assert len({c.name for c in cs}) == len(cs)
    return cs


def turn_resolve_cases():
    """The turn solver's re-solving call (names tres-...), every case at a grid of 1.  NOT part of all_cases()."""
    from pokerl_amd.solver import turn_tree
    allin, small = STU.allin_turn_tree(), turn_tree(30, 20, (1.0,), 1)
    rnode = small.river_decision_nodes[0]
    chance = next(v for v in range(small.n) if small.kind[v] == 5)
    cs = [resolve_case("tres-river-at-first-and-last-card", 4, (7, 6, 8, 7), [small], None, 2, 131, at=[rnode, rnode, chance, "last"],
                       at_card=["first", "last", 0xFF, "last"]),
          resolve_case("tres-refused-bad-at-bad-card-between", 4, (8, 7, 9, 6, 7, 6, 7), [small, allin], [1, 0, 2, 0, 0, 0, 1], 2, 132,
                       at=[0, 1, 0, 200, rnode, rnode, "last"], at_card=[0xFF, 0, 0, 0, 0x3F, "board", "first"],
                       refused={1: True, 2: True, 3: True, 4: True, 5: True}, edit=break_second_board),
          resolve_case("tres-at-root-leaf-last", 4, (7, 8, 6), [small], None, 2, 133, at=["root", "leaf", "last"], at_card=[0xFF, 0xFF, "first"]),
          resolve_case("tres-reach-above-the-limit", 4, (7, 6), [small], None, 2, 134, at=[1, rnode], at_card=[0xFF, "last"], over=(0, 1)),
          resolve_case("tres-large-after-small", 4, (7, 6, 8), [allin, small], [0, 1, 0], 1, 135, at=["last", "last", "root"], at_card=["first", "first", 0xFF]),
          resolve_case("tres-iters0-all-locked", 4, (8, 6), [small], None, 0, 136, at=[rnode + 1, chance], at_card=["last", 0xFF], patterns=["all", "p1"]),
          resolve_case("tres-pools-5-9-20", 4, (5, 9, 20), [small], [0, 0, 0], 2, 137, at=[rnode, chance, "last"], at_card=["first", 0xFF, "last"]),
          resolve_case("tres-ranges-no-reach-no-at", 4, (7, 6), [small], None, 2, 138, use_reach=False),
          resolve_case("tres-p48-fixture", 4, (48,), None, None, None, 139, quick=False, fixture="turn_p48",
                       outputs=("value", "br", "node_reach", "node_value", "node_br", "status"))]
    assert len({c.name for c in cs}) == len(cs)
    return cs


# ---------------------------------------------------------------------------------------------------------------- resuming
def resume_case(name, street, pools, trees, tree_of, iters, seed, t0, at=None, at_card=None, patterns=None, beyond=(), edit=None, quick=True):
    """k_rs_prep / k_ts_prep (+ k_trees_prep, k_resolve_prep) + k_resume_prep + k_resume_river_solve / k_resume_turn_solve at a grid of 1 against
    tests/resume_spec.py.  t0: per spot.  Every state array is pre-filled with the sentinel; a spot with t0 > 0 holds random regrets and
    accumulators at the entries the definition reads (the spots in `beyond`: values past both clamps, the extremes of int64 among them) and
    the sentinel everywhere else, so that an entry that must not be read, or must survive, shows."""
    m = len(pools)
    family = "riverresume" if street == 5 else "turnresume"
    board, _, dead = board_spots(seed, [(street, p) for p in pools])
    board = np.ascontiguousarray(board[:, :street])
    if edit:
        edit(board, dead)
    if tree_of is not None:
        tree_of = np.asarray(tree_of, np.uint32)
    tree_at = lambda i: trees[min(int(tree_of[i]) if tree_of is not None else 0, len(trees) - 1)]
    ats = None
    if at is not None:
        ats = np.array([{"root": 0, "last": tree_at(i).n - 1}.get(a, a) for i, a in enumerate(at)], np.uint8)
    cards = None
    if at_card is not None:
        cards = np.zeros(m, np.uint8)
        for i, c in enumerate(at_card):
            _, gone = VS.check_spot([int(x) for x in board[i]], street, int(dead[i]))
            pool = [k for k in range(52) if k not in gone]
            cards[i] = {"first": int(VS.CANON[pool[0]]), "last": int(VS.CANON[pool[-1]])}.get(c, c)
    reach = resolve_reach(seed + 4, board, street, dead, RZS.RIVER_LIM if street == 5 else RZS.TURN_LIM)
    has_given = street == 5 and any(RZS.GIVEN in [int(x) for x in t.kind] for t in trees)
    given = resolve_given(seed + 5, trees, tree_of, m) if has_given else None
    lock = locked = rlock = rlocked = None
    if patterns is not None:
        lock, locked = lock_arrays(seed + 2, trees, tree_of, patterns)
        if street == 4:
            rlock, rlocked = lock_arrays(seed + 3, trees, tree_of, patterns, river=True)
    t0 = np.asarray(t0, np.uint32)
    rng = np.random.default_rng(seed + 6)
    if street == 5:
        masks = [SMU.river_read_mask(board, dead, trees, tree_of, lock)] * 2
        lims = (RMS.RIVER_RMAX, RMS.RIVER_AMAX)
    else:
        tm, rm = SMU.turn_read_masks(board, dead, trees, tree_of, lock, rlock)
        masks, lims = [tm, tm, rm, rm], (RMS.TURN_RMAX, RMS.TURN_AMAX, RMS.TURN_RMAX, RMS.TURN_AMAX)
    big = np.iinfo(np.int64)
    state = []
    for j, mask in enumerate(masks):
        a = np.full(mask.shape, SMU.SENTINEL, np.int64)
        lim = lims[j % 2]
        for i in range(m):
            if not t0[i]:
                continue
            if i in beyond:
                vals = rng.choice(np.array([big.min, -1, 0, 4242, lim, lim + 1, big.max, lim // 2], np.int64), mask[i].shape)
            else:
                vals = rng.integers(0, 1 << (40 if j % 2 == 0 else 30), mask[i].shape).astype(np.int64)
                vals[rng.random(mask[i].shape) < 0.3] = 0
            a[i][mask[i]] = vals[mask[i]]
        state.append(a)
    names = RMS.STATE_KEYS if street == 5 else RMS.TURN_STATE_KEYS
    arrays = {"m": ("u32", [m]), "grid": ("u32", [1]), "iters": ("u32", [iters]), **tree_rows(trees, 64 if street == 5 else 128),
              "tree_of": ("u32", tree_of), "board": ("u8", board), "dead": ("u64", dead), "reach": ("u32", reach),
              "given": ("u64", None if given is None else given.view(np.uint64)), "at": ("u8", ats), "at_card": ("u8", cards),
              "lock": ("u8", lock), "locked": ("u16", locked), "river_lock": ("u8", rlock), "river_locked": ("u16", rlocked), "t0": ("u32", t0),
              **{k: ("u64", a.view(np.uint64)) for k, a in zip(names, state)}}
    outputs = tuple(k for k in OUTPUTS[family] if ats is not None or not k.startswith("node_"))

    def expect():
        if street == 5:
            r = RMS.solve_river_batch(board, None, trees, tree_of, iters, lock, locked, dead, reach, given, ats, t0, *state)
        else:
            r = RMS.solve_turn_batch(board, None, trees, tree_of, iters, lock, locked, rlock, rlocked, dead, reach, ats, cards, t0, *state)
        return {k: (r[k].view(np.uint64) if r[k].dtype == np.int64 else r[k]) for k in OUTPUTS[family]}
    return Case(name, family, arrays, expect, outputs, quick)


def break_board_one(board, dead):
    board[1, 1] = board[1, 0]


def river_resume_cases():
    """The river solver's resuming call (names rsum-...), every case at a grid of 1: ONE workgroup takes the spots in turn, so the state, the t0
    or stale R / A of the spot before would show.  NOT part of all_cases()."""
    from pokerl_amd.solver import river_tree
    forced, four, chain = STU.forced_river_tree(), STU.four_action_river_tree(), STU.chain_river_tree()
    small, default = river_tree(100, 50), river_tree(100, 400)
    gsmall = gadget_of(small, 1)
    cs = [resume_case("rsum-t0-after-zero-and-back", 5, (9, 7, 10, 6), [small, default], [0, 1, 0, 1], 2, 211, [0, 3, 0, 2], at=[1, "root", "last", 2]),
          resume_case("rsum-zero-after-t0", 5, (8, 9), [four], None, 3, 212, [5, 0]),
          resume_case("rsum-refused-bad-iter-dup-card-between", 5, (9, 8, 10, 7, 9, 8), [small, gsmall], [1, 0, 0, 2, 1, 0], 2, 213, [1, 3, 4095, 6, 0xFFFFFFFF, 4094],
                      at=[0, 1, 0, 0, 2, 3], edit=break_board_one),
          resume_case("rsum-locked-rows-keep-their-state", 5, (9, 7, 8), [small, four], [0, 1, 0], 2, 214, [2, 0, 0], patterns=["p1", "all", "p1"]),
          resume_case("rsum-iters0", 5, (7, 9), [gsmall], None, 0, 215, [0, 5]),
          resume_case("rsum-state-beyond-both-clamps", 5, (8, 10), [small], None, 3, 216, [7, 4000], beyond=(0, 1)),
          resume_case("rsum-large-after-small", 5, (8, 7, 9, 6), [forced, chain], [0, 1, 0, 1], 1, 217, [1, 1, 0, 0]),
          resume_case("rsum-pools-4-9-33", 5, (4, 9, 33), [small], [0, 0, 0], 2, 218, [1, 0, 2], at=[2, 3, "last"])]
    assert len({c.name for c in cs}) == len(cs)
    return cs


def turn_resume_cases():
    """The turn solver's resuming call (names tsum-...), every case at a grid of 1.  NOT part of all_cases()."""
    from pokerl_amd.solver import turn_tree
    allin, small = STU.allin_turn_tree(), turn_tree(30, 20, (1.0,), 1)
    cs = [resume_case("tsum-t0-after-zero-and-back", 4, (7, 6, 8), [allin], None, 2, 231, [0, 3, 0], at=[6, "root", "last"], at_card=["first", 0xFF, "last"]),
          resume_case("tsum-zero-after-t0", 4, (6, 7), [small], None, 2, 232, [2, 0]),
          resume_case("tsum-refused-bad-iter-dup-card-between", 4, (8, 7, 9, 6, 7), [allin], [0, 0, 0, 1, 0], 2, 233, [1, 3, 4095, 6, 4094], edit=break_board_one),
          resume_case("tsum-locked-rows-keep-their-state", 4, (7, 6, 8), [allin], None, 2, 234, [2, 0, 3], patterns=["p1", "all", [1]]),
          resume_case("tsum-iters0", 4, (7, 6), [allin], None, 0, 235, [0, 5]),
          resume_case("tsum-state-beyond-both-clamps", 4, (7, 8), [allin], None, 3, 236, [7, 4000], beyond=(0, 1)),
          resume_case("tsum-large-after-small", 4, (7, 6, 6), [allin, small], [0, 1, 0], 1, 237, [1, 1, 0]),
          resume_case("tsum-pools-5-9-20", 4, (5, 9, 20), [allin], [0, 0, 0], 2, 238, [1, 0, 2], at=[6, "root", "last"], at_card=["first", 0xFF, "last"])]
    assert len({c.name for c in cs}) == len(cs)
    return cs


# ---------------------------------------------------------------------------------------------------------------- the solvers' arithmetic
def arith_case(name, street, call, quick=True, fixture=None):
    """A call of tests/solver_rule_cases.py (rule_call: the operand tables through the rule; corner_call: the bounds corner) on the resuming
    kernels at a grid of 1, against tests/resume_spec.py -- and, for the tables, against rule_exact in Python integers, which the spec's
    result must meet before it is the expected value.  The state arrays hold the tables, the sentinel where nothing is read (rule_call) or the
    clamps everywhere (corner_call): not every case holds the sentinel, which is why these are not among river_resume_cases().
    fixture: an .npz of tests/golden/solver_arith (the spec's result at a pool where it takes minutes; digests for the large arrays)."""
    import solver_rule_cases as SRC      # here, not at the top: every other family's cases load without it
    family = "riverresume" if street == 5 else "turnresume"
    names = RMS.STATE_KEYS if street == 5 else RMS.TURN_STATE_KEYS
    m = len(call["board"])
    arrays = {"m": ("u32", [m]), "grid": ("u32", [1]), "iters": ("u32", [call["iters"]]), **tree_rows(call["trees"], 64 if street == 5 else 128),
              "tree_of": ("u32", call["tree_of"]), "board": ("u8", call["board"]), "dead": ("u64", call["dead"]), "ranges": ("u16", call["ranges"]),
              "t0": ("u32", call["t0"]), **{k: ("u64", a.view(np.uint64)) for k, a in zip(names, call["state"])}}
    outputs = tuple(k for k in OUTPUTS[family] if not k.startswith("node_"))

    def expect():
        if fixture is not None:
            fx = np.load(os.path.join(ROOT, "tests", "golden", "solver_arith", fixture))
            assert fx["board"].tolist() == call["board"][0].tolist() and int(fx["t0"]) == int(call["t0"][0]) and int(fx["iters"]) == call["iters"]
            out = {k: (fx[k][None].view(np.uint64) if fx[k].dtype == np.int64 else fx[k][None]) for k in ("strategy", "value", "br", "status")}
            out.update({k: str(fx["sha256_" + k]) for k in ("river_strategy",) + names})
            return out
        r = SRC.spec_of(street, call)
        assert not r["status"].any() and ("where" not in call or SRC.rule_wanted(call, r) == [])
        return {k: (r[k].view(np.uint64) if r[k].dtype == np.int64 else r[k]) for k in outputs}
    return Case(name, family, arrays, expect, outputs, quick)


def river_arith_cases():
    """The river solver's arithmetic (names rarith-...; family riverresume, grid 1): the A tables through `average` (iters = 0), the R tables
    through `regret` (iters = 1, root reach ONE) at t0 = 1 and 4095, and the bounds corner at the full pool from three states at the clamps.
    NOT part of all_cases()."""
    import solver_rule_cases as SRC
    from pokerl_amd.solver import river_tree
    forced, four, nine, default = STU.forced_river_tree(), STU.four_action_river_tree(), SRC.nine_node_tree(), river_tree(100, 400)
    cs = [arith_case("rarith-rule-average", 5, SRC.rule_call(5, [forced, default, four], "average", 7, 47)),
          arith_case("rarith-rule-regret-t1", 5, SRC.rule_call(5, [forced, nine, default, four], "regret", 1, 47)),
          arith_case("rarith-rule-regret-t4095", 5, SRC.rule_call(5, [forced, nine, default, four], "regret", 4095, 47))]
    cs += [arith_case("rarith-corner-" + v, 5, SRC.corner_call(5, 47, v)) for v in ("top", "swing", "mix")]
    return cs


def turn_arith_cases():
    """The turn solver's arithmetic (names tarith-...; family turnresume, grid 1): the tables at both levels at P = 9, the bounds corner at
    P = 12 and, from tests/golden/solver_arith/turn_corner_p48.npz, at the full pool (not quick).  The tables are cut to two (A) and three (R) spots
    a tree (the root row has 36 holdings at this pool and a workgroup takes ten seconds a spot here; the river cases carry them whole).
    NOT part of all_cases()."""
    import solver_rule_cases as SRC
    from pokerl_amd.solver import turn_tree
    four, small = SRC.four_action_turn_tree(), turn_tree(30, 20, (1.0,), 1)
    return [arith_case("tarith-rule-average", 4, SRC.rule_call(4, [four], "average", 9, 9, spots=2)),
            arith_case("tarith-rule-regret-t4095", 4, SRC.rule_call(4, [small], "regret", 4095, 9, spots=3), quick=False),
            arith_case("tarith-rule-regret-four-t1", 4, SRC.rule_call(4, [four], "regret", 1, 9, spots=3), quick=False),
            arith_case("tarith-corner-top-p12", 4, SRC.corner_call(4, 12, "top")),
            arith_case("tarith-corner-swing-p12", 4, SRC.corner_call(4, 12, "swing"), quick=False),
            arith_case("tarith-corner-p48-fixture", 4, SRC.corner_call(4, 48, "top"), quick=False, fixture="turn_corner_p48.npz")]

# ---------------------------------------------------------------------------------------------------------------- pre-flop solver
def pfsolve_case(name, trees, tree_of, iters, seed, m=None, outputs=None, quick=True, redit=None):
    """k_preflop_solve at a grid of 1 against tests/preflop_solver_spec.py on the driver's fixed-pattern table (preflop_table());
    tree_of None: the driver gets none, every spot uses tree 0.  int64 value / br are compared as their bit patterns."""
    m = len(tree_of) if tree_of is not None else m
    rng = np.random.default_rng(seed)
    ranges = rng.integers(0, 65536, (m, 2, HOLDINGS)).astype(np.uint16)
    for row in ranges.reshape(-1, HOLDINGS):
        row[rng.integers(0, HOLDINGS, 200)] = 0
        row[rng.integers(0, HOLDINGS, 100)] = 65535
    if redit:
        redit(ranges)
    arrays = {"m": ("u32", [m]), "grid": ("u32", [1]), "iters": ("u32", [iters]), **tree_rows(trees, 64), "ranges": ("u16", ranges)}
    if tree_of is not None:
        tree_of = np.asarray(tree_of, np.uint32)
        arrays["tree_of"] = ("u32", tree_of)

    def expect():
        r = PFS.solve_batch(preflop_table(), ranges, trees, iters, tree_of)
        return {k: (r[k].view(np.uint64) if k in ("value", "br") else r[k]) for k in OUTPUTS["pfsolve"]}
    return Case(name, "pfsolve", arrays, expect, outputs, quick)


def pfsolve_cases():
    """The pre-flop solver's cases (names pfsolve-...), every one at a grid of 1: ONE workgroup takes the spots in turn, so a stale tree,
    stale regrets or stale LDS of the spot before would show.  NOT part of all_cases()."""
    from pokerl_amd.solver import RiverTree, preflop_tree, push_fold_tree
    FF = 0xFF
    big = preflop_tree(40, 1, 2, 0, (0.75, 2.0), 3)
    assert big.n == 64
    three = RiverTree([0, 1, 4], [[1, FF, FF, FF], [2, FF, FF, FF], [FF] * 4], [[1, 2], [2, 2], [2, 2]], 3)
    pf, pf_ante, limp = push_fold_tree(20), push_fold_tree(9, 1, 2, 1), preflop_tree(12, 1, 2, 0, (1.0,), 2)

    def empty(ranges):
        ranges[0, 1] = 0
        ranges[1, 0] = 0

    def single(ranges):
        ranges[0, 0] = 0
        ranges[0, 0, 1325] = 40000
        ranges[1, 1] = 0
        ranges[1, 1, 0] = 65535
    cs = [pfsolve_case("pfsolve-pushfold-after-64-before-3", [big, pf, three], [0, 1, 2, 1], 2, 91),
          pfsolve_case("pfsolve-bad-tree-between", [pf, limp], [1, 2, 0, 0xFFFFFFFF, 1], 2, 92),
          pfsolve_case("pfsolve-empty-range", [pf_ante], None, 2, 93, m=2, redit=empty),
          pfsolve_case("pfsolve-one-holding", [limp], None, 3, 94, m=2, redit=single),
          pfsolve_case("pfsolve-iters1", [pf, three], [1, 0, 0], 1, 95),
          pfsolve_case("pfsolve-iters3-limp", [limp, pf_ante], [0, 1], 3, 96),
          pfsolve_case("pfsolve-no-strategy", [limp, three], [0, 1], 2, 97, outputs=("value", "br", "status")),
          pfsolve_case("pfsolve-strategy-alone", [pf], None, 2, 98, m=1, outputs=("strategy", "status")),
          pfsolve_case("pfsolve-status-only", [pf, three], [0, 7, 1], 1, 99, outputs=("status",))]
    assert len({c.name for c in cs}) == len(cs)
    return cs


def all_cases():
    cs = rvr_hist_cases() + range_cases() + equity_cases() + sampled_cases()
    assert len({c.name for c in cs}) == len(cs)
    return cs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--exe", action="append", help="the driver; given several times, every case runs on each build")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--keep")
    a = ap.parse_args()
    cases = [c for c in all_cases() + ranged_cases() + ev_cases() + ranged_ev_cases() + cluster_cases() + hero_hist_cases() + preflop_cases() + river_cases() + turn_cases() + river_trees_cases() + turn_trees_cases() + river_lock_cases() + turn_lock_cases() + river_resolve_cases() + turn_resolve_cases() + river_resume_cases() + turn_resume_cases() + river_arith_cases() + turn_arith_cases() + pfsolve_cases() if (c.quick or not a.quick) and a.only in c.name]
    if a.list:
        for c in cases:
            print("%-34s %-8s %s" % (c.name, c.family, "quick" if c.quick else ""))
        return 0
    if not a.exe:
        ap.error("--exe")
    work = a.keep or tempfile.mkdtemp(prefix="equity_sim_")
    os.makedirs(work, exist_ok=True)
    failed, total = 0, [0.0] * len(a.exe)
    for c in cases:
        for k, exe in enumerate(a.exe):
            bad, sec, log = run_case(exe, c, work)
            total[k] += sec
            stats = [ln for ln in log.splitlines() if ln.startswith("equity_sim:")]
            print("%-34s %-18s %s  %7.2f s  %s" % (c.name, os.path.basename(exe), "FAILED" if bad else "== spec", sec, stats[-1].split(" done: ")[-1] if stats and not bad else ""))
            if bad:
                failed += 1
                for b in bad:
                    print("    " + b)
                print("    " + "\n    ".join(log.splitlines()[-30:]))
            sys.stdout.flush()
    print("%d cases x %d builds, %d failed; in the driver: %s" % (len(cases), len(a.exe), failed, ", ".join("%s %.1f s" % (os.path.basename(e), t) for e, t in zip(a.exe, total))))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
