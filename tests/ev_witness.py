"""The game itself as a witness of the showdown EV (TEST INFRASTRUCTURE): tables are driven to late streets by the never-fold caller of
oracle/rng_spec.py on ladder stacks, the tables that stand at the start of the river's betting round are picked, their EV is recorded, and
the hand is played out by seats that check -- with no bet outstanding that adds no money; a CALL would: the reference's call of a zero
high bet still puts chips in -- so the payoffs end_hand pays must equal the recorded ev bit for bit.  Works on any backend of tests/golden_util.py's interface (the C oracle on the CPU, the HIP product)."""
import numpy as np

from oracle import rng_spec as R

import equity_spec as ES

CHECK, CALL, ALL_IN = 1, 2, 6
# (tables, seats) -> (seed, steps of the never-fold caller): chosen on the CPU oracle so that river tables with a side pot exist
WITNESS = {(64, 6): (5, 17), (200, 3): (31, 8)}


def ladder_stacks(n):
    return [20.0 * (p + 1) + 0.5 * (p % 2) for p in range(n)]


def deep_steps(b, steps):
    b.reset()
    for _ in range(steps):
        b.step(b.pick_actions(R.POLICY_DEEP))
    return b.snapshot()


def spots_of(snap):
    """The table form's spots from a snapshot: holes, board, nboard, live, bets (= bets + pending_bets)."""
    n = snap["states"].shape[1]
    holes, board, nboard, live = ES.table_spots(snap["cards"][:, :5 + 2 * n], snap["states"], snap["turn"])
    return holes, board, nboard, live, snap["bets"] + snap["pending"]


def live_levels(live, bets):
    """Per table: (number of live seats, number of distinct bets among them)."""
    out = []
    for lv, b in zip(live, bets):
        seats = [p for p in range(len(b)) if (int(lv) >> p) & 1]
        out.append((len(seats), len({float(b[p]) for p in seats})))
    return out


def river_candidates(snap):
    """Tables at the start of the river's betting round (no bet outstanding) with at least two live seats."""
    holes, board, nboard, live, bets = spots_of(snap)
    ll = live_levels(live, bets)
    return [t for t in range(len(live)) if snap["turn"][t] == 3 and not snap["pending"][t].any() and ll[t][0] >= 2]


def passive_actions(valid):
    """CHECK where it is valid, else CALL, else ALL_IN: valid uint8 [T] action masks."""
    v = np.asarray(valid).astype(np.int64)
    return np.where((v >> CHECK) & 1, CHECK, np.where((v >> CALL) & 1, CALL, ALL_IN)).astype(np.int32)


def play_out_passively(b, tables, max_steps=64):
    """Steps every table with passive_actions until each of `tables` has ended its hand; -> {table: payoffs at the end of that hand}."""
    paid, todo = {}, set(tables)
    for _ in range(max_steps):
        if not todo:
            break
        flags, _ = b.step(passive_actions(b.snapshot()["valid"]))
        ended = [t for t in todo if (int(flags[t]) >> 1) & 1]
        if ended:
            pay = b.snapshot()["payoffs"]
            for t in ended:
                paid[t] = pay[t].copy()
                todo.discard(t)
    assert not todo, sorted(todo)
    return paid
