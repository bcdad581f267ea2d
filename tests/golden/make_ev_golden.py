#!/usr/bin/env python3
"""Fixture generator of the showdown EV: runs the REAL reference's Game.end_hand (imported read-only from
/root/reference) once per completion of a spot's board and writes tests/golden/ev_ref.json.  Runs only in the build container -- nothing in
tests/, bench.py or the package reads the reference.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ev_golden.py

Per spot a Game is put into a FINAL state by hand (deck, player_states, bets; pending_bets 0), setup_hand is stubbed (end_hand calls it last,
game.py:539, and it would deal the next hand) and pokerl.game.np.argsort is the stable one, as tests/golden/make_golden.py pins it.  The
file holds data only: per spot the inputs, `boards`, and for a complete board the payoffs end_hand wrote, as hex floats; otherwise the mean
payoff per seat over the boards (in the definition's order: combinations of the pool in canonical order), as float of the exact
fractions.Fraction mean."""
import itertools
import json
import os
import sys
from fractions import Fraction

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

import pokerl.game as G  # noqa: E402
from pokerl.cards import Card  # noqa: E402
from pokerl.enums import PlayerState  # noqa: E402


class _StableArgsortNumpy:
    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def argsort(a, *args, **kwargs):
        kwargs.setdefault("kind", "stable")
        return np.argsort(a, *args, **kwargs)


G.np = _StableArgsortNumpy()
CANON = [((c % 4) << 4) | (c // 4) for c in range(52)]
BETS = (0.0, 5.0, 10.0, 20.0, 37.0, 50.0)


def end_hand_payoffs(n, deck_values, states, bets):
    g = G.Game(num_players=n)
    g.setup_hand = lambda: None
    g.deck = [Card(int(v)) for v in deck_values]
    g.turn = 3
    g.player_states = np.array(states, np.uint8)
    g.bets = np.array(bets, np.float64)
    g.pending_bets = np.zeros(n)
    g.credits = np.full(n, 1000.0)
    g.end_hand()
    return [float(x) for x in g.payoffs]


def make_spot(n, holes, board, states, bets):
    """holes [n][2], board: the known cards; states: PlayerState per seat."""
    live = sum(1 << p for p, s in enumerate(states) if s in (PlayerState.CALLED, PlayerState.ALL_IN))
    dead = set(board) | {c for h in holes for c in h}
    pool = [c for c in CANON if c not in dead]
    k = 5 - len(board)
    total = [Fraction(0)] * n
    boards = 0
    last = None
    for combo in itertools.combinations(pool, k):
        deck = list(board) + list(combo) + [c for h in holes for c in h]
        last = end_hand_payoffs(n, deck, states, bets)
        total = [t + Fraction(x) for t, x in zip(total, last)]
        boards += 1
    spot = dict(n=n, holes=[list(map(int, h)) for h in holes], board=[int(c) for c in board], live=live, states=[int(s) for s in states],
                bets=[float(b) for b in bets], boards=boards)
    if k == 0:
        spot["payoffs"] = [x.hex() for x in last]
    else:
        spot["mean"] = [float(t / boards).hex() for t in total]
    return spot, boards


def random_spot(rng, n, nb):
    while True:
        cards = [CANON[c] for c in rng.permutation(52)]
        board = cards[:nb]
        holes = [cards[5 + 2 * p:7 + 2 * p] for p in range(n)]
        states = [int(rng.choice([PlayerState.CALLED, PlayerState.ALL_IN, PlayerState.ALL_IN, PlayerState.FOLDED, PlayerState.BROKEN])) for _ in range(n)]
        bets = [float(rng.choice(BETS)) for _ in range(n)]
        for p, s in enumerate(states):
            if s == PlayerState.BROKEN:
                bets[p] = 0.0
        if any(s in (PlayerState.CALLED, PlayerState.ALL_IN) for s in states):
            return holes, board, states, bets


def main():
    rng = np.random.default_rng(20240607)
    spots, calls = [], 0
    C, A, F = PlayerState.CALLED, PlayerState.ALL_IN, PlayerState.FOLDED
    # line 148: three live seats of one rank class (a pair of aces on the board plays for all), the lowest bettor first with the lowest
    # kicker -- taking its hand out changes who wins among the other two
    b148 = [0x00, 0x10, 0x06, 0x18, 0x22]                       # AS AH 7S 9H 3D
    h148 = [[0x09, 0x31], [0x1C, 0x34], [0x0B, 0x33]]           # T, K, Q kickers: W_0 = {2} (line 148), W_1 = {1}
    s, c = make_spot(3, h148, b148, [A, C, C], [10.0, 50.0, 50.0])
    spots.append(s); calls += c
    # a folded seat whose bet exceeds every live bet; the two top live bets equal under such dead money; one live seat; all bets zero
    hand = [[0x01, 0x12], [0x23, 0x34], [0x05, 0x16], [0x27, 0x38]]
    brd = [0x00, 0x1A, 0x2B, 0x3C, 0x09]
    for states, bets in (([C, A, F, C], [20.0, 10.0, 50.0, 20.0]), ([C, C, F, A], [37.0, 37.0, 50.0, 5.0]), ([F, C, F, F], [20.0, 10.0, 50.0, 5.0]),
                         ([C, C, A, C], [0.0, 0.0, 0.0, 0.0]), ([C, A, C, C], [0.0, 5.0, 20.0, 20.0])):
        s, c = make_spot(4, hand, brd, states, bets)
        spots.append(s); calls += c
    for n in range(2, 10):                                      # river: one end_hand call per spot
        for _ in range(5):
            s, c = make_spot(n, *random_spot(rng, n, 5))
            spots.append(s); calls += c
    for n in (2, 3, 4, 5, 6, 7, 8, 9, 3, 6, 9, 4):              # turn: one call per card of the pool
        s, c = make_spot(n, *random_spot(rng, n, 4))
        spots.append(s); calls += c
    for n in (3, 6, 9):                                         # flop: C(P, 2) calls
        s, c = make_spot(n, *random_spot(rng, n, 3))
        spots.append(s); calls += c
    out = dict(share_unit=720720, bets_from=list(BETS), end_hand_calls=calls, spots=spots)
    with open(os.path.join(HERE, "ev_ref.json"), "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
        f.write("\n")
    multi = sum(1 for s in spots if len({b for p, b in enumerate(s["bets"]) if (s["live"] >> p) & 1}) > 1)
    print("spots", len(spots), "end_hand calls", calls, "with more than one live bet level", multi)


if __name__ == "__main__":
    main()
