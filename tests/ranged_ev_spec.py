"""The ranged-showdown-EV definition restated in numpy (TEST INFRASTRUCTURE): include/pokerl_hip.h "Ranged showdown EV" / DESIGN.md section
3.11, on top of the two restatements it is made of -- equity_ranged_spec (check_spot, attempts: the accepted attempts and their cards) and
ev_spec (bad_bets, levels, level_winners, ev_formula) -- and oracle.loader.eval_hands.  Nothing in it comes from a kernel."""
import numpy as np

import equity_ranged_spec as WS
import equity_sampled_spec as SS
import equity_spec as ES
import ev_spec as EV
from oracle import loader as O

SHARE_UNIT = ES.SHARE_UNIT
BAD_BET = EV.BAD_BET
NO_LEVEL = EV.NO_LEVEL
UNIFORM = WS.UNIFORM
DEFAULT_SEED = WS.DEFAULT_SEED
OBSERVER_NONE, OBSERVER_ACTIVE = WS.OBSERVER_NONE, WS.OBSERVER_ACTIVE
INT_KEYS = ("status", "accepted", "level_seat", "share")
F64_KEYS = ("amount", "ev")
KEYS = INT_KEYS + F64_KEYS


def ev_formula(amount, share, accepted, bets):
    """ev_spec.ev_formula with boards := accepted; accepted == 0: the row is +0.0 (no estimate)."""
    if int(accepted) == 0:
        return np.zeros(len(bets), np.float64)
    return EV.ev_formula(amount, share, int(accepted), bets)


def attempt_rankings(hands, live):
    """rank uint8 [N, A], kick uint32 [N, A] of the accepted attempts' hands [A, N, 7] (a seat that is not live: (NONE, []))."""
    a, n = hands.shape[:2]
    rank = np.full((n, a), ES.NONE_RANK, np.uint8)
    kick = np.zeros((n, a), np.uint32)
    for p in range(n):
        if (live >> p) & 1:
            rank[p], kick[p], _ = O.eval_hands(np.ascontiguousarray(hands[:, p]))
    return rank, kick


def spot_ev(holes, board, nb, live, bets, samples, weights=None, range_of=None, seed=DEFAULT_SEED, nonce=0, ident=0, key=None):
    """One spot -> dict(share [N, N], level_seat [N], amount [N], ev [N], accepted, status)."""
    holes = np.asarray(holes, np.uint8)
    n = holes.shape[0]
    bets = np.asarray(bets, np.float64)
    zero = dict(share=np.zeros((n, n), np.uint64), level_seat=np.full(n, NO_LEVEL, np.uint8), amount=np.zeros(n, np.float64),
                ev=np.zeros(n, np.float64), accepted=0)
    status, _, lv, _ = WS.check_spot(holes, board, int(nb), live, range_of, len(WS.as_ranges(weights)))
    if EV.bad_bets(bets):
        status |= BAD_BET
    if status:
        return dict(zero, status=status)
    out = dict(zero, status=0)
    bets = np.where(bets == 0, 0.0, bets)                              # a -0.0 bet is a zero and is read as +0.0
    levels = EV.levels(bets, lv)
    hands, lv, took = WS.attempts(holes, board, int(nb), live, weights, range_of, key or WS.R.seed_key(seed), ident, nonce, samples)
    acc = len(took)
    out["accepted"] = acc
    rank = kick = None
    for i, (s, amount, remain, last) in enumerate(levels):
        out["level_seat"][i] = s
        out["amount"][i] = amount
        if last:
            out["share"][i][s] = SHARE_UNIT * acc
        elif amount > 0 and acc:
            if rank is None:
                rank, kick = attempt_rankings(hands, lv)
            win = EV.level_winners(rank, kick, remain)
            nw = np.zeros(acc, np.int64)
            for p in range(n):
                nw += (win >> np.uint32(p)) & 1
            for p in range(n):
                inw = ((win >> np.uint32(p)) & 1).astype(bool)
                out["share"][i][p] = int(np.sum(SHARE_UNIT // nw[inw]))
    out["ev"] = ev_formula(out["amount"], out["share"], acc, bets)
    return out


def batch_ev(holes, board, nboard, live, bets, samples, weights=None, range_of=None, per_spot=False, seed=DEFAULT_SEED, nonce=0, ids=None, key=None):
    """The batch form: holes [m, N, 2], board [m, 5], nboard [m], live [m], bets [m, N], range_of [N] (or [m, N] with per_spot), ids [m] or
    None (= i) -> dict of [m, N, N] / [m, N] / [m] arrays."""
    holes = np.asarray(holes, np.uint8)
    m, n = holes.shape[:2]
    out = dict(share=np.zeros((m, n, n), np.uint64), level_seat=np.zeros((m, n), np.uint8), amount=np.zeros((m, n), np.float64),
               ev=np.zeros((m, n), np.float64), accepted=np.zeros(m, np.uint32), status=np.zeros(m, np.uint8))
    for i in range(m):
        ro = None if range_of is None else (np.asarray(range_of)[i] if per_spot else np.asarray(range_of))
        r = spot_ev(holes[i], [int(x) for x in board[i]], int(nboard[i]), int(live[i]), np.asarray(bets)[i], samples, weights, ro, seed, nonce,
                    i if ids is None else int(ids[i]), key)
        for k in out:
            out[k][i] = r[k]
    return out


def table_spots(deck, player_states, turn, active, observer, bets, pending_bets):
    """The table form's spots from the getters: equity_sampled_spec.table_spots for a seat or OBSERVER_ACTIVE, and bets + pending_bets (one
    binary64 addition each) -> (holes, board, nboard, live, bets)."""
    assert observer != OBSERVER_NONE
    holes, board, nboard, live = SS.table_spots(deck, player_states, turn, active, observer)
    return holes, board, nboard, live, np.asarray(bets, np.float64) + np.asarray(pending_bets, np.float64)


def merged(a, b, bets):
    """Two results of the same spot(s) with different nonces: counts add, ev by the formula on the sums."""
    share = np.asarray(a["share"], np.uint64) + np.asarray(b["share"], np.uint64)
    acc = np.asarray(a["accepted"], np.uint64) + np.asarray(b["accepted"], np.uint64)
    out = dict(a, share=share, accepted=acc)
    if share.ndim == 2:
        out["ev"] = ev_formula(a["amount"], share, acc, bets)
    else:
        out["ev"] = np.array([ev_formula(a["amount"][i], share[i], acc[i], np.asarray(bets)[i]) for i in range(share.shape[0])], np.float64)
    return out


def bet_patterns(n, live, i):
    """Bets [n] of spot i, cycling through: equal, a full ladder 10 (p + 1), a ladder with ties and zeros, and dead money at folded seats."""
    kind = i % 4
    if kind == 0:
        return np.full(n, 25.0)
    if kind == 1:
        return 10.0 * (np.arange(n) + 1)
    if kind == 2:
        return np.array([(0.0, 15.0, 15.0, 40.0, 0.0, 7.5)[p % 6] for p in range(n)])
    b = 20.0 + 5.0 * (np.arange(n) % 3)
    for p in range(n):
        if not (int(live) >> p) & 1:
            b[p] = 3.0 + p                                            # folded: its money stays in the pot
    return b


def turn_spot():
    """Section 3.6's fixed turn spot: hero AS AD against one hidden hand on KS 7D 7C 2H -> (holes, board, nb, live)."""
    from pokerl_amd.cards import card_value as cv
    holes = np.array([[cv("AS"), cv("AD")], [ES.UNKNOWN, ES.UNKNOWN]], np.uint8)
    return holes, [cv("KS"), cv("7D"), cv("7C"), cv("2H"), 0], 4, 0b11


def turn_range():
    """The fixed range of section 3.6's convergence test: numpy's default_rng(20241), about 60 % zeros, weights 0 .. 49."""
    rng = np.random.default_rng(20241)
    w = rng.integers(0, 50, WS.HOLDINGS)
    w[rng.random(WS.HOLDINGS) < 0.6] = 0
    return w.astype(np.uint16)


THREE_BETS = (20.0, 10.0, 30.0)      # two compared levels (seat 1, then seat 0) and a last stand (seat 2)


def three_seat_spot():
    """The fixed river spot of the convergence tests: hero 9S 9D shown on KS 7D 7C 2H 4C, seats 1 and 2 hidden behind two 40-holding ranges
    (default_rng(311)) -> (holes, board, nb, live, weights [2, 1326], range_of)."""
    from pokerl_amd.cards import card_value as cv
    holes = np.array([[cv("9S"), cv("9D")], [ES.UNKNOWN] * 2, [ES.UNKNOWN] * 2], np.uint8)
    board = [cv("KS"), cv("7D"), cv("7C"), cv("2H"), cv("4C")]
    rng = np.random.default_rng(311)
    w = np.zeros((2, WS.HOLDINGS), np.uint16)
    for r in range(2):
        w[r, rng.choice(WS.HOLDINGS, 40, replace=False)] = rng.integers(1, 100, 40)
    return holes, board, 5, 0b111, w, np.array([UNIFORM, 0, 1], np.uint16)


def three_seat_exact(bets=THREE_BETS):
    """(mean [3], variance [3], pairs) of a seat's per-attempt PAYOUT at three_seat_spot(): the host enumeration of the <= 1 600 pairs of
    holdings disjoint from each other and from the dead cards, under weight w1 * w2 (the accepted joint law of section 3.6); a pair's payout
    is the sum over the levels of amount_i / |W_i| for the seats in W_i, by ev_spec's levels and level_winners."""
    holes, board, nb, live, w, _ = three_seat_spot()
    dead = set(holes[0].tolist()) | set(board)
    hands, weights = [], []
    for h1 in np.flatnonzero(w[0]):
        for h2 in np.flatnonzero(w[1]):
            c = [ES.CANON[WS.PAIR_A[h1]], ES.CANON[WS.PAIR_B[h1]], ES.CANON[WS.PAIR_A[h2]], ES.CANON[WS.PAIR_B[h2]]]
            if len(set(c)) == 4 and not set(c) & dead:
                hands.append([board + holes[0].tolist(), board + c[:2], board + c[2:]])
                weights.append(int(w[0, h1]) * int(w[1, h2]))
    hands, weights = np.array(hands, np.uint8), np.array(weights, np.float64)
    assert 0 < len(hands) <= 1600
    rank, kick = attempt_rankings(hands, live)
    pay = np.zeros((len(hands), 3), np.float64)
    for s, amount, remain, last in EV.levels(np.array(bets, np.float64), live):
        if last:
            pay[:, s] += amount
        elif amount > 0:
            win = EV.level_winners(rank, kick, remain)
            nw = sum(((win >> np.uint32(p)) & 1).astype(np.float64) for p in range(3))
            for p in range(3):
                pay[:, p] += np.where((win >> np.uint32(p)) & 1, amount / nw, 0.0)
    q = weights / weights.sum()
    mean = (q[:, None] * pay).sum(axis=0)
    var = (q[:, None] * (pay - mean) ** 2).sum(axis=0)
    return mean, var, len(hands)


def assert_same(got, want, what=""):
    """Every output against the spec: integers equal, floating point bit for bit."""
    for key in INT_KEYS:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape and np.array_equal(g.astype(np.uint64), w.astype(np.uint64)), (what, key, np.argwhere(g.astype(np.uint64) != w.astype(np.uint64))[:4].tolist())
    for key in F64_KEYS:
        g, w = np.ascontiguousarray(got[key], np.float64), np.ascontiguousarray(want[key], np.float64)
        assert g.shape == w.shape and np.array_equal(g.view(np.uint64), w.view(np.uint64)), (what, key, g, w)
