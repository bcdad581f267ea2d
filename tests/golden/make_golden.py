#!/usr/bin/env python3
"""Golden-vector generator: runs the REAL reference (imported read-only from
/root/reference) under the build's RNG spec and writes small fixtures next to
this script.  Runs only in the build container -- /root/reference does not
exist on the GPU box, and nothing in tests/, bench.py or the package reads it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden.py [--only NAME]

What is injected (reference untouched on disk):
  * pokerl.game.random  -> object whose .shuffle(deck) installs the Philox deck
    of oracle/rng_spec.py for (seed, table_id, hand_serial)     [game.py:1,424]
  * pokerl.game.eval_hand -> recording wrapper (captures showdown rankings)  [game.py:489]
  * agents -> oracle/rng_spec.pick_action(seed, table_id, step_serial, mask)
  * pokerl.game.np -> numpy with a STABLE np.argsort [game.py:495].  The side-pot order of seats with EQUAL bets is
    whatever np.argsort returns for ties, and that is platform-dependent: numpy 2.2.6 on this AVX-512 host uses
    x86-simd-sort (e.g. argsort([2,1,0,0,0,0,1]) = [3,2,5,4,6,1,0]), while the numpy the reference pins
    (requirements.txt:4, 1.18.4) insertion-sorts arrays shorter than 16 and is stable.  The tie order decides who
    collects a folded seat's surplus chips through the `num_potential_winners == 1` branch (game.py:500-505), so parity
    is pinned to the reference's pinned-numpy behaviour: ascending seat index among equal bets.
Everything else (Game, judger, cards, envs) is the reference's own code.
"""
import argparse
import hashlib
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

import pokerl.game as G  # noqa: E402
from pokerl.cards import Card  # noqa: E402
from pokerl.envs import PokerGameEnv  # noqa: E402
from pokerl.enums import PlayerState  # noqa: E402
from pokerl import judger as J  # noqa: E402

from oracle import rng_spec as R  # noqa: E402

SNAP_FIELDS = ("active", "turn", "dealer", "sb", "bb", "hand", "states", "credits", "bets",
               "pending", "payoffs", "min_raise", "cards", "srank", "skick", "valid",
               "hand_serial", "step_serial")


# --------------------------------------------------------------------------- injection
class _DeckInjector:
    def __init__(self):
        self.by_deck = {}

    def shuffle(self, deck):
        t = self.by_deck[id(deck)]
        perm = R.deck_permutation(t.seed, t.table_id, t.hand_serial)
        deck[:] = [t.canon[i] for i in perm]
        t.hand_serial += 1


_injector = _DeckInjector()
G.random = _injector


class _StableArgsortNumpy:
    """numpy as pokerl.game sees it: identical except that argsort's default kind is the stable one."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def argsort(a, *args, **kwargs):
        kwargs.setdefault("kind", "stable")
        return np.argsort(a, *args, **kwargs)


class _ReversedTieArgsortNumpy:
    """The opposite deterministic tie rule (ascending values, DESCENDING seat index among equal bets): used only to show
    that a TIE_SETS fixture really depends on the rule."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def argsort(a, *args, **kwargs):
        a = np.asarray(a)
        return len(a) - 1 - np.argsort(a[::-1], kind="stable")


_STABLE_NP = _StableArgsortNumpy()
G.np = _STABLE_NP

_eval_sink = []
_real_eval = G.eval_hand


def _recording_eval(hand):
    out = _real_eval(hand)
    _eval_sink.append(out)
    return out


G.eval_hand = _recording_eval


class Table:
    """One reference Game plus the per-table serials of the RNG spec."""

    def __init__(self, seed, table_id, n, game=None, serial_base=(0, 0), **cfg):
        self.seed, self.table_id, self.n = seed, table_id, n
        self.hand_serial, self.step_serial = serial_base  # RNG-spec serials (64-bit); non-zero = a resumed stream
        self.game = game if game is not None else G.Game(num_players=n, **cfg)
        self.canon = list(self.game.deck)
        _injector.by_deck[id(self.game.deck)] = self
        self.srank = np.full(n, 10, np.uint8)
        self.skick = np.zeros(n, np.uint32)
        real_step = self.game.step

        def counted_step(action):
            del _eval_sink[:]
            out = real_step(action)
            self.step_serial += 1  # only reached when the action was valid
            self._absorb_showdowns()
            return out

        self.game.step = counted_step
        # content counters (the deep sets' meta): showdowns at the river among three or more seats, hands that pay three or more amounts
        self.river_showdowns_3way, self.hands_paying_3_amounts, self._ending = 0, 0, None
        real_end, real_setup = self.game.end_hand, self.game.setup_hand

        def counted_end():
            g = self.game
            live = int(np.sum((g.player_states != PlayerState.BROKEN) & (g.player_states != PlayerState.FOLDED)))
            self.river_showdowns_3way += int(g.turn == 4 and live >= 3)      # (next_turn has counted the river's end, game.py:561-564)
            self._ending = g.bets + g.pending_bets                           # what every seat has put in, before game.py:457
            real_end()

        def counted_setup():
            if self._ending is not None:        # called by end_hand (game.py:539): payoffs are net of the seats' own bets (game.py:531)
                got = self.game.payoffs + self._ending
                self.hands_paying_3_amounts += int(len(set(got[got != 0].tolist())) >= 3)
                self._ending = None
            real_setup()

        self.game.end_hand, self.game.setup_hand = counted_end, counted_setup

    def _absorb_showdowns(self):
        # every showdown evaluates exactly num_players hands in seat order (game.py:488-489)
        assert len(_eval_sink) % self.n == 0
        if _eval_sink:
            last = _eval_sink[-self.n:]
            for p, (rank, kick) in enumerate(last):
                self.srank[p] = rank
                self.skick[p] = J.get_kickers_value(kick)
        del _eval_sink[:]

    def mask_bits(self):
        onehot, _ = self.game.get_valid_actions()
        return sum(1 << a for a in range(7) if onehot[a])

    def pick(self, policy):
        return R.pick_action(self.seed, self.table_id, self.step_serial, self.mask_bits(), policy)

    def snapshot(self):
        g = self.game
        ncards = 5 + 2 * self.n
        return dict(
            active=g.active_player, turn=g.turn, dealer=g.dealer_idx, sb=g.small_blind_idx,
            bb=g.big_blind_idx, hand=g.hand, states=g.player_states.copy(),
            credits=g.credits.copy(), bets=g.bets.copy(), pending=g.pending_bets.copy(),
            payoffs=g.payoffs.copy(), min_raise=float(g.minimum_raise_value),
            cards=np.array([c.value for c in g.deck[:ncards]], np.uint8),
            srank=self.srank.copy(), skick=self.skick.copy(), valid=self.mask_bits(),
            hand_serial=self.hand_serial, step_serial=self.step_serial)


_DT = dict(active=np.uint8, turn=np.uint8, dealer=np.uint8, sb=np.uint8, bb=np.uint8,
           hand=np.int32, states=np.uint8, credits=np.float64, bets=np.float64,
           pending=np.float64, payoffs=np.float64, min_raise=np.float64, cards=np.uint8,
           srank=np.uint8, skick=np.uint32, valid=np.uint8, hand_serial=np.uint64,
           step_serial=np.uint64)


def _stack(snaps, prefix):
    return {prefix + k: np.array([s[k] for s in snaps], dtype=_DT[k]) for k in SNAP_FIELDS}


def snap_digest(snaps_by_table):
    """sha256 over one lockstep snapshot of all tables (fixed field order, C order)."""
    h = hashlib.sha256()
    for k in SNAP_FIELDS:
        h.update(np.ascontiguousarray(np.array([s[k] for s in snaps_by_table], dtype=_DT[k])).tobytes())
    return h.hexdigest()


# --------------------------------------------------------------------------- StateView records (f4)
def _hex(a):
    return [float(x).hex() for x in np.asarray(a, np.float64).ravel()]


def _state_tuple(sv):
    """StateView.__getstate__() (game.py:208-223) as JSON-able data; floats as hex strings (bit-exact)."""
    st = sv.__getstate__()
    return dict(player=int(st[0]), valid_actions=_hex(st[1]), num_players=int(st[2]), turn=int(st[3]),
                player_cards=[int(c.value) for c in st[4]], community_cards=[int(c.value) for c in st[5]],
                credits=_hex(st[6]), bets=_hex(st[7]), pending_bets=_hex(st[8]), minimum_raise_value=float(st[9]).hex())


def view_record(game):
    """What the reference exposes about one table to ANY seat: active_state (game.py:323-332), StateView(game, p)
    for every p (game.py:117-131; p = 0 means the active player, `player or game.active_player`), get_valid_actions(p)
    (game.py:339-383; p = 0 IS seat 0 there), and the properties pot / high_bet / game_over (game.py:281-320)."""
    n = game.num_players
    return dict(active=_state_tuple(game.active_state),
                per_player=[_state_tuple(G.Game.StateView(game, p)) for p in range(n)],
                valid_for=[_hex(game.get_valid_actions(p)[0]) for p in range(n)],
                pot=float(game.pot).hex(), high_bet=float(game.high_bet).hex(), game_over=bool(game.game_over))


# --------------------------------------------------------------------------- Game trajectories
class _HandCapProbe:
    """The cap rule (docs/history.md section 2, "Steps that never return", rule (b)): a Game.step that rolls more than `cap` hands
    is ended by the product right after its (cap+1)-th setup_hand() with PK_TERR_HAND_CAP, although the reference -- on the
    configuration pinned here -- does return, thousands of hands later.  This probe wraps the reference game's setup_hand
    (called as self.setup_hand() by end_hand, game.py:539) and snapshots the table right after that call: what the product
    must hold when it stops."""

    def __init__(self, table, cap):
        self.t, self.cap, self.calls, self.mid = table, cap, 0, None
        real = table.game.setup_hand

        def counted():
            real()
            self.calls += 1
            if self.calls == self.cap + 1:
                t = self.t
                last = _eval_sink[-t.n:] if _eval_sink else []        # rankings of the last showdown so far (game.py:488-489)
                for p, (rank, kick) in enumerate(last):
                    t.srank[p] = rank
                    t.skick[p] = J.get_kickers_value(kick)
                self.mid = t.snapshot()
                self.mid["step_serial"] = t.step_serial + 1          # the product's step returns here (one completed step)
                self.mid_srank, self.mid_skick = t.srank.copy(), t.skick.copy()

        table.game.setup_hand = counted


def game_trajectory(n, policy, seed, tables, steps, table_id_base=0, cfg=None, full=True, digest_every=0,
                    auto_reset=True, dealer=0, serial_base=(0, 0), views=None, hand_cap=None, held=None):
    """auto_reset=False: finished games are NOT reset (the lone survivor keeps being stepped, which the
    reference allows); a survivor's FOLD then trips `assert num_potential_winners > 0` (game.py:473):
    recorded as err=2 with the partially mutated state, after which that table is reset."""
    cfg = cfg or dict(start_credits=100, big_blind=2, small_blind=1)
    ts = [Table(seed, table_id_base + i, n, serial_base=serial_base, **cfg) for i in range(tables)]
    for t in ts:
        t.game.reset(dealer=dealer)          # only the FIRST reset takes the dealer; auto-resets use the default (0)
    probes = [_HandCapProbe(t, hand_cap) for t in ts] if hand_cap else None
    max_hands_in_step = 0
    init = [t.snapshot() for t in ts]
    out = {}
    meta = dict(kind="game", n=n, policy=policy, seed=seed, tables=tables, steps=steps,
                table_id_base=table_id_base, cfg=cfg, auto_reset=auto_reset, dealer=dealer,
                serial_base=list(serial_base))
    actions = np.zeros((steps, tables), np.int8)
    flags = np.zeros((steps, tables), np.uint8)
    errs = np.zeros((steps, tables), np.uint8)
    post, resets, reset_idx, digests = [], [], [], []
    for s in range(steps):
        row = []
        if held is not None:     # a StateView HELD across the step: its arrays alias the game's (game.py:128-130), see ALIAS_SETS
            kept = [(t.game.active_state, t.hand_serial) for t in ts]
            made = [_state_tuple(v) for v, _ in kept]
        for i, t in enumerate(ts):
            a = t.pick(policy)
            actions[s, i] = a
            if probes:
                probes[i].calls, probes[i].mid = 0, None
            try:
                over, hand, turn = t.game.step(int(a))
                flags[s, i] = int(bool(over)) | int(bool(hand)) << 1 | int(bool(turn)) << 2
            except AssertionError:
                assert not auto_reset
                errs[s, i] = 2
            if probes and probes[i].mid is not None:
                # the reference returned after probes[i].calls hands; the pinned rule stops the step after hand_cap + 1 of them:
                # record the table as it was THERE and rewind the harness' deck stream to it (the reset below deals from there)
                max_hands_in_step = max(max_hands_in_step, probes[i].calls)
                errs[s, i], flags[s, i] = 4, 0
                t.hand_serial = int(probes[i].mid["hand_serial"])
                t.srank, t.skick = probes[i].mid_srank, probes[i].mid_skick
                row.append(probes[i].mid)
                continue
            row.append(t.snapshot())
        if views is not None:
            views.append([view_record(t.game) for t in ts])
        if held is not None:     # (before the auto-reset below)
            held.append([dict(at_creation=made[i], after_step=_state_tuple(kept[i][0]), setup_hands=int(t.hand_serial - kept[i][1]),
                              live=dict(credits=_hex(t.game.credits), bets=_hex(t.game.bets), pending_bets=_hex(t.game.pending_bets),
                                        sb=int(t.game.small_blind_idx), bb=int(t.game.big_blind_idx)))
                         for i, t in enumerate(ts)])
        if full:
            post.append(row)
        if digest_every and (s + 1) % digest_every == 0:
            digests.append(snap_digest(row))
        for i, t in enumerate(ts):  # auto-reset finished games, as bench/rollout do
            if (flags[s, i] & 1 and auto_reset) or errs[s, i]:
                t.game.reset()
                if full:
                    resets.append(t.snapshot())
                    reset_idx.append((s, i))
    out["actions"], out["flags"], out["errs"] = actions, flags, errs
    out.update(_stack(init, "init_"))
    if full:
        flat = [sn for row in post for sn in row]
        st = _stack(flat, "post_")
        for k, v in st.items():
            out[k] = v.reshape((steps, tables) + v.shape[1:])
        if resets:
            out.update(_stack(resets, "reset_"))
        out["reset_idx"] = np.array(reset_idx, np.int32).reshape(-1, 2)
    if digest_every:
        meta["digest_every"] = digest_every
        meta["digests"] = digests
    meta.update(_content(ts))
    if hand_cap:
        meta["hand_cap"] = hand_cap
        meta["reference_hands_in_its_longest_step"] = max_hands_in_step
    out["meta"] = np.array(json.dumps(meta))
    return out


def _content(ts):
    return dict(river_showdowns_3way=sum(t.river_showdowns_3way for t in ts), hands_paying_3_amounts=sum(t.hands_paying_3_amounts for t in ts))


# --------------------------------------------------------------------------- PokerGameEnv trajectories
def env_trajectory(n, policy, opp_policy, seed, tables, steps, table_id_base=0, cfg=None):
    """opp_policy: one rng_spec policy for every opponent, or a list with one per opponent seat (seat 1 first) -- the
    reference's own `agents` list (envs/game_env.py:13-18) then holds a different callable per seat."""
    cfg = cfg or dict(start_credits=100, big_blind=2, small_blind=1)
    per_seat = list(opp_policy) if isinstance(opp_policy, (list, tuple)) else [opp_policy] * (n - 1)
    assert len(per_seat) == n - 1
    envs, ts = [], []
    for i in range(tables):
        holder = {}

        def make_agent(pol, holder=holder):
            def agent(state):
                assert state.player == holder["t"].game.active_player
                return holder["t"].pick(pol)
            return agent

        env = PokerGameEnv([make_agent(pol) for pol in per_seat], num_players=n, **cfg)
        t = Table(seed, table_id_base + i, n, game=env.game)
        holder["t"] = t
        envs.append(env)
        ts.append(t)
    for env in envs:
        env.reset()
    init = [t.snapshot() for t in ts]
    actions = np.zeros((steps, tables), np.int8)
    reward = np.zeros((steps, tables), np.float64)
    done = np.zeros((steps, tables), np.uint8)
    hand = np.zeros((steps, tables), np.uint8)
    post, resets, reset_idx = [], [], []
    for s in range(steps):
        row = []
        for i, (env, t) in enumerate(zip(envs, ts)):
            a = t.pick(policy)
            _, r, d, h = env.step(int(a))
            actions[s, i], reward[s, i], done[s, i], hand[s, i] = a, r, bool(d), bool(h)
            row.append(t.snapshot())
        post.append(row)
        for i, (env, t) in enumerate(zip(envs, ts)):
            if done[s, i]:
                env.reset()
                resets.append(t.snapshot())
                reset_idx.append((s, i))
    out = dict(actions=actions, reward=reward, done=done, hand_over=hand)
    out.update(_stack(init, "init_"))
    flat = [sn for row in post for sn in row]
    for k, v in _stack(flat, "post_").items():
        out[k] = v.reshape((steps, tables) + v.shape[1:])
    if resets:
        out.update(_stack(resets, "reset_"))
    out["reset_idx"] = np.array(reset_idx, np.int32).reshape(-1, 2)
    meta = dict(kind="env", n=n, policy=policy, opp_policy=opp_policy, seed=seed, tables=tables,
                steps=steps, table_id_base=table_id_base, cfg=cfg)
    meta.update(_content(ts))
    out["meta"] = np.array(json.dumps(meta))
    return out


# --------------------------------------------------------------------------- judger vectors
# Inputs of the reference's own known-answer tests (tests/pokerl/test_judger.py:14-78 and
# :83-117), as data.  Expected outputs are produced by running the reference below.
KAT_EVAL = [
    "2C 3C 4C 5C 6C 7C 8C", "1D 2D 3D 4D 5D 6C 7C", "1D 2D 3D 4D 8D 6C 7C", "1D 3D 5H 7H 7S 9S JS",
    "1D 3D 5H 8H 7S 9S 1S", "1D 1C 5H 6H 6H TS TS", "KD QC JH TH 9H 9S 9D", "KD QC JH TH 9H 5S 9D",
    "KD QC JH TH 9H 5S 7D", "8D 9C 7H 6H 9H 5S 7D", "2H 3C 4H 5H 6H 7H 8D", "8D 8C 8H 5H 5S 5D 3D",
    "8D 8C 8H 5H 5S 4D 3D", "1D 1C 1H 5H 5S 5D 5C", "1D 1C 1H 1S KS KD KC", "2D 3D 4D 5D 7D 6C KC",
    "2D 3C 4D 5D 8D JC KC", "2D 2C 3D 3D JD JC KC", "2D 2C 3D 3D JD JC JC", "2D 2C 3D 3D 3D JC JC",
    "KC QC JC TC 9C AD 4D", "9D 8C 4D 5D 6D JD KC",
]
KAT_EVAL_EXPECT = [  # (HandRanking, kickers) asserted at test_judger.py:15-78
    (1, [7]), (1, [4]), (4, [13, 7, 3, 2, 1]), (8, [6, 13, 10, 8]), (8, [13, 8, 7, 6]), (7, [13, 9, 5]),
    (5, [12]), (5, [12]), (5, [12]), (5, [8]), (4, [6, 5, 4, 3, 1]), (3, [7, 4]), (3, [7, 4]),
    (2, [4, 13]), (2, [13, 12]), (4, [6, 4, 3, 2, 1]), (9, [12, 10, 7, 4, 3]), (7, [10, 2, 12]),
    (3, [10, 2]), (3, [2, 10]), (1, [12]), (4, [10, 8, 5, 4, 3]),
]
KAT_COMPARE = [
    (["1D 1C 1H 5H 6H 1S KS", "1D 1C 1H 5H 6H QS JS"], [1, 0]),
    (["1D 1C 1H 5H 6H 1S KS", "1D 1C 1H 5H 6H QH JH"], [1, 0]),
    (["1D 1C 1H 2H 3H 1S KS", "1D 1C 1H 2H 3H 4H 5H"], [0, 1]),
    (["1D 3C 5H 7H 9H KS JS", "1D 3C 5H 7H 9H QS TS"], [1, 0]),
    (["1D 3C 5H 7H 9H KS JS", "1D 3C 5H 7H 9H QS TS"], [1, 0]),
    (["1D 3C 5H 7H 9H KS JS", "1D 3C 5H 7H 9H 3S TS"], [0, 1]),
    (["1D 3C 5H 7H 9H 1S 9D", "1D 3C 5H 7H 9H 7S 7S", "1D 3C 5H 7H 9H 9S 9S"], [0, 0, 1]),
]
# Quirk hands of SURVEY.md Appendix A.1 (straight-flush reset, wheel if/elif, ...)
QUIRK_EVAL = [
    "KC QC JC TC 9C 2C 3D", "KC 9C 8C 7C 6C 5C 2D", "AC KC QC 5D 4D 3D 2D", "AS KC QC 5D 4D 3D 2D",
    "AD 5D 4D 3D 2D KC QC", "AC 2D 3H 4S 5C 6D 9H", "AC 2D 3H 4S 5C KD 9H", "7C 7D 7H 4S 4C 4D 2H",
    "7C 7D 9H 9S 4C 4D 2H", "7C 7D 9H 9S 4C 4D KH", "AC AD AH AS 2C 2D 2H", "2C 3C 4C 5C 7C 8C 9C",
]


def cards_from(s):
    return [Card(x) for x in s.split()]


def pack_eval(out):
    rank, kick = out
    return int(rank), int(J.get_kickers_value(kick)), len(kick)


def judger_vectors(seed=1234):
    rng = np.random.default_rng(seed)
    kat = []
    for s, exp in zip(KAT_EVAL, KAT_EVAL_EXPECT):
        out = J.eval_hand(cards_from(s))
        assert (out[0], list(out[1])) == (exp[0], exp[1]), (s, out, exp)
        kat.append(dict(cards=s, values=[c.value for c in cards_from(s)], rank=int(out[0]),
                        kickers=[int(k) for k in out[1]]))
    quirks = []
    for s in QUIRK_EVAL:
        out = J.eval_hand(cards_from(s))
        quirks.append(dict(cards=s, values=[c.value for c in cards_from(s)], rank=int(out[0]),
                           kickers=[int(k) for k in out[1]]))
    cmp_kat = []
    for hands, exp in KAT_COMPARE:
        out = J.compare_hands([cards_from(h) for h in hands])
        assert out[0] == exp
        cmp_kat.append(dict(hands=hands, values=[[c.value for c in cards_from(h)] for h in hands],
                            onehot=out[0], winners=out[1],
                            rankings=[[int(r), [int(k) for k in ks]] for r, ks in out[2]]))
    canon = R.canonical_deck_values()

    def batch(m, ncards, distinct):
        cards = np.full((m, 7), 0xFF, np.uint8)
        rank = np.zeros(m, np.uint8)
        kick = np.zeros(m, np.uint32)
        nk = np.zeros(m, np.uint8)
        for i in range(m):
            idx = rng.choice(52, ncards, replace=not distinct) if ncards else []
            vals = [canon[j] for j in idx]
            cards[i, :ncards] = vals
            rank[i], kick[i], nk[i] = pack_eval(J.eval_hand([Card(int(v)) for v in vals]))
        return cards, rank, kick, nk

    arrays = {}
    parts = [batch(20000, 7, True), batch(4000, 7, False)]
    for nc in range(0, 7):
        parts.append(batch(1500, nc, True))
        if nc >= 2:
            parts.append(batch(500, nc, False))
    ncards = np.concatenate([np.full(len(p[0]), (p[0][0] != 0xFF).sum() if len(p[0]) else 0, np.uint8)
                             for p in parts])
    arrays["eval_cards"] = np.concatenate([p[0] for p in parts])
    arrays["eval_ncards"] = (arrays["eval_cards"] != 0xFF).sum(axis=1).astype(np.uint8)
    del ncards
    arrays["eval_rank"] = np.concatenate([p[1] for p in parts])
    arrays["eval_kick"] = np.concatenate([p[2] for p in parts])
    arrays["eval_nkick"] = np.concatenate([p[3] for p in parts])

    # compare_rankings on random ranking lists (incl. NONE entries and exact ties), judger.py:111-158
    m = 6000
    cr_n = np.zeros(m, np.uint8)
    cr_rank = np.full((m, 10), 10, np.uint8)
    cr_kick = np.zeros((m, 10), np.uint32)
    cr_onehot = np.zeros((m, 10), np.uint8)
    for i in range(m):
        n = int(rng.integers(1, 11))
        cr_n[i] = n
        board = [Card(int(canon[j])) for j in rng.choice(52, 5, replace=False)] if i % 2 else None
        rankings = []
        for p in range(n):
            if rng.random() < 0.25:
                rankings.append((10, []))
                continue
            if board is not None:  # shared board -> frequent equal ranks / exact ties
                hole = [Card(int(canon[j])) for j in rng.choice(52, 2, replace=False)]
                rankings.append(J.eval_hand(board + hole))
            else:
                rankings.append(J.eval_hand([Card(int(canon[j])) for j in rng.choice(52, 7, replace=False)]))
        onehot, winners = J.compare_rankings(rankings)
        for p, (r, k) in enumerate(rankings):
            cr_rank[i, p] = r
            cr_kick[i, p] = J.get_kickers_value(k)
        cr_onehot[i, :n] = onehot
    arrays.update(cr_n=cr_n, cr_rank=cr_rank, cr_kick=cr_kick, cr_onehot=cr_onehot)
    return dict(kat=kat, quirks=quirks, compare_kat=cmp_kat), arrays


# --------------------------------------------------------------------------- main
SEED = R.DEFAULT_SEED
GAME_SETS = {
    # name: (n, policy, seed, tables, steps, table_id_base, cfg)
    "game_n2_random": (2, R.POLICY_RANDOM, SEED, 8, 256, 0, None),
    "game_n6_random": (6, R.POLICY_RANDOM, SEED, 8, 256, 0, None),
    "game_n9_random": (9, R.POLICY_RANDOM, SEED, 6, 200, 0, None),
    "game_n6_allin": (6, R.POLICY_ALLIN, SEED, 6, 128, 0, None),
    "game_n9_allin": (9, R.POLICY_ALLIN, SEED, 6, 128, 0, None),
    "game_n4_example_cfg": (4, R.POLICY_RANDOM, SEED ^ 0x5555, 6, 200, 1000,
                            dict(start_credits=1000, big_blind=40, small_blind=20)),  # examples/random_game.py:9
    "game_n3_percredits": (3, R.POLICY_RANDOM, 7, 6, 200, 77,
                           dict(start_credits=[30, 100, 5], big_blind=4, small_blind=2)),
    "game_n10_random": (10, R.POLICY_RANDOM, 99, 4, 150, 5, None),
    # round 3: more than ten seats (PK_MAX_PLAYERS 15: np.sum's unrolled block once, np.argsort's insertion sort)
    "game_n12_random": (12, R.POLICY_RANDOM, 1212, 4, 160, 3, None),
    "game_n15_random": (15, R.POLICY_RANDOM, 1515, 4, 160, 0, dict(start_credits=50, big_blind=4, small_blind=2)),
    # round 4: sixteen seats (PK_MAX_PLAYERS 16: np.sum runs its unrolled block of eight TWICE, np.argsort is still the insertion sort)
    "game_n16_random": (16, R.POLICY_RANDOM, 1616, 4, 160, 0, dict(start_credits=50, big_blind=4, small_blind=2)),
}
# odd configurations found worth pinning by tests/golden/fuzz_oracle_vs_reference.py: (n, policy, seed, tables, steps, base, cfg, dealer)
# resumed RNG streams: hand_serial crosses 2^32 and the action block index (step_serial >> 3) crosses 2^32 mid-run
SERIAL_SETS = {
    "game_n6_serial_hi": (6, R.POLICY_RANDOM, SEED, 6, 120, 70000, None, ((1 << 32) - 9, (1 << 35) - 37)),
}
# observation contract: StateView.__getstate__ tuples of the reference itself, every seat
# A StateView held ACROSS a Game.step (SURVEY a13 "arrays are aliases of live game arrays"): `self.credits = game.credits` (game.py:128-130) shares
# the game's numpy arrays, so the held view's credits / bets change with the game (they are only ever mutated in place: game.py:408, :457-458, :480,
# :528, :554-555); `pending_bets` is shared until the next setup_hand REBINDS the game's attribute (game.py:445 `self.pending_bets = np.minimum(...)`),
# after which the view keeps the old array as :438-440 left it (zeros + the new hand's blinds, unclipped).  Everything else in the view is a value or
# a fresh object.  The product's StateView is a SNAPSHOT (pokerl_amd/state_view.py); this fixture pins what the reference does, so that the
# difference is a documented, tested rule: INTEGRATION.md section 3.
ALIAS_SETS = {
    "views_alias_n6_random": (6, R.POLICY_RANDOM, SEED ^ 0xA11A5, 4, 90, 0, None),
    "views_alias_n3_percredits": (3, R.POLICY_RANDOM, 99, 4, 90, 5, dict(start_credits=[30, 100, 5], big_blind=4, small_blind=2)),
}

VIEW_SETS = {
    "views_n6_random": (6, R.POLICY_RANDOM, SEED ^ 0x77, 4, 60, 0, None),
    "views_n3_percredits": (3, R.POLICY_RANDOM, 7, 4, 60, 77, dict(start_credits=[30, 100, 5], big_blind=4, small_blind=2)),
    "views_n13_random": (13, R.POLICY_RANDOM, 1313, 2, 24, 0, None),
    "views_n16_random": (16, R.POLICY_RANDOM, 1616, 2, 24, 3, None),
}
ODD_SETS = {
    "game_n5_zero_blinds": (5, R.POLICY_RANDOM, 21, 6, 150, 9, dict(start_credits=10, big_blind=0, small_blind=0), 3),
    "game_n4_sb_gt_bb_fractional": (4, R.POLICY_RANDOM, 22, 6, 150, 0, dict(start_credits=[37.5, 3, 1000, 0.5], big_blind=0.25, small_blind=7.5), 1),
    "game_n7_blinds_gt_stacks": (7, R.POLICY_RANDOM, 23, 6, 150, 4000000000, dict(start_credits=5, big_blind=40, small_blind=250), 6),
    "game_n8_mixed_allin": (8, R.POLICY_ALLIN, 24, 6, 100, 0, dict(start_credits=[1, 2, 3, 5, 10, 100, 1000, 0.5], big_blind=3, small_blind=1), 0),
    "game_n14_mixed_allin": (14, R.POLICY_ALLIN, 1414, 4, 100, 77,
                             dict(start_credits=[1, 2, 3, 5, 10, 100, 1000, 0.5, 37.5, 3, 2, 10, 5, 100], big_blind=3, small_blind=1), 11),
    "game_n16_mixed_allin": (16, R.POLICY_ALLIN, 1616, 4, 100, 5,
                             dict(start_credits=[1, 2, 3, 5, 10, 100, 1000, 0.5, 37.5, 3, 2, 10, 5, 100, 7, 2], big_blind=3, small_blind=1), 13),
}
# Configurations whose payoffs DEPEND on the order in which np.argsort(bets) (game.py:495) returns seats with EQUAL bets
# (found with the fuzz generator): the reference with its pinned numpy (stable), which the fixtures pin, differs from the
# reversed tie rule AND from the un-injected numpy 2.2.6 of this AVX-512 host (x86-simd-sort is not stable).  The
# generator asserts both, so these vectors are the reference-held evidence for "ascending seat index among equal bets".
TIE_SETS = {
    "game_n8_argsort_tie": (8, R.POLICY_RANDOM, 349423999861, 4, 100, 0, dict(start_credits=1, big_blind=40, small_blind=2)),
    "game_n9_argsort_tie": (9, R.POLICY_RANDOM, 141532477888, 4, 100, 0, dict(start_credits=10, big_blind=7.5, small_blind=40)),
    # sixteen seats: the widest table whose argsort the pinned numpy still insertion-sorts (found by scanning seeds, round 4)
    "game_n16_argsort_tie": (16, R.POLICY_RANDOM, 1001, 4, 60, 0, dict(start_credits=1, big_blind=40, small_blind=2)),
}
# The one configuration of the fuzz (tests/golden/fuzz_oracle_vs_reference.py, round 200 of its generator) on which the
# reference DOES return from a Game.step that rolls more than PK_HAND_CAP = 4 096 hands (5 204 of them, step 9): the product
# ends that step after 4 097 hands with PK_TERR_HAND_CAP (errs == 4) -- the documented divergence, pinned here with the
# reference's own table state at that point (_HandCapProbe) and the reset that follows.
CAP_SETS = {
    "game_n6_hand_cap": (6, R.POLICY_RANDOM, 3107974733015276566, 1, 12, 551120854,
                         dict(start_credits=[37.5, 5, 1, 2, 2, 0.5], big_blind=0.5, small_blind=250), 5),
}
NORESET_SETS = {
    "game_n2_noreset": (2, R.POLICY_RANDOM, 11, 6, 150, 0, None),
    "game_n3_noreset": (3, R.POLICY_RANDOM, 12, 6, 200, 0, dict(start_credits=20, big_blind=2, small_blind=1)),
}
DIGEST_SETS = {
    # long runs pinned by sha256 digests only (every 100 steps)
    "digest_n2_random": (2, R.POLICY_RANDOM, SEED, 64, 2000, 0, None),
    "digest_n6_random": (6, R.POLICY_RANDOM, SEED, 64, 2000, 0, None),
    "digest_n9_random": (9, R.POLICY_RANDOM, SEED, 32, 1500, 0, None),
    "digest_n9_allin": (9, R.POLICY_ALLIN, SEED, 32, 1000, 0, None),
    "digest_n6_shard1": (6, R.POLICY_RANDOM, SEED, 32, 1000, 65536, None),  # table_id_base of rank 1 at C4
    "digest_n6_shard7": (6, R.POLICY_RANDOM, SEED, 32, 1000, 7 * 65536, None),  # ... of rank 7 (last shard of 524 288)
    "digest_n15_random": (15, R.POLICY_RANDOM, SEED, 16, 800, 0, None),
    "digest_n16_random": (16, R.POLICY_RANDOM, SEED, 16, 800, 0, None),
}
# Deep hands: the never-fold caller of rng_spec.py (POLICY_DEEP, test infrastructure) on per-seat fractional stacks -- raises on several
# streets, short stacks all-in on different streets, multi-way river showdowns that pay several different amounts.  First dealer N - 1,
# table ids that wrap 2^32 inside the set.  (n, seed, tables, steps)
def deep_cfg(n, reverse=False):
    return dict(start_credits=[7.5 * (p + 1) + 0.25 * (p % 3) for p in range(n)][::-1 if reverse else 1], big_blind=2, small_blind=1)


DEEP_BASE = 2 ** 32 - 3
DEEP_GAME_SETS = {"game_n%d_deep" % n: (n, 0xDEE9 + n, 6 if n <= 9 else 4, 200 if n <= 9 else 250) for n in (2, 3, 6, 9, 13, 16)}
# seat 0 deep against call agents: every hand an N-way river showdown raised on every street; and against a different agent per seat.
# PokerGameEnv.step never returns early for a seat 0 that goes broke while an OPPONENT's step ends the hand (game_env.py:49-52 then plays
# the opponents until the game is over), and call agents alone need thousands of hands for that: the product ends such a step with
# PK_TERR_ENV_CAP, a documented divergence no fixture can hold.  So seeds and lengths are chosen (by scanning with the oracle) such
# that no env.step of the set plays 8 192 Game.steps, and at sixteen seats the stacks are dealt in REVERSE seat order (seat 0 the deepest):
# with seat 0 the shortest of sixteen no seed gives more than three such steps.  (n, opponents, seed, tables, steps, stacks reversed)
DEEP_ENV_SETS = {
    "env_n4_deep_vs_call": (4, R.POLICY_CALL, 0xDEE9 + 104, 6, 150, False),
    "env_n9_deep_vs_call": (9, R.POLICY_CALL, 0xDEE9 + 109 + 72000, 4, 110, False),
    "env_n16_deep_vs_call": (16, R.POLICY_CALL, 0xDEE9 + 116 + 11000, 4, 85, True),
    "env_n6_deep_vs_mixed": (6, [R.POLICY_CALL, R.POLICY_RANDOM, R.POLICY_CALL, R.POLICY_ALLIN, R.POLICY_CALL], 0xDEE9 + 206, 6, 150, False),
}
ENV_SETS = {
    "env_n4_random": (4, R.POLICY_RANDOM, R.POLICY_RANDOM, SEED, 8, 200, 0, None),
    "env_n6_random": (6, R.POLICY_RANDOM, R.POLICY_RANDOM, SEED, 6, 200, 0, None),
    "env_n6_vs_allin": (6, R.POLICY_RANDOM, R.POLICY_ALLIN, SEED, 6, 150, 0, None),
    "env_n2_random": (2, R.POLICY_RANDOM, R.POLICY_RANDOM, SEED, 8, 200, 0, None),
    # odd configurations (round 2): per-seat stacks with seat 0 short, nine seats at a high table-id base, blinds above
    # most stacks against all-in opponents
    "env_n5_percredits": (5, R.POLICY_RANDOM, R.POLICY_RANDOM, 1234567, 6, 150, 4096,
                          dict(start_credits=[5, 100, 37.5, 1000, 10], big_blind=3, small_blind=7.5)),
    "env_n9_random_hi_base": (9, R.POLICY_RANDOM, R.POLICY_RANDOM, 99, 4, 120, 4000000000, None),
    "env_n3_big_blinds_vs_allin": (3, R.POLICY_RANDOM, R.POLICY_ALLIN, 2026, 6, 120, 0,
                                   dict(start_credits=[10, 40, 100], big_blind=40, small_blind=2)),
    # round 3: the call agent (rng_spec policy 2) and a DIFFERENT agent per opponent seat, as PokerGameEnv(agents=[...]) takes them
    "env_n3_vs_call": (3, R.POLICY_RANDOM, R.POLICY_CALL, 31337, 6, 150, 0, None),
    "env_n4_mixed_opponents": (4, R.POLICY_RANDOM, [R.POLICY_CALL, R.POLICY_RANDOM, R.POLICY_ALLIN], SEED ^ 0x1234, 6, 150, 0, None),
    "env_n6_mixed_percredits": (6, R.POLICY_RANDOM, [R.POLICY_CALL, R.POLICY_CALL, R.POLICY_ALLIN, R.POLICY_RANDOM, R.POLICY_CALL],
                                424242, 6, 150, 123456, dict(start_credits=[50, 100, 20, 200, 100, 75], big_blind=4, small_blind=2)),
    "env_n2_call_vs_call": (2, R.POLICY_CALL, R.POLICY_CALL, 5, 4, 120, 0, dict(start_credits=6, big_blind=2, small_blind=1)),
    # more than ten seats: random opponents, and one agent per seat with seats 8..10 (policy nibbles above bit 31) differing
    "env_n11_random": (11, R.POLICY_RANDOM, R.POLICY_RANDOM, 1111, 4, 100, 0, None),
    "env_n12_mixed_opponents": (12, R.POLICY_RANDOM, [R.POLICY_RANDOM, R.POLICY_ALLIN, R.POLICY_RANDOM, R.POLICY_CALL, R.POLICY_RANDOM, R.POLICY_RANDOM,
                                                     R.POLICY_ALLIN, R.POLICY_CALL, R.POLICY_ALLIN, R.POLICY_RANDOM, R.POLICY_CALL],
                                1212, 4, 100, 9, dict(start_credits=40, big_blind=4, small_blind=2)),
    # sixteen seats: one agent per opponent seat, the policy nibble of seat 15 in bits 60..63 of the word
    "env_n16_mixed_opponents": (16, R.POLICY_RANDOM, [R.POLICY_RANDOM, R.POLICY_ALLIN, R.POLICY_RANDOM, R.POLICY_CALL, R.POLICY_RANDOM, R.POLICY_RANDOM,
                                                     R.POLICY_ALLIN, R.POLICY_CALL, R.POLICY_ALLIN, R.POLICY_RANDOM, R.POLICY_CALL, R.POLICY_RANDOM,
                                                     R.POLICY_CALL, R.POLICY_RANDOM, R.POLICY_ALLIN],
                                1616, 4, 100, 16, dict(start_credits=40, big_blind=4, small_blind=2)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()

    def want(name):
        return args.only is None or args.only == name

    if want("judger"):
        js, arrays = judger_vectors()
        with open(os.path.join(HERE, "judger_kat.json"), "w") as f:
            json.dump(js, f, indent=1)
        np.savez_compressed(os.path.join(HERE, "judger_vectors.npz"), **arrays)
        print("judger: %d eval vectors, %d compare vectors" % (len(arrays["eval_rank"]), len(arrays["cr_n"])))
    for name, (n, pol, seed, tables, steps, base, cfg) in GAME_SETS.items():
        if want(name):
            out = game_trajectory(n, pol, seed, tables, steps, base, cfg)
            np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
            print(name, "resets:", len(out["reset_idx"]), "hands:", int(out["post_hand_serial"].max()))
    for name, (n, seed, tables, steps) in DEEP_GAME_SETS.items():
        if want(name):
            out = game_trajectory(n, R.POLICY_DEEP, seed, tables, steps, DEEP_BASE, deep_cfg(n), dealer=n - 1)
            meta = json.loads(str(out["meta"]))
            assert meta["river_showdowns_3way"] > 0 or n == 2, meta
            assert meta["hands_paying_3_amounts"] > 0 or n == 2, meta
            assert not out["errs"].any() and not (out["actions"] == 0).any()
            np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
            print(name, "resets:", len(out["reset_idx"]), "hands:", int(out["post_hand_serial"].max()), "river showdowns 3+-way:",
                  meta["river_showdowns_3way"], "hands paying 3+ amounts:", meta["hands_paying_3_amounts"])
    for name, (n, opp, seed, tables, steps, reverse) in DEEP_ENV_SETS.items():
        if want(name):
            out = env_trajectory(n, R.POLICY_DEEP, opp, seed, tables, steps, DEEP_BASE, deep_cfg(n, reverse))
            meta = json.loads(str(out["meta"]))
            assert meta["river_showdowns_3way"] > 0 and meta["hands_paying_3_amounts"] > 0, meta
            np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
            print(name, "episodes:", int(out["done"].sum()), "river showdowns 3+-way:", meta["river_showdowns_3way"],
                  "hands paying 3+ amounts:", meta["hands_paying_3_amounts"])
    for name, (n, pol, seed, tables, steps, base, cfg, dealer) in ODD_SETS.items():
        if want(name):
            out = game_trajectory(n, pol, seed, tables, steps, base, cfg, dealer=dealer)
            np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
            print(name, "resets:", len(out["reset_idx"]), "hands:", int(out["post_hand_serial"].max()))
    for name, (n, pol, seed, tables, steps, base, cfg) in TIE_SETS.items():
        if want(name):
            out = game_trajectory(n, pol, seed, tables, steps, base, cfg)

            def first_diff(other_np):
                G.np = other_np
                try:
                    alt = game_trajectory(n, pol, seed, tables, steps, base, cfg)
                finally:
                    G.np = _STABLE_NP
                diff = (out["post_payoffs"].view(np.uint64) != alt["post_payoffs"].view(np.uint64)).any(axis=(1, 2))
                return int(np.argmax(diff)) if diff.any() else -1

            rev, native = first_diff(_ReversedTieArgsortNumpy()), first_diff(np)
            assert rev >= 0, "%s does not depend on the argsort tie rule" % name
            native_is_stable = list(np.argsort(np.array([2., 1, 0, 0, 0, 0, 1]))) == [2, 3, 4, 5, 1, 6, 0]
            assert native >= 0 or native_is_stable, "%s: the un-injected numpy is unstable here yet gives the same payoffs" % name
            meta = json.loads(str(out["meta"]))
            meta["tie_rule"] = dict(rule="ascending seat index among equal bets (np.argsort of the reference's pinned numpy 1.18.4)",
                                    first_step_where_reversed_tie_rule_differs=rev,
                                    first_step_where_uninjected_numpy_differs=native, numpy=np.__version__)
            out["meta"] = np.array(json.dumps(meta))
            np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
            print(name, "resets:", len(out["reset_idx"]), "reversed tie rule differs from step", rev, "| un-injected numpy from step", native)
    for name, (n, pol, seed, tables, steps, base, cfg, dealer) in CAP_SETS.items():
        if want(name):
            out = game_trajectory(n, pol, seed, tables, steps, base, cfg, dealer=dealer, hand_cap=4096)
            meta = json.loads(str(out["meta"]))
            assert (out["errs"] == 4).sum() == 1 and meta["reference_hands_in_its_longest_step"] > 4097, meta
            np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
            print(name, "capped steps:", int((out["errs"] == 4).sum()), "at", np.argwhere(out["errs"] == 4).tolist(),
                  "reference rolled", meta["reference_hands_in_its_longest_step"], "hands there")
    for name, (n, pol, seed, tables, steps, base, cfg, sbase) in SERIAL_SETS.items():
        if want(name):
            out = game_trajectory(n, pol, seed, tables, steps, base, cfg, serial_base=sbase)
            np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
            print(name, "resets:", len(out["reset_idx"]), "hand_serial max: %#x" % int(out["post_hand_serial"].max()))
    for name, (n, pol, seed, tables, steps, base, cfg) in VIEW_SETS.items():
        if want(name):
            views = []
            out = game_trajectory(n, pol, seed, tables, steps, base, cfg, full=False, views=views)
            meta = json.loads(str(out["meta"]))
            meta["actions"] = out["actions"].tolist()
            meta["flags"] = out["flags"].tolist()
            meta["views"] = views            # [step][table] -> view_record, taken right after the step (before auto-reset)
            with open(os.path.join(HERE, name + ".json"), "w") as f:
                json.dump(meta, f)
            print(name, "view records:", len(views) * tables)
    for name, (n, pol, seed, tables, steps, base, cfg) in ALIAS_SETS.items():
        if want(name):
            held = []
            out = game_trajectory(n, pol, seed, tables, steps, base, cfg, full=False, held=held)
            meta = json.loads(str(out["meta"]))
            meta["actions"] = out["actions"].tolist()
            meta["flags"] = out["flags"].tolist()
            meta["held"] = held              # [step][table] -> the view made BEFORE the step, as it was then and as it reads after the step
            with open(os.path.join(HERE, name + ".json"), "w") as f:
                json.dump(meta, f)
            print(name, "held views:", len(held) * tables, "of which across a setup_hand:", sum(h["setup_hands"] > 0 for row in held for h in row))
    for name, (n, pol, seed, tables, steps, base, cfg) in NORESET_SETS.items():
        if want(name):
            out = game_trajectory(n, pol, seed, tables, steps, base, cfg, auto_reset=False)
            np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
            print(name, "assertion errors:", int((out["errs"] != 0).sum()), "game-over steps:", int((out["flags"] & 1).sum()))
    for name, (n, pol, seed, tables, steps, base, cfg) in DIGEST_SETS.items():
        if want(name):
            out = game_trajectory(n, pol, seed, tables, steps, base, cfg, full=False, digest_every=100)
            meta = json.loads(str(out["meta"]))
            meta["flags_sha256"] = hashlib.sha256(out["flags"].tobytes()).hexdigest()
            meta["actions_sha256"] = hashlib.sha256(out["actions"].tobytes()).hexdigest()
            with open(os.path.join(HERE, name + ".json"), "w") as f:
                json.dump(meta, f, indent=1)
            print(name, "digests:", len(meta["digests"]))
    for name, (n, pol, opp, seed, tables, steps, base, cfg) in ENV_SETS.items():
        if want(name):
            out = env_trajectory(n, pol, opp, seed, tables, steps, base, cfg)
            np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
            print(name, "episodes:", int(out["done"].sum()))


if __name__ == "__main__":
    main()
