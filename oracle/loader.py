"""ctypes binding of the CPU oracle (TEST INFRASTRUCTURE -- not product code).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import this.
The product package pokerl_amd never does.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libpokerl_oracle.so")

ERR_INVALID_ACTION, ERR_NO_WINNER, ERR_HAND_CAP, ERR_ENV_CAP = 1, 2, 4, 8
F_CREDITS, F_BETS, F_PENDING, F_PAYOFFS = 0, 1, 2, 3

_u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
_u64p = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")

_lib = None


def build(force=False):
    src = [os.path.join(HERE, f) for f in ("pokerl_oracle.c", "pokerl_oracle.h")]
    if force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in src):
        subprocess.check_call(["make", "-C", HERE, "-B", "libpokerl_oracle.so"], stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    build()
    L = C.CDLL(LIB_PATH)
    L.orc_create.restype = C.c_void_p
    L.orc_create.argtypes = [C.c_int, C.c_int, _f64p, C.c_double, C.c_double, C.c_uint64, C.c_uint32]
    L.orc_destroy.argtypes = [C.c_void_p]
    L.orc_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.orc_step.argtypes = [C.c_void_p, _i32p, _u8p, _u8p]
    L.orc_step.restype = C.c_int
    L.orc_valid_actions.argtypes = [C.c_void_p, _u8p]
    L.orc_valid_actions_for.argtypes = [C.c_void_p, C.c_int, _u8p]
    L.orc_pick_actions.argtypes = [C.c_void_p, C.c_int, _i32p]
    L.orc_rollout.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _u64p]
    L.orc_rollout.restype = C.c_int
    L.orc_env_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.orc_env_step.argtypes = [C.c_void_p, _i32p, C.c_int, _f64p, _u8p, _u8p, _u8p]
    L.orc_env_step.restype = C.c_int
    L.orc_env_reset_seats.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.orc_env_step_seats.argtypes = [C.c_void_p, _i32p, C.c_uint64, _f64p, _u8p, _u8p, _u8p]
    L.orc_env_step_seats.restype = C.c_int
    L.orc_get_f64.argtypes = [C.c_void_p, C.c_int, _f64p]
    L.orc_get_min_raise.argtypes = [C.c_void_p, _f64p]
    L.orc_get_states.argtypes = [C.c_void_p, _u8p]
    L.orc_get_cursors.argtypes = [C.c_void_p, _i32p]
    L.orc_get_serials.argtypes = [C.c_void_p, _u64p, _u64p]
    L.orc_get_errs.argtypes = [C.c_void_p, _u8p]
    L.orc_set_serials.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.orc_get_cards.argtypes = [C.c_void_p, _u8p]
    L.orc_get_showdown.argtypes = [C.c_void_p, _u8p, _u32p]
    L.orc_eval_hands.argtypes = [_u8p, C.c_void_p, C.c_size_t, _u8p, _u32p, _u8p]
    L.orc_eval_hands_bytes.argtypes = L.orc_eval_hands.argtypes
    L.orc_compare_rankings.argtypes = [_u8p, _u32p, C.c_int, _u8p]
    L.orc_compare_rankings.restype = C.c_int
    L.orc_philox4x32_10.argtypes = [_u32p, _u32p, _u32p]
    L.orc_deck.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, _u8p]
    L.orc_pick_action.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint, C.c_int]
    L.orc_pick_action.restype = C.c_int
    L.orc_eval7_digest.argtypes = [C.c_int, C.c_int, _u64p, _u64p]
    L.orc_eval7_prefix.argtypes = [C.c_int, C.c_int, _u32p]
    L.orc_eval7_prefix.restype = C.c_size_t
    L.orc_np_sum.argtypes = [_f64p, C.c_int]
    L.orc_np_sum.restype = C.c_double
    _lib = L
    return L


class OracleGame:
    """T lockstep tables of the reference Game (scalar C restatement)."""

    def __init__(self, num_tables, num_players, start_credits=100, big_blind=2, small_blind=1,
                 seed=0x706F6B65726C, table_id_base=0):
        self.L = lib()
        self.T, self.N = int(num_tables), int(num_players)
        sc = np.broadcast_to(np.asarray(start_credits, np.float64), (self.N,)).copy()
        self.h = self.L.orc_create(self.T, self.N, sc, float(big_blind), float(small_blind), int(seed), int(table_id_base))
        if not self.h:
            raise ValueError("orc_create failed")

    def __del__(self):
        if getattr(self, "h", None):
            self.L.orc_destroy(self.h)
            self.h = None

    @staticmethod
    def _mask(mask):
        if mask is None:
            return None, None
        m = np.ascontiguousarray(mask, np.uint8)
        return m, m.ctypes.data_as(C.c_void_p)

    def reset(self, mask=None, dealer=0):
        keep, p = self._mask(mask)
        self.L.orc_reset(self.h, p, int(dealer))

    def step(self, actions):
        a = np.ascontiguousarray(actions, np.int32)
        flags = np.zeros(self.T, np.uint8)
        err = np.zeros(self.T, np.uint8)
        self.L.orc_step(self.h, a, flags, err)
        return flags, err

    def errs(self):
        """Error bits each table's last Game.step left (how an error raised inside env_reset's loop becomes visible)."""
        e = np.zeros(self.T, np.uint8)
        self.L.orc_get_errs(self.h, e)
        return e

    def valid_actions(self):
        m = np.zeros(self.T, np.uint8)
        self.L.orc_valid_actions(self.h, m)
        return m

    def valid_actions_for(self, player):
        m = np.zeros(self.T, np.uint8)
        self.L.orc_valid_actions_for(self.h, int(player), m)
        return m

    def pick_actions(self, policy):
        a = np.zeros(self.T, np.int32)
        self.L.orc_pick_actions(self.h, int(policy), a)
        return a

    def rollout(self, K, policy, auto_reset=True):
        c = np.zeros(4, np.uint64)
        e = self.L.orc_rollout(self.h, int(K), int(policy), int(bool(auto_reset)), c)
        return c, e

    @staticmethod
    def _seats(opp_policy):
        """int: every opponent plays that policy; list: one policy per OPPONENT seat (seat 1 first), as the reference's
        PokerGameEnv(agents=[...]) takes them."""
        if isinstance(opp_policy, (list, tuple)):
            from . import rng_spec as R
            return R.seat_policies([0] + list(opp_policy))
        return 0x1111111111111111 * (int(opp_policy) & 15)

    def env_reset(self, mask=None, opp_policy=0):
        keep, p = self._mask(mask)
        self.L.orc_env_reset_seats(self.h, p, self._seats(opp_policy))

    def env_step(self, actions, opp_policy=0):
        a = np.ascontiguousarray(actions, np.int32)
        reward = np.zeros(self.T, np.float64)
        done = np.zeros(self.T, np.uint8)
        hand = np.zeros(self.T, np.uint8)
        err = np.zeros(self.T, np.uint8)
        self.L.orc_env_step_seats(self.h, a, self._seats(opp_policy), reward, done, hand, err)
        return reward, done, hand, err

    def set_serials(self, hand_serial=None, step_serial=None):
        """Resume the RNG streams at given 64-bit serials (scalars broadcast over tables)."""
        def arr(v):
            return None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.uint64), (self.T,)))
        hs, ss = arr(hand_serial), arr(step_serial)
        self.L.orc_set_serials(self.h, None if hs is None else hs.ctypes.data_as(C.c_void_p),
                               None if ss is None else ss.ctypes.data_as(C.c_void_p))

    def f64(self, field):
        out = np.zeros((self.T, self.N), np.float64)
        self.L.orc_get_f64(self.h, field, out)
        return out

    def snapshot(self):
        """Same fields/dtypes as tests/golden/make_golden.py SNAP_FIELDS, stacked over tables."""
        T, N = self.T, self.N
        cur = np.zeros((T, 6), np.int32)
        self.L.orc_get_cursors(self.h, cur)
        states = np.zeros((T, N), np.uint8)
        self.L.orc_get_states(self.h, states)
        mr = np.zeros(T, np.float64)
        self.L.orc_get_min_raise(self.h, mr)
        cards = np.zeros((T, min(52, 5 + 2 * N)), np.uint8)
        self.L.orc_get_cards(self.h, cards)
        srank = np.zeros((T, N), np.uint8)
        skick = np.zeros((T, N), np.uint32)
        self.L.orc_get_showdown(self.h, srank, skick)
        hs = np.zeros(T, np.uint64)
        ss = np.zeros(T, np.uint64)
        self.L.orc_get_serials(self.h, hs, ss)
        return dict(active=cur[:, 0].astype(np.uint8), turn=cur[:, 1].astype(np.uint8),
                    dealer=cur[:, 2].astype(np.uint8), sb=cur[:, 3].astype(np.uint8),
                    bb=cur[:, 4].astype(np.uint8), hand=cur[:, 5].copy(), states=states,
                    credits=self.f64(F_CREDITS), bets=self.f64(F_BETS), pending=self.f64(F_PENDING),
                    payoffs=self.f64(F_PAYOFFS), min_raise=mr, cards=cards, srank=srank, skick=skick,
                    valid=self.valid_actions(), hand_serial=hs, step_serial=ss)


def eval_hands(cards, ncards=None, any_bytes=False):
    """any_bytes: orc_eval_hands_bytes, pk_eval_hands' documented reading of bytes that are no card."""
    cards = np.ascontiguousarray(cards, np.uint8).reshape(-1, 7)
    m = cards.shape[0]
    rank = np.zeros(m, np.uint8)
    kick = np.zeros(m, np.uint32)
    nk = np.zeros(m, np.uint8)
    if ncards is None:
        p = None
    else:
        ncards = np.ascontiguousarray(ncards, np.uint8)
        p = ncards.ctypes.data_as(C.c_void_p)
    (lib().orc_eval_hands_bytes if any_bytes else lib().orc_eval_hands)(cards, p, m, rank, kick, nk)
    return rank, kick, nk


def compare_rankings(rank, kick):
    rank = np.ascontiguousarray(rank, np.uint8)
    kick = np.ascontiguousarray(kick, np.uint32)
    onehot = np.zeros(len(rank), np.uint8)
    lib().orc_compare_rankings(rank, kick, len(rank), onehot)
    return onehot


def eval7_digest(first_lo=0, first_hi=52):
    per_first = np.zeros(52, np.uint64)
    counts = np.zeros(11, np.uint64)
    lib().orc_eval7_digest(int(first_lo), int(first_hi), per_first, counts)
    return per_first, counts
