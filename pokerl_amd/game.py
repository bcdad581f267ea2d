"""VecGame: T independent reference `Game`s stepped in lockstep on one MI355X.

Host-side mirror of the reference's pokerl/game.py `Game` API for the data-parallel hot path: same method and
attribute names, same argument meaning and error behaviour, with a leading table axis on everything.  All game
logic runs in hand-written HIP kernels behind the C ABI of include/pokerl_hip.h (ctypes; no torch, no CPU fallback).
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .enums import PokerMoves

DEFAULT_SEED = 0x706F6B65726C  # 'pokerl'


def snapshot_nbytes(num_players, m):
    """Bytes of a snapshot blob of m table records at num_players seats (pk_snapshot_bytes); 0 for a seat count the ABI does not take."""
    return int(L.lib().pk_snapshot_bytes(int(num_players), int(m)))


class VecGame:
    """`Game(**config)` (pokerl/game.py:242-264) for `num_tables` tables.

    config: num_players=4, start_credits=100 (int or per-seat list/array), big_blind=2, small_blind=1, dealer=0 -- as
    the reference -- plus num_tables, seed, device, table_id_base (global id of table 0: RNG streams are keyed by the
    global table id, so a table's trajectory does not depend on which GPU/shard hosts it).
    """

    def __init__(self, num_tables=1, **config):
        self.num_tables = int(num_tables)
        self.num_players = int(config.get('num_players', 4))
        self.start_credits = config.get('start_credits', 100)
        self.big_blind = config.get('big_blind', 2)
        self.small_blind = config.get('small_blind', 1)
        self.dealer = int(config.get('dealer', 0))
        self.seed = int(config.get('seed', DEFAULT_SEED))
        self.device = int(config.get('device', 0))
        self.table_id_base = int(config.get('table_id_base', 0))
        if not (L.MIN_PLAYERS <= self.num_players <= L.MAX_PLAYERS):
            raise ValueError('num_players must be in [%d, %d]' % (L.MIN_PLAYERS, L.MAX_PLAYERS))
        self._lib = L.lib()
        self._h = C.c_void_p()
        if isinstance(self.start_credits, (int, float, np.integer, np.floating)):
            sc, scalar = None, float(self.start_credits)
        else:
            sc = np.ascontiguousarray(self.start_credits, np.float64)
            if sc.shape != (self.num_players,):
                raise ValueError('start_credits must be a scalar or one value per player')
            scalar = 0.0
        rc = self._lib.pk_create(C.byref(self._h), self.device, self.num_tables, self.num_players, L.ptr(sc), scalar,
                                 float(self.big_blind), float(self.small_blind), self.dealer, self.seed,
                                 self.table_id_base)
        if rc != L.PK_OK:
            self._h = C.c_void_p()
            L.check(rc)

    def close(self):
        if getattr(self, '_h', None) and self._h.value:
            self._lib.pk_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ reset / step
    def reset(self, mask=None, **config):
        """`Game.reset(**config)` (game.py:397-412) on every table, or on tables where mask != 0.  Only `dealer` is
        re-read from config (game.py:403)."""
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        if m is not None and m.shape != (self.num_tables,):
            raise ValueError('mask must have shape (num_tables,)')
        L.check(self._lib.pk_reset(self._h, L.ptr(m), int(config.get('dealer', 0))), self._h)

    def _actions(self, actions):
        a = np.asarray(actions)
        if a.dtype.kind not in 'iu':          # game.py:646,700: only int actions are implemented
            raise NotImplementedError
        a = np.ascontiguousarray(np.broadcast_to(a, (self.num_tables,)), np.int32)
        return a

    def step(self, actions, strict=True):
        """`Game.step(action)` (game.py:621-700), one action per table.

        Returns (game_over, hand_over, turn_over) as bool arrays [T] -- the reference's tuple, vectorised.
        strict=True mirrors the reference's error contract for the batch: if ANY action is invalid a ValueError
        ('Player %d invalid move: `%s`', game.py:651) is raised before any table is mutated.  strict=False steps the
        tables whose action is valid, leaves the others untouched and returns a 4th array of per-table error bits.
        """
        a = self._actions(actions)
        if strict:
            self.check_actions(a)
        flags = np.zeros(self.num_tables, np.uint8)
        terr = np.zeros(self.num_tables, np.uint8)
        rc = self._lib.pk_step(self._h, L.ptr(a), L.ptr(flags), L.ptr(terr))
        L.check(rc, self._h, allow_table_errors=True)
        out = ((flags & L.FLAG_GAME_OVER) != 0, (flags & L.FLAG_HAND_OVER) != 0, (flags & L.FLAG_TURN_OVER) != 0)
        if strict:
            if (terr & L.TERR_NO_WINNER).any():   # game.py:473
                raise AssertionError('Invalid state: no potential winner (table %d)' % int(np.argmax(terr & L.TERR_NO_WINNER)))
            if terr.any():
                raise L.PokerlHipError('table error bits %s' % np.unique(terr))
            return out
        return out + (terr,)

    # ---- device-resident forms (a learner on the same GPU: no host round trip; asynchronous on the handle's stream)
    @staticmethod
    def _dptr(p):
        """A device pointer as c_void_p: an int (tensor.data_ptr()), a c_void_p, or an object with .ptr (hipmem.DeviceBuffer)."""
        if p is None:
            return None
        if hasattr(p, 'ptr'):
            p = p.ptr
        return p if isinstance(p, C.c_void_p) else C.c_void_p(int(p))

    def step_d(self, actions_d, flags_d, terr_d=None, auto_reset=False):
        """`Game.step` (game.py:621-700) on DEVICE buffers (pk_step_d): actions_d i32[T] in, flags_d u8[T] (PK_FLAG_* bits =
        the reference's (game_over, hand_over, turn_over)) and terr_d u8[T] (optional) out.  A table whose action is not
        valid is left untouched and gets PK_TERR_INVALID_ACTION (game.py:649-651); nothing is raised -- the caller reads
        terr_d.  Asynchronous: order it with your stream through set_stream / wait_event / record_event.
        auto_reset=True (pk_step_auto_d): a table whose step ends its game is `Game.reset()` in the same launch (flags_d still says
        game_over) -- the rollout loop of examples/random_game.py:8-12 without a separate reset launch."""
        fn = self._lib.pk_step_auto_d if auto_reset else self._lib.pk_step_d
        L.check(fn(self._h, self._dptr(actions_d), self._dptr(flags_d), self._dptr(terr_d)), self._h)

    def step_async_d(self, actions_d, flags_d, terr_d, ready_d, max_hands=1, auto_reset=False):
        """`Game.step` as a bounded launch (pk_step_async_d): tables whose step has returned get ready_d[t] = 1 and their flags_d /
        terr_d; a table whose step rolls on through further hands (game.py:607-611) stays in flight on the device, ready_d[t] = 0,
        and the next call carries on with it, ignoring actions_d[t].  max_hands <= 0 drains (every table ready); until then every
        other method that reads or changes tables raises (PK_E_BUSY).  Per table the steps, flags and RNG draws are the synchronous ones.
        A drain is a full step call -- idle tables are stepped with actions_d[t] -- unless actions_d is None (drain only: nobody steps, idle
        tables come back untouched with TERR_INVALID_ACTION in terr_d)."""
        L.check(self._lib.pk_step_async_d(self._h, self._dptr(actions_d), self._dptr(flags_d), self._dptr(terr_d), self._dptr(ready_d),
                                          int(max_hands), int(bool(auto_reset))), self._h)

    def set_step_obs(self, obs_d=None, obs_packed_d=None):
        """`game.active_state` (game.py:323-332) from the step kernels themselves (pk_set_step_obs): from now on step_d / step_async_d (and
        step) write the StateView row of the player to act of every table whose step returned into obs_d (f64 [T, PK_OBS_DIM(N)], the row of
        observations_of(None)) and / or obs_packed_d ([T] rows of state_view.packed_dtype(N)) -- device buffers the caller keeps alive;
        None, None switches it off.  One launch per step instead of step + observation."""
        L.check(self._lib.pk_set_step_obs(self._h, self._dptr(obs_d), self._dptr(obs_packed_d)), self._h)

    def pick_actions_d(self, actions_d, policy=0):
        """The action the in-kernel agent `policy` takes on every table -> actions_d i32[T] (pk_pick_actions_d)."""
        L.check(self._lib.pk_pick_actions_d(self._h, int(policy), self._dptr(actions_d)), self._h)

    def reset_d(self, mask_d=None, mask_bits=0xff, dealer=0):
        """`Game.reset` on the tables with (mask_d[t] & mask_bits) != 0 (pk_reset_d; mask_d None = all): with step_d's flags_d
        and mask_bits = FLAG_GAME_OVER this is `if game_over: game.reset()` of examples/random_game.py:8-12 on the device."""
        L.check(self._lib.pk_reset_d(self._h, self._dptr(mask_d), int(mask_bits), int(dealer)), self._h)

    def check_actions(self, actions, table_offset=0):
        """Game.step's precondition (game.py:648-651) for the whole batch, checked on the device (pk_check_actions): raises
        the reference's ValueError naming the first offending table; nothing is mutated."""
        a = self._actions(actions)
        bad = C.c_int32(-1)
        L.check(self._lib.pk_check_actions(self._h, L.ptr(a), C.byref(bad)), self._h)
        if bad.value >= 0:
            t = bad.value
            name = PokerMoves.as_string[a[t]] if 0 <= a[t] < PokerMoves.NUM_MOVES else str(int(a[t]))
            raise ValueError('Player %d invalid move: `%s` (table %d)' % (int(self.active_player[t]), name, t + table_offset))

    def _seat(self, player):
        """None -> -1 (each table's active player); else a seat index valid for every table."""
        if player is None:
            return -1
        p = int(player)
        if not (0 <= p < self.num_players):
            raise IndexError('player %d out of range' % p)   # the reference's credits[player] would raise the same way
        return p

    def get_valid_actions(self, player=None):
        """`Game.get_valid_actions(player=None)` (game.py:339-383): (onehot f64 [T,7], generator of index arrays).
        player=None: each table's active player; an int: that seat on every table (0 IS seat 0 here, game.py:363)."""
        out = np.zeros((self.num_tables, PokerMoves.NUM_MOVES), np.uint8)
        L.check(self._lib.pk_get_valid_actions(self._h, self._seat(player), L.ptr(out)), self._h)
        onehot = out.astype(np.float64)
        return onehot, (np.nonzero(row)[0] for row in out)

    # ------------------------------------------------------------------ throughput / agents
    def pick_actions(self, policy=0):
        a = np.zeros(self.num_tables, np.int32)
        L.check(self._lib.pk_pick_actions(self._h, int(policy), L.ptr(a)), self._h)
        return a

    def rollout(self, steps, policy=0, auto_reset=True, fused=True, counters=True):
        """`steps` lockstep Game.step()s per table with in-kernel agents (examples/random_game.py:8-12 as a kernel).
        Returns dict(steps, hands, evals, games) when counters=True (synchronises), else None (asynchronous)."""
        c = np.zeros(L.NUM_COUNTERS, np.uint64) if counters else None
        L.check(self._lib.pk_rollout(self._h, int(steps), int(policy), int(bool(auto_reset)), int(bool(fused)), L.ptr(c)),
                self._h)
        if c is not None:
            return dict(steps=int(c[0]), hands=int(c[1]), evals=int(c[2]), games=int(c[3]))

    def time_rollout(self, steps, policy=0, auto_reset=True, fused=True, reps=1):
        """Average device milliseconds per kernel launch (HIP events on the handle's stream) + counters."""
        ms = C.c_double(0.0)
        c = np.zeros(L.NUM_COUNTERS, np.uint64)
        L.check(self._lib.pk_time_rollout(self._h, int(steps), int(policy), int(bool(auto_reset)), int(bool(fused)),
                                          int(reps), C.byref(ms), L.ptr(c)), self._h)
        return ms.value, dict(steps=int(c[0]), hands=int(c[1]), evals=int(c[2]), games=int(c[3]))

    def sync(self):
        """Completes deferred rollout steps and waits for the handle's stream."""
        L.check(self._lib.pk_sync(self._h), self._h)

    def flush(self):
        L.check(self._lib.pk_flush(self._h), self._h)

    @property
    def owed(self):
        """Diagnostic: steps each table still owes after the launches queued so far (deferred work is NOT completed)."""
        out = np.zeros(self.num_tables, np.uint32)
        L.check(self._lib.pk_get_owed(self._h, L.ptr(out)), self._h)
        return out

    def set_tuning(self, park=0, endk=0):
        L.check(self._lib.pk_set_tuning(self._h, int(park), int(endk)), self._h)

    def set_coalesce(self, max_steps):
        """Asynchronous rollout calls that arrive while two launches are in flight are merged on the host into launches
        of up to `max_steps` steps (0: every call launches; default 1024)."""
        L.check(self._lib.pk_set_coalesce(self._h, int(max_steps)), self._h)

    def launch_stats(self, reset=False):
        """dict(launches, steps, min, max) of the fused rollout launches since the last reset."""
        out = np.zeros(4, np.uint64)
        L.check(self._lib.pk_get_launch_stats(self._h, L.ptr(out), int(bool(reset))), self._h)
        return dict(launches=int(out[0]), steps=int(out[1]), min=int(out[2]), max=int(out[3]))

    # ------------------------------------------------------------------ streams (callers with their own HIP stream)
    @property
    def stream(self):
        s = C.c_void_p()
        L.check(self._lib.pk_get_stream(self._h, C.byref(s)), self._h)
        return s.value

    def set_stream(self, stream):
        """Run on the caller's hipStream_t (int / c_void_p).  0 / None IS a stream -- the legacy default stream, which is
        what torch.cuda.current_stream().cuda_stream returns outside a torch.cuda.Stream context; use_own_stream() goes
        back to the handle's own non-blocking stream."""
        L.check(self._lib.pk_set_stream(self._h, C.c_void_p(stream) if isinstance(stream, int) else stream), self._h)

    def use_own_stream(self):
        L.check(self._lib.pk_use_own_stream(self._h), self._h)

    def wait_event(self, event):
        L.check(self._lib.pk_wait_event(self._h, C.c_void_p(event) if isinstance(event, int) else event), self._h)

    def record_event(self, event):
        L.check(self._lib.pk_record_event(self._h, C.c_void_p(event) if isinstance(event, int) else event), self._h)

    @property
    def wave_shape(self):
        """(tables per wavefront, ... of the PokerGameEnv kernels) as pk_create laid this handle out (pk_get_wave_shape): powers of two, 64
        only above 32 768 tables unless PK_TPB / PK_ENV_TPB say otherwise.  Results do not depend on it."""
        a, b = C.c_int(), C.c_int()
        L.check(self._lib.pk_get_wave_shape(self._h, C.byref(a), C.byref(b)), self._h)
        return a.value, b.value

    # ------------------------------------------------------------------ RNG-spec serials (checkpoint / resume)
    def _serials(self):
        hs = np.zeros(self.num_tables, np.uint64)
        ss = np.zeros(self.num_tables, np.uint64)
        L.check(self._lib.pk_get_serials(self._h, L.ptr(hs), L.ptr(ss)), self._h)
        return hs, ss

    hand_serial = property(lambda self: self._serials()[0])
    step_serial = property(lambda self: self._serials()[1])

    def set_serials(self, hand_serial=None, step_serial=None):
        def arr(v):
            return None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.uint64), (self.num_tables,)))
        hs, ss = arr(hand_serial), arr(step_serial)
        L.check(self._lib.pk_set_serials(self._h, L.ptr(hs), L.ptr(ss)), self._h)

    # ------------------------------------------------------------------ snapshots: save / load / clone tables (pokerl_hip.h "Snapshots")
    # A snapshot is a position-independent byte blob of table records (snapshot_nbytes(N, m) bytes).  Future randomness belongs to the
    # DESTINATION (its seed and table ids): a table restored into the same slot of a handle with the same seed and table_id_base continues
    # bit-identically; a table cloned into another slot plays its current hand on identically, then deals the decks of its new table id.
    def _config(self):
        sc = self.start_credits
        return dict(num_players=self.num_players, start_credits=sc if isinstance(sc, (int, float, np.integer, np.floating)) else list(np.asarray(sc, np.float64)),
                    big_blind=self.big_blind, small_blind=self.small_blind, dealer=self.dealer, seed=self.seed, device=self.device,
                    table_id_base=self.table_id_base)

    def _tables(self, tables, what='tables'):
        if tables is None:
            return None
        a = np.asarray(tables).reshape(-1)
        if a.dtype.kind not in 'iu':
            raise TypeError('%s must be integers' % what)
        if a.size and (a.min() < np.iinfo(np.int32).min or a.max() > np.iinfo(np.int32).max):   # a cast would wrap to another table
            raise IndexError('%s: table index out of range' % what)
        return np.ascontiguousarray(a, np.int32)

    def save(self, tables=None):
        """The records of `tables` (all tables if None, in order) as a uint8 blob (pk_save_tables)."""
        t = self._tables(tables)
        m = self.num_tables if t is None else len(t)
        blob = np.zeros(snapshot_nbytes(self.num_players, m), np.uint8)
        L.check(self._lib.pk_save_tables(self._h, L.ptr(t), m, L.ptr(blob)), self._h)
        return blob

    def load(self, blob, tables=None):
        """Restores the blob's records into `tables` (tables 0 .. m-1 if None); the records are checked on the device first and a blob
        that fails is refused as a whole (pk_load_tables).  Deferred and in-flight bookkeeping of the restored tables is cleared."""
        blob = np.ascontiguousarray(blob, np.uint8).reshape(-1)
        if blob.nbytes < 256:
            raise ValueError('not a snapshot blob (shorter than its header)')
        m = int(blob[16:24].view(np.uint64)[0])              # header: magic, version, N, 0, m
        t = self._tables(tables)
        if t is not None:
            m = len(t)
        if blob.nbytes < snapshot_nbytes(self.num_players, m):
            raise ValueError('blob too short for %d records of %d seats' % (m, self.num_players))
        L.check(self._lib.pk_load_tables(self._h, L.ptr(t), m, L.ptr(blob)), self._h)

    def save_d(self, blob_d, tables_d=None, m=None):
        """pk_save_tables_d: m records (default: every table, or tables_d's length must be given as m) into the device buffer blob_d of
        snapshot_nbytes(N, m) bytes; asynchronous on the handle's stream unless tables_d is given (its indices are checked first)."""
        m = self.num_tables if m is None else int(m)
        L.check(self._lib.pk_save_tables_d(self._h, self._dptr(tables_d), m, self._dptr(blob_d)), self._h)

    def load_d(self, blob_d, tables_d=None, m=None):
        """pk_load_tables_d: restores m records of the device blob blob_d (m defaults to every table)."""
        m = self.num_tables if m is None else int(m)
        L.check(self._lib.pk_load_tables_d(self._h, self._dptr(tables_d), m, self._dptr(blob_d)), self._h)

    @staticmethod
    def _observer(observer):
        if observer is None:
            return L.OBSERVER_NONE
        if observer == 'active':
            return L.OBSERVER_ACTIVE
        return int(observer)

    def clone_tables_d(self, dst_tables_d, src_tables_d, m, src=None, observer=None, nonce=0):
        """pk_clone_tables_d on device index arrays (int32 [m], None = 0 .. m-1): table src_tables_d[i] of `src` (default: this game)
        -> table dst_tables_d[i] of this game.  observer None: an exact copy; a seat or 'active' (= OBSERVER_ACTIVE): redeal the cards that
        seat cannot see (see pokerl_hip.h), drawn from this game's seed, the destination table id and `nonce`."""
        src = self if src is None else src
        L.check(self._lib.pk_clone_tables_d(self._h, self._dptr(dst_tables_d), src._h, self._dptr(src_tables_d), int(m),
                                            self._observer(observer), int(nonce) & 0xFFFFFFFFFFFFFFFF), self._h)

    def clone_tables(self, dst_tables, src_tables, src=None, observer=None, nonce=0):
        """clone_tables_d on host index arrays (src_tables broadcasts: [0] fans one table out to every destination); synchronous."""
        from .hipmem import DeviceBuffer
        src = self if src is None else src
        d = self._tables(dst_tables, 'dst_tables')
        m = self.num_tables if d is None else len(d)
        s = self._tables(src_tables, 'src_tables')
        if s is not None:
            s = np.ascontiguousarray(np.broadcast_to(s, (m,)) if s.size == 1 else s, np.int32)
            if len(s) != m:
                raise ValueError('src_tables and dst_tables differ in length')
        bufs = [None if a is None else DeviceBuffer(max(a.nbytes, 4), self.device).upload(a) for a in (d, s)]
        try:
            self.clone_tables_d(bufs[0], bufs[1], m, src=src, observer=observer, nonce=nonce)
            self.sync()
            if src is not self:
                src.sync()
        finally:
            for b in bufs:
                if b is not None:
                    b.free()

    def equity(self, tables=None):
        """Showdown equity of `tables` (all tables if None; indices may repeat) as they stand: every completion of the board enumerated on
        the device (pk_table_equity; definition: pokerl_hip.h "Showdown equity").  Board = the community cards dealt so far, hole cards =
        every seat's (all dead), live = the seats still in the hand; the future board cards the deck holds are unknown.  Returns a
        judger.Equity of [m, N] / [m] arrays; a table that cannot be evaluated (never reset, step in flight) has a non-zero status."""
        from .judger import Equity
        t = self._tables(tables)
        m = self.num_tables if t is None else len(t)
        n = self.num_players
        win, tie, share = np.zeros((m, n), np.uint32), np.zeros((m, n), np.uint32), np.zeros((m, n), np.uint64)
        boards, status = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
        L.check(self._lib.pk_table_equity(self._h, L.ptr(t), m, L.ptr(win), L.ptr(tie), L.ptr(share), L.ptr(boards), L.ptr(status)), self._h)
        return Equity(win, tie, share, boards, status)

    def equity_d(self, m=None, tables_d=None, win_d=None, tie_d=None, share_d=None, boards_d=None, status_d=None):
        """pk_table_equity_d: the same into device buffers (uint32 [m, N] win / tie, uint64 [m, N] share, uint32 [m] boards, uint8 [m]
        status; any may be None), asynchronous on the handle's stream.  m defaults to every table."""
        m = self.num_tables if m is None else int(m)
        L.check(self._lib.pk_table_equity_d(self._h, self._dptr(tables_d), m, self._dptr(win_d), self._dptr(tie_d), self._dptr(share_d),
                                            self._dptr(boards_d), self._dptr(status_d)), self._h)

    def equity_ev(self, tables=None):
        """Showdown EV in chips of `tables` (all tables if None; indices may repeat) as they stand: the side pots of end_hand over every
        completion of the board (pk_table_equity_ev; definition: pokerl_hip.h "Showdown EV").  Cards and live seats as equity(); an ACTIVE
        seat counts as one that shows down ("nobody bets further"), bets = bets + pending_bets.  Returns a judger.ShowdownEV of [m, N] /
        [m, N, N] / [m] arrays; a table that cannot be evaluated (never reset, step in flight, index out of range) has a non-zero status
        (`bets` and `payout` are None while asynchronous steps are in flight: they are formed from the getters)."""
        from .judger import NO_LEVEL, ShowdownEV
        t = self._tables(tables)
        m = self.num_tables if t is None else len(t)
        n = self.num_players
        share = np.zeros((m, n, n), np.uint64)
        level_seat = np.full((m, n), NO_LEVEL, np.uint8)
        amount, ev = np.zeros((m, n), np.float64), np.zeros((m, n), np.float64)
        boards, status = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
        L.check(self._lib.pk_table_equity_ev(self._h, L.ptr(t), m, L.ptr(share), L.ptr(level_seat), L.ptr(amount), L.ptr(ev), L.ptr(boards),
                                             L.ptr(status)), self._h)
        try:                            # (`bets` is formed from the getters, which refuse with PK_E_BUSY while asynchronous steps are in flight)
            bets = self.bets + self.pending_bets
            if t is not None:
                ok = (t >= 0) & (t < self.num_tables)
                bets = np.where(ok[:, None], bets[np.where(ok, t, 0)], 0.0)
        except L.PokerlHipError as e:
            if e.code != L.PK_E_BUSY:       # (any other failure of a getter is the caller's to see)
                raise
            bets = None
        return ShowdownEV(ev, share, level_seat, amount, boards, status, bets)

    def equity_ev_d(self, status_d, m=None, tables_d=None, share_d=None, level_seat_d=None, amount_d=None, ev_d=None, boards_d=None):
        """pk_table_equity_ev_d: the same into device buffers (uint64 [m, N, N] share, uint8 [m, N] level_seat, float64 [m, N] amount / ev,
        uint32 [m] boards, uint8 [m] status; any but status_d may be None), asynchronous on the handle's stream.  m defaults to every table."""
        m = self.num_tables if m is None else int(m)
        L.check(self._lib.pk_table_equity_ev_d(self._h, self._dptr(tables_d), m, self._dptr(share_d), self._dptr(level_seat_d), self._dptr(amount_d),
                                               self._dptr(ev_d), self._dptr(boards_d), self._dptr(status_d)), self._h)

    def _equity_observer(self, observer):
        """observer of equity_sampled: a seat, OBSERVER_ACTIVE / 'active', or OBSERVER_NONE / None; ValueError otherwise (before any call)."""
        o = self._observer(observer)
        if not (L.OBSERVER_ACTIVE <= o < self.num_players):
            raise ValueError('observer must be a seat 0 .. %d, OBSERVER_ACTIVE or OBSERVER_NONE' % (self.num_players - 1))
        return o

    def equity_sampled(self, tables=None, observer=L.OBSERVER_ACTIVE, samples=1024, nonce=0):
        """Sampled showdown equity of `tables` (all tables if None; indices may repeat) as `observer` sees them (pk_table_equity_sampled;
        definition: pokerl_hip.h "Sampled showdown equity"): a seat or OBSERVER_ACTIVE (each table's active seat) knows the board so far and
        its own two cards -- the other live seats' cards and the board to come are drawn `samples` times, folded hands are in the pool;
        OBSERVER_NONE knows every hole card and only the board is drawn.  The stream is the handle's seed, table id and `nonce`: the result
        does not depend on sharding, and counts of calls with different nonces add.  Returns a judger.SampledEquity of [m, N] / [m] arrays."""
        from .judger import SampledEquity, check_samples
        o = self._equity_observer(observer)
        samples, nonce = check_samples(samples, nonce)
        t = self._tables(tables)
        m = self.num_tables if t is None else len(t)
        n = self.num_players
        win, tie, share = np.zeros((m, n), np.uint32), np.zeros((m, n), np.uint32), np.zeros((m, n), np.uint64)
        count, status = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
        L.check(self._lib.pk_table_equity_sampled(self._h, L.ptr(t), m, o, samples, nonce, L.ptr(win), L.ptr(tie), L.ptr(share), L.ptr(count),
                                                  L.ptr(status)), self._h)
        return SampledEquity(win, tie, share, count, status)

    def equity_sampled_d(self, m=None, tables_d=None, observer=L.OBSERVER_ACTIVE, samples=1024, nonce=0, win_d=None, tie_d=None, share_d=None,
                         samples_d=None, status_d=None):
        """pk_table_equity_sampled_d: the same into device buffers (uint32 [m, N] win / tie, uint64 [m, N] share, uint32 [m] samples, uint8 [m]
        status; any may be None), asynchronous on the handle's stream.  m defaults to every table."""
        from .judger import check_samples
        o = self._equity_observer(observer)
        samples, nonce = check_samples(samples, nonce)
        m = self.num_tables if m is None else int(m)
        L.check(self._lib.pk_table_equity_sampled_d(self._h, self._dptr(tables_d), m, o, samples, nonce, self._dptr(win_d), self._dptr(tie_d),
                                                    self._dptr(share_d), self._dptr(samples_d), self._dptr(status_d)), self._h)

    def equity_ranged(self, tables=None, observer=L.OBSERVER_ACTIVE, ranges=None, range_of=None, samples=1024, nonce=0):
        """Sampled showdown equity of `tables` (all tables if None; indices may repeat) as `observer` (a seat or OBSERVER_ACTIVE) sees them,
        where every other live seat draws its holding from a weighted range (pk_table_equity_ranged; definition: pokerl_hip.h "Ranged
        sampled equity").  ranges: uint16 [1326] or [R, 1326], R <= 16; range_of: the row of each SEAT, [N] for all tables or [m, N] per
        table (0xFFFF = uniform; None: uniform, or the one row where ranges is a single vector); the observer's own entry is ignored.  The
        stream is the handle's seed, table id and `nonce`, as equity_sampled.  Returns a judger.RangedEquity of [m, N] / [m] arrays."""
        from .judger import RangedEquity, check_ranges, check_samples
        o = self._range_observer(observer)
        samples, nonce = check_samples(samples, nonce)
        t = self._tables(tables)
        m = self.num_tables if t is None else len(t)
        n = self.num_players
        w, r, ro, per = check_ranges(ranges, range_of, n, m)
        win, tie, share = np.zeros((m, n), np.uint32), np.zeros((m, n), np.uint32), np.zeros((m, n), np.uint64)
        count, status = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
        L.check(self._lib.pk_table_equity_ranged(self._h, L.ptr(t), m, o, samples, nonce, L.ptr(w), r, L.ptr(ro), int(per), L.ptr(win), L.ptr(tie),
                                                 L.ptr(share), L.ptr(count), L.ptr(status)), self._h)
        return RangedEquity(win, tie, share, count, status, samples)

    def equity_ranged_d(self, m=None, tables_d=None, observer=L.OBSERVER_ACTIVE, weights_d=None, num_ranges=0, range_of_d=None,
                        range_per_table=False, samples=1024, nonce=0, win_d=None, tie_d=None, share_d=None, accepted_d=None, status_d=None):
        """pk_table_equity_ranged_d: the same on device buffers (weights_d uint16 [num_ranges, 1326], range_of_d uint16 [N] or [m, N]; outputs
        uint32 [m, N] win / tie, uint64 [m, N] share, uint32 [m] accepted, uint8 [m] status; any may be None), asynchronous on the handle's
        stream.  m defaults to every table."""
        from .judger import check_samples
        o = self._range_observer(observer)
        samples, nonce = check_samples(samples, nonce)
        if not 0 <= int(num_ranges) <= L.EQW_MAX_RANGES:
            raise ValueError('at most %d ranges per call' % L.EQW_MAX_RANGES)
        m = self.num_tables if m is None else int(m)
        L.check(self._lib.pk_table_equity_ranged_d(self._h, self._dptr(tables_d), m, o, samples, nonce, self._dptr(weights_d), int(num_ranges),
                                                   self._dptr(range_of_d), int(bool(range_per_table)), self._dptr(win_d), self._dptr(tie_d),
                                                   self._dptr(share_d), self._dptr(accepted_d), self._dptr(status_d)), self._h)

    def ev_ranged(self, tables=None, observer=L.OBSERVER_ACTIVE, ranges=None, range_of=None, samples=1024, nonce=0):
        """Showdown EV in chips of `tables` (all tables if None; indices may repeat) as `observer` (a seat or OBSERVER_ACTIVE) sees them,
        where every other live seat draws its holding from a weighted range: the side pots of equity_ev over the attempts of equity_ranged
        (pk_table_ev_ranged; definition: pokerl_hip.h "Ranged showdown EV").  ranges, range_of, samples, nonce as equity_ranged; bets = bets +
        pending_bets as equity_ev.  Returns a judger.RangedEV of [m, N] / [m, N, N] / [m] arrays (`bets` and `payout` are None while
        asynchronous steps are in flight: they are formed from the getters)."""
        from .judger import NO_LEVEL, RangedEV, check_ranges, check_samples
        o = self._range_observer(observer)
        samples, nonce = check_samples(samples, nonce)
        t = self._tables(tables)
        m = self.num_tables if t is None else len(t)
        n = self.num_players
        w, r, ro, per = check_ranges(ranges, range_of, n, m)
        share = np.zeros((m, n, n), np.uint64)
        level_seat = np.full((m, n), NO_LEVEL, np.uint8)
        amount, ev = np.zeros((m, n), np.float64), np.zeros((m, n), np.float64)
        count, status = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
        L.check(self._lib.pk_table_ev_ranged(self._h, L.ptr(t), m, o, samples, nonce, L.ptr(w), r, L.ptr(ro), int(per), L.ptr(share),
                                             L.ptr(level_seat), L.ptr(amount), L.ptr(ev), L.ptr(count), L.ptr(status)), self._h)
        try:                            # (`bets` is formed from the getters, which refuse with PK_E_BUSY while asynchronous steps are in flight)
            bets = self.bets + self.pending_bets
            if t is not None:
                ok = (t >= 0) & (t < self.num_tables)
                bets = np.where(ok[:, None], bets[np.where(ok, t, 0)], 0.0)
        except L.PokerlHipError as e:
            if e.code != L.PK_E_BUSY:
                raise
            bets = None
        return RangedEV(ev, share, level_seat, amount, count, status, bets, samples)

    def ev_ranged_d(self, status_d, m=None, tables_d=None, observer=L.OBSERVER_ACTIVE, weights_d=None, num_ranges=0, range_of_d=None,
                    range_per_table=False, samples=1024, nonce=0, share_d=None, level_seat_d=None, amount_d=None, ev_d=None, accepted_d=None):
        """pk_table_ev_ranged_d: the same on device buffers (weights_d uint16 [num_ranges, 1326], range_of_d uint16 [N] or [m, N]; outputs
        uint64 [m, N, N] share, uint8 [m, N] level_seat, float64 [m, N] amount / ev, uint32 [m] accepted, uint8 [m] status; any but status_d
        may be None), asynchronous on the handle's stream.  m defaults to every table."""
        from .judger import check_samples
        o = self._range_observer(observer)
        samples, nonce = check_samples(samples, nonce)
        if not 0 <= int(num_ranges) <= L.EQW_MAX_RANGES:
            raise ValueError('at most %d ranges per call' % L.EQW_MAX_RANGES)
        if status_d is None:
            raise ValueError('status_d is required')
        m = self.num_tables if m is None else int(m)
        L.check(self._lib.pk_table_ev_ranged_d(self._h, self._dptr(tables_d), m, o, samples, nonce, self._dptr(weights_d), int(num_ranges),
                                               self._dptr(range_of_d), int(bool(range_per_table)), self._dptr(share_d), self._dptr(level_seat_d),
                                               self._dptr(amount_d), self._dptr(ev_d), self._dptr(accepted_d), self._dptr(status_d)), self._h)

    def _range_observer(self, observer):
        """observer of equity_range: a seat or OBSERVER_ACTIVE / 'active'; ValueError otherwise (before any call)."""
        o = self._observer(observer)
        if o != L.OBSERVER_ACTIVE and not (0 <= o < self.num_players):
            raise ValueError('observer must be a seat 0 .. %d or OBSERVER_ACTIVE' % (self.num_players - 1))
        return o

    def equity_range(self, observer='active', weights=None, tables=None, per_holding=False):
        """Exact hand strength of `observer` (a seat, or 'active' / OBSERVER_ACTIVE: each table's active seat) against ONE hidden hand at
        `tables` (all tables if None; indices may repeat), post-flop (pk_table_equity_range; definition: pokerl_hip.h "Range equity"): the
        observer's two cards and the board so far against every holding of the other cards, every completion of the board enumerated.
        weights: None (uniform), uint16 [1326] (one range) or [m, 1326] over judger.holding_index.  Returns a judger.RangeEquity: agg [m, 3]
        and `strength` [m] always, win / tie [m, 1326] and `valid` with per_holding=True (`valid` is None while asynchronous steps are in
        flight: it is formed from the getters).  A table that cannot be evaluated (pre-flop, never
        reset, step in flight) has a non-zero status and strength 0."""
        from .judger import RangeEquity, range_weights, valid_holdings
        o = self._range_observer(observer)
        t = self._tables(tables)
        m = self.num_tables if t is None else len(t)
        w, per_spot = range_weights(weights, m)
        win = np.zeros((m, L.EQ_HOLDINGS), np.uint32) if per_holding else None
        tie = np.zeros((m, L.EQ_HOLDINGS), np.uint32) if per_holding else None
        agg, boards, status = np.zeros((m, 3), np.uint64), np.zeros(m, np.uint32), np.zeros(m, np.uint8)
        L.check(self._lib.pk_table_equity_range(self._h, L.ptr(t), m, o, L.ptr(w), per_spot, L.ptr(agg), L.ptr(win), L.ptr(tie), L.ptr(boards),
                                                L.ptr(status)), self._h)
        valid = None
        if per_holding and not status.all():    # (from the getters, which refuse with PK_E_BUSY while asynchronous steps are in flight: no mask then)
            try:
                deck, turn, active = self.deck, self.turn, self.active_player
            except L.PokerlHipError as e:
                if e.code != L.PK_E_BUSY:       # (any other failure of a getter is the caller's to see)
                    raise
                deck = None
            if deck is not None:
                idx = np.arange(self.num_tables) if t is None else t
                sel = idx[status == 0]
                who = active[sel].astype(np.int64) if o == L.OBSERVER_ACTIVE else np.full(len(sel), o, np.int64)
                hero = np.stack([deck[sel, 5 + 2 * who], deck[sel, 6 + 2 * who]], axis=1)
                valid = np.zeros((m, L.EQ_HOLDINGS), bool)
                valid[status == 0] = valid_holdings(hero, deck[sel, :5], np.minimum(turn[sel] + 2, 5))
        elif per_holding:
            valid = np.zeros((m, L.EQ_HOLDINGS), bool)
        return RangeEquity(win, tie, boards, status, agg, valid)

    def equity_range_d(self, m=None, tables_d=None, observer='active', weights_d=None, weights_per_spot=False, agg_d=None, win_d=None, tie_d=None,
                       boards_d=None, status_d=None):
        """pk_table_equity_range_d: the same into device buffers (uint64 [m, 3] agg, uint32 [m, 1326] win / tie, uint32 [m] boards, uint8 [m]
        status; any may be None; weights_d uint16 [1326] or [m, 1326] or None), asynchronous on the handle's stream.  m defaults to every table."""
        o = self._range_observer(observer)
        m = self.num_tables if m is None else int(m)
        L.check(self._lib.pk_table_equity_range_d(self._h, self._dptr(tables_d), m, o, self._dptr(weights_d), int(bool(weights_per_spot)),
                                                  self._dptr(agg_d), self._dptr(win_d), self._dptr(tie_d), self._dptr(boards_d), self._dptr(status_d)),
                self._h)

    def equity_preflop(self, observer='active', weights=None, tables=None, per_holding=False):
        """Exact STARTING-HAND strength of `observer` (a seat, or 'active' / OBSERVER_ACTIVE: each table's active seat) against ONE hidden hand
        at `tables` (all tables if None; indices may repeat): the observer's two hole cards against every holding of the other fifty cards
        over every five-card board (pk_table_equity_preflop; definition: pokerl_hip.h "Pre-flop matchups").  The board is NOT read, at
        whatever turn a table rests: a caller who wants "pre-flop here, post-flop there" passes `tables` to this call and to equity_range.
        weights: None (uniform), uint16 [1326] (one range) or [m, 1326] over judger.holding_index.  Returns a judger.RangeEquity: agg [m, 3]
        and `strength` [m] always, win / tie [m, 1326] and `valid` with per_holding=True (`valid` is None while asynchronous steps are in
        flight: it is formed from the getters).  A table that cannot be evaluated (never reset, step in flight, index out of range) has a
        non-zero status and strength 0."""
        from .judger import RangeEquity, preflop_valid_holdings, range_weights
        o = self._range_observer(observer)
        t = self._tables(tables)
        m = self.num_tables if t is None else len(t)
        w, per_spot = range_weights(weights, m)
        win = np.zeros((m, L.EQ_HOLDINGS), np.uint32) if per_holding else None
        tie = np.zeros((m, L.EQ_HOLDINGS), np.uint32) if per_holding else None
        agg, boards, status = np.zeros((m, 3), np.uint64), np.zeros(m, np.uint32), np.zeros(m, np.uint8)
        L.check(self._lib.pk_table_equity_preflop(self._h, L.ptr(t), m, o, L.ptr(w), per_spot, L.ptr(agg), L.ptr(win), L.ptr(tie), L.ptr(boards),
                                                  L.ptr(status)), self._h)
        valid = None
        if per_holding and not status.all():    # (from the getters, which refuse with PK_E_BUSY while asynchronous steps are in flight: no mask then)
            try:
                deck, active = self.deck, self.active_player
            except L.PokerlHipError as e:
                if e.code != L.PK_E_BUSY:       # (any other failure of a getter is the caller's to see)
                    raise
                deck = None
            if deck is not None:
                idx = np.arange(self.num_tables) if t is None else t
                sel = idx[status == 0]
                who = active[sel].astype(np.int64) if o == L.OBSERVER_ACTIVE else np.full(len(sel), o, np.int64)
                valid = np.zeros((m, L.EQ_HOLDINGS), bool)
                valid[status == 0] = preflop_valid_holdings(np.stack([deck[sel, 5 + 2 * who], deck[sel, 6 + 2 * who]], axis=1))
        elif per_holding:
            valid = np.zeros((m, L.EQ_HOLDINGS), bool)
        return RangeEquity(win, tie, boards, status, agg, valid)

    def equity_preflop_d(self, m=None, tables_d=None, observer='active', weights_d=None, weights_per_spot=False, agg_d=None, win_d=None, tie_d=None,
                         boards_d=None, status_d=None):
        """pk_table_equity_preflop_d: the same into device buffers (uint64 [m, 3] agg, uint32 [m, 1326] win / tie, uint32 [m] boards, uint8 [m]
        status; any may be None; weights_d uint16 [1326] or [m, 1326] or None), asynchronous on the handle's stream.  m defaults to every table."""
        o = self._range_observer(observer)
        m = self.num_tables if m is None else int(m)
        L.check(self._lib.pk_table_equity_preflop_d(self._h, self._dptr(tables_d), m, o, self._dptr(weights_d), int(bool(weights_per_spot)),
                                                    self._dptr(agg_d), self._dptr(win_d), self._dptr(tie_d), self._dptr(boards_d), self._dptr(status_d)),
                self._h)

    def equity_rvr(self, weights=None, tables=None):
        """Range against range on the PUBLIC board of `tables` (all tables if None; indices may repeat), post-flop (pk_table_equity_rvr;
        definition: pokerl_hip.h "Range vs range"): for every holding the hero can have, the weight of the opponent's range it beats, ties
        and meets, every completion of the board enumerated.  No hole card is read.  weights: None (uniform), uint16 [1326] (one range) or
        [m, 1326] over judger.holding_index.  Returns a judger.RangeVsRange with uint64 [m, 1326] win / tie / tot (`valid` is None while
        asynchronous steps are in flight: it is formed from the getters).  A table that cannot be evaluated (pre-flop, step in flight) has a
        non-zero status and zeros."""
        from .judger import RangeVsRange, range_weights, rvr_valid_holdings
        t = self._tables(tables)
        m = self.num_tables if t is None else len(t)
        w, per_spot = range_weights(weights, m)
        win, tie, tot = (np.zeros((m, L.EQ_HOLDINGS), np.uint64) for _ in range(3))
        boards, status = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
        L.check(self._lib.pk_table_equity_rvr(self._h, L.ptr(t), m, L.ptr(w), per_spot, L.ptr(win), L.ptr(tie), L.ptr(tot), L.ptr(boards),
                                              L.ptr(status)), self._h)
        valid = np.zeros((m, L.EQ_HOLDINGS), bool)
        if not status.all():    # (from the getters, which refuse with PK_E_BUSY while asynchronous steps are in flight: no mask then)
            try:
                deck, turn = self.deck, self.turn
                idx = np.arange(self.num_tables) if t is None else t
                sel = idx[status == 0]
                valid[status == 0] = rvr_valid_holdings(deck[sel, :5], np.minimum(turn[sel] + 2, 5))
            except L.PokerlHipError as e:
                if e.code != L.PK_E_BUSY:       # (any other failure of a getter is the caller's to see)
                    raise
                valid = None
        return RangeVsRange(win, tie, tot, boards, status, valid)

    def equity_rvr_d(self, m=None, tables_d=None, weights_d=None, weights_per_spot=False, win_d=None, tie_d=None, tot_d=None, boards_d=None,
                     status_d=None):
        """pk_table_equity_rvr_d: the same into device buffers (uint64 [m, 1326] win / tie / tot, uint32 [m] boards, uint8 [m] status; any may
        be None; weights_d uint16 [1326] or [m, 1326] or None), asynchronous on the handle's stream.  m defaults to every table."""
        m = self.num_tables if m is None else int(m)
        L.check(self._lib.pk_table_equity_rvr_d(self._h, self._dptr(tables_d), m, self._dptr(weights_d), int(bool(weights_per_spot)),
                                                self._dptr(win_d), self._dptr(tie_d), self._dptr(tot_d), self._dptr(boards_d), self._dptr(status_d)),
                self._h)

    def equity_hist(self, weights=None, tables=None, bins=10):
        """Strength histograms on the PUBLIC board of `tables` (all tables if None; indices may repeat), post-flop (pk_table_equity_hist;
        definition: pokerl_hip.h "Strength histograms"): for every holding the hero can have, the distribution of its river strength against
        the opponent's range over the completions of the board, in `bins` (1 .. 32) equal parts of [0, 1].  No hole card is read.  weights:
        None (uniform), uint16 [1326] (one range) or [m, 1326] over judger.holding_index.  Returns a judger.StrengthHistogram with uint16
        [m, 1326, bins] hist and [m, 1326] void (`valid` is None while asynchronous steps are in flight: it is formed from the getters).  A
        table that cannot be evaluated (pre-flop, step in flight) has a non-zero status and zeros."""
        from .judger import StrengthHistogram, check_bins, range_weights, rvr_valid_holdings
        bins = check_bins(bins)
        t = self._tables(tables)
        m = self.num_tables if t is None else len(t)
        w, per_spot = range_weights(weights, m)
        hist, void = np.zeros((m, L.EQ_HOLDINGS, bins), np.uint16), np.zeros((m, L.EQ_HOLDINGS), np.uint16)
        completions, status = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
        L.check(self._lib.pk_table_equity_hist(self._h, L.ptr(t), m, L.ptr(w), per_spot, bins, L.ptr(hist), L.ptr(void), L.ptr(completions),
                                               L.ptr(status)), self._h)
        valid = np.zeros((m, L.EQ_HOLDINGS), bool)
        if not status.all():    # (from the getters, which refuse with PK_E_BUSY while asynchronous steps are in flight: no mask then)
            try:
                deck, turn = self.deck, self.turn
                idx = np.arange(self.num_tables) if t is None else t
                sel = idx[status == 0]
                valid[status == 0] = rvr_valid_holdings(deck[sel, :5], np.minimum(turn[sel] + 2, 5))
            except L.PokerlHipError as e:
                if e.code != L.PK_E_BUSY:       # (any other failure of a getter is the caller's to see)
                    raise
                valid = None
        return StrengthHistogram(hist, void, completions, status, valid)

    def equity_hist_d(self, m=None, tables_d=None, weights_d=None, weights_per_spot=False, bins=10, hist_d=None, void_d=None, completions_d=None,
                      status_d=None):
        """pk_table_equity_hist_d: the same into device buffers (uint16 [m, 1326, bins] hist, uint16 [m, 1326] void, uint32 [m] completions,
        uint8 [m] status; any may be None; weights_d uint16 [1326] or [m, 1326] or None), asynchronous on the handle's stream.  m defaults
        to every table."""
        from .judger import check_bins
        m = self.num_tables if m is None else int(m)
        L.check(self._lib.pk_table_equity_hist_d(self._h, self._dptr(tables_d), m, self._dptr(weights_d), int(bool(weights_per_spot)),
                                                 check_bins(bins), self._dptr(hist_d), self._dptr(void_d), self._dptr(completions_d),
                                                 self._dptr(status_d)), self._h)

    def equity_hist_hero(self, observer='active', weights=None, tables=None, bins=10, centroids=None):
        """The strength histogram of ONE seat's holding at `tables` (all tables if None; indices may repeat), post-flop
        (pk_table_equity_hist_hero; definition: pokerl_hip.h "Hero strength histogram"): the distribution of the river strength of
        `observer` (a seat, or 'active' / OBSERVER_ACTIVE: each table's active seat) against the opponent's range over the completions of
        the board, in `bins` (1 .. 32) equal parts of [0, 1] -- the row of equity_hist for that seat's hand, at the cost of equity_range.
        weights: None (uniform), uint16 [1326] (one range) or [m, 1326] over judger.holding_index.  centroids: None, or uint16 [k, bins]
        (cluster_histograms(...).centroids): the result then carries each table's bucket `label` and `dist` from the same call.  Returns a
        judger.HeroHistogram with uint16 [m, bins] hist.  A table that cannot be evaluated (pre-flop, never reset, step in flight) has a
        non-zero status, zeros, and label PK_CL_NONE."""
        from .judger import HeroHistogram, hero_bucket_args, range_weights
        o = self._range_observer(observer)
        t = self._tables(tables)
        m = self.num_tables if t is None else len(t)
        w, per_spot = range_weights(weights, m)
        bins, cen, k, label, dist = hero_bucket_args(bins, centroids, m)
        hist, void = np.zeros((m, bins), np.uint16), np.zeros(m, np.uint16)
        completions, status = np.zeros(m, np.uint32), np.zeros(m, np.uint8)
        L.check(self._lib.pk_table_equity_hist_hero(self._h, L.ptr(t), m, o, L.ptr(w), per_spot, bins, L.ptr(hist), L.ptr(void), L.ptr(completions),
                                                    L.ptr(status), k, L.ptr(cen), L.ptr(label), L.ptr(dist)), self._h)
        return HeroHistogram(hist, void, completions, status, label, dist)

    def equity_hist_hero_d(self, m=None, tables_d=None, observer='active', weights_d=None, weights_per_spot=False, bins=10, hist_d=None, void_d=None,
                           completions_d=None, status_d=None, k=0, centroids_d=None, label_d=None, dist_d=None):
        """pk_table_equity_hist_hero_d: the same into device buffers (uint16 [m, bins] hist, uint16 [m] void, uint32 [m] completions, uint8
        [m] status, and with k > 0 and centroids_d uint16 [k, bins]: uint16 [m] label, uint32 [m] dist; any output may be None; weights_d
        uint16 [1326] or [m, 1326] or None), asynchronous on the handle's stream.  m defaults to every table."""
        from .judger import _cl_int, check_bins
        o = self._range_observer(observer)
        m = self.num_tables if m is None else int(m)
        k = _cl_int('k', k, 0, L.CL_MAX_K)
        if k and centroids_d is None:
            raise ValueError('k > 0 needs centroids_d')
        if not k and (label_d is not None or dist_d is not None):
            raise ValueError('label_d / dist_d need k > 0 and centroids_d')
        L.check(self._lib.pk_table_equity_hist_hero_d(self._h, self._dptr(tables_d), m, o, self._dptr(weights_d), int(bool(weights_per_spot)),
                                                      check_bins(bins), self._dptr(hist_d), self._dptr(void_d), self._dptr(completions_d),
                                                      self._dptr(status_d), k, self._dptr(centroids_d), self._dptr(label_d), self._dptr(dist_d)),
                self._h)

    def bucket(self, centroids, observer='active', weights=None, tables=None):
        """The bucket of `observer`'s hand at `tables` -> uint16 [m]: the label of equity_hist_hero(..., bins=centroids.shape[1],
        centroids=centroids), asked for alone (the histograms stay on the device).  PK_CL_NONE (0xFFFF) where a table cannot be evaluated."""
        from .judger import hero_bucket_args, range_weights
        o = self._range_observer(observer)
        t = self._tables(tables)
        m = self.num_tables if t is None else len(t)
        w, per_spot = range_weights(weights, m)
        if centroids is None or np.ndim(centroids) != 2:
            raise ValueError('centroids must have shape [k, bins]')
        bins, cen, k, label, _ = hero_bucket_args(int(np.shape(centroids)[1]), centroids, m)
        L.check(self._lib.pk_table_equity_hist_hero(self._h, L.ptr(t), m, o, L.ptr(w), per_spot, bins, None, None, None, None, k, L.ptr(cen),
                                                    L.ptr(label), None), self._h)
        return label

    def __deepcopy__(self, memo):
        """A new handle with the same configuration (seed and table ids included) holding a copy of every table: it continues
        bit-identically to this game under the same actions, and stepping one leaves the other untouched.  Only the construction
        config and the tables are copied (also by pickle): runtime settings of this handle -- its stream (set_stream), coalescing,
        tuning, env sub-batches, set_step_obs / packed-observation buffers -- start at their defaults in the copy."""
        g = VecGame(self.num_tables, **self._config())
        g.load(self.save())
        return g

    def __getstate__(self):
        return dict(num_tables=self.num_tables, config=self._config(), blob=self.save())

    def __setstate__(self, state):
        """Unpickling creates a handle on the pickled `device` and loads the tables."""
        self.__init__(state['num_tables'], **state['config'])
        self.load(state['blob'])

    # ------------------------------------------------------------------ state reads (Game attributes)
    def _f64(self, field):
        out = np.zeros((self.num_tables, self.num_players), np.float64)
        L.check(self._lib.pk_get_f64(self._h, field, L.ptr(out)), self._h)
        return out

    def _i32(self, field):
        out = np.zeros(self.num_tables, np.int32)
        L.check(self._lib.pk_get_i32(self._h, field, L.ptr(out)), self._h)
        return out

    credits = property(lambda self: self._f64(L.F_CREDITS))
    bets = property(lambda self: self._f64(L.F_BETS))
    pending_bets = property(lambda self: self._f64(L.F_PENDING_BETS))
    payoffs = property(lambda self: self._f64(L.F_PAYOFFS))
    active_player = property(lambda self: self._i32(L.I_ACTIVE_PLAYER))
    turn = property(lambda self: self._i32(L.I_TURN))
    dealer_idx = property(lambda self: self._i32(L.I_DEALER_IDX))
    small_blind_idx = property(lambda self: self._i32(L.I_SMALL_BLIND_IDX))
    big_blind_idx = property(lambda self: self._i32(L.I_BIG_BLIND_IDX))
    hand = property(lambda self: self._i32(L.I_HAND))

    def _table_f64(self, field):
        out = np.zeros(self.num_tables, np.float64)
        L.check(self._lib.pk_get_table_f64(self._h, field, L.ptr(out)), self._h)
        return out

    minimum_raise_value = property(lambda self: self._table_f64(L.TF_MIN_RAISE))
    pot = property(lambda self: self._table_f64(L.TF_POT))            # game.py:281-284, np.sum order kept on the device
    high_bet = property(lambda self: self._table_f64(L.TF_HIGH_BET))  # game.py:287-290

    @property
    def player_states(self):
        out = np.zeros((self.num_tables, self.num_players), np.uint8)
        L.check(self._lib.pk_get_player_states(self._h, L.ptr(out)), self._h)
        return out

    @property
    def deck(self):
        """deck[:, 0:5+2N] as Card.value bytes -- the only part of the deck the game ever reads (game.py:278,385-395)."""
        out = np.zeros((self.num_tables, 5 + 2 * self.num_players), np.uint8)
        L.check(self._lib.pk_get_cards(self._h, L.ptr(out)), self._h)
        return out

    @property
    def community_cards(self):
        """[T,5] card values, -1 where not yet visible (game.py:266-278: [] at turn 0, deck[:turn+2] after)."""
        cards = self.deck[:, :5].astype(np.int16)
        turn = self.turn
        visible = (turn[:, None] != 0) & (np.arange(5)[None, :] < (turn[:, None] + 2))
        cards[~visible] = -1
        return cards

    def get_cards_of(self, player):
        """game.py:385-389.  player: int or int array [T]."""
        p = np.broadcast_to(np.asarray(player), (self.num_tables,))
        d = self.deck
        t = np.arange(self.num_tables)
        return np.stack([d[t, 5 + 2 * p], d[t, 6 + 2 * p]], axis=1)

    def get_hand_for(self, player):
        """game.py:391-395: the 5 community cards + the player's 2 hole cards, [T,7]."""
        return np.concatenate([self.deck[:, :5], self.get_cards_of(player)], axis=1)

    @property
    def hand_rankings(self):
        """Rankings of each table's last showdown (game.py:488-489): (rank [T,N] HandRanking, kickers value [T,N])."""
        rank = np.zeros((self.num_tables, self.num_players), np.uint8)
        kick = np.zeros((self.num_tables, self.num_players), np.uint32)
        L.check(self._lib.pk_get_hand_ranks(self._h, L.ptr(rank), L.ptr(kick)), self._h)
        return rank, kick

    @property
    def game_over(self):
        out = np.zeros(self.num_tables, np.uint8)                     # game.py:317-320
        L.check(self._lib.pk_get_game_over(self._h, L.ptr(out)), self._h)
        return out != 0

    def observations_of(self, player=None, out=None):
        """Dense `StateView(game, player)` rows (game.py:117-131), f64 [T, PK_OBS_DIM(N)]; layout in pokerl_hip.h.
        player=None or 0: each table's active player (`player or game.active_player`, game.py:122).
        out: a C-contiguous f64 [T, PK_OBS_DIM] array to fill (a pinned one -- pokerl_amd.pinned_empty -- copies at PCIe rate)."""
        seat = -1 if not player else self._seat(player)
        shape = (self.num_tables, 17 + 3 * self.num_players)
        if out is None:
            out = np.empty(shape, np.float64)
        elif out.shape != shape or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError('out must be a C-contiguous f64 array of shape %s' % (shape,))
        L.check(self._lib.pk_get_obs(self._h, seat, L.ptr(out)), self._h)
        return out

    def observations_packed_of(self, player=None, out=None):
        """The same rows in the compact form (pk_get_obs_packed: 16 header bytes + (3N+1) f64 per table, 168 B against 280 at six
        seats) as a structured array [T] of state_view.packed_dtype(N); state_view.unpack_obs() gives the dense rows back."""
        from .state_view import packed_dtype
        seat = -1 if not player else self._seat(player)
        dt = packed_dtype(self.num_players)
        if out is None:
            out = np.empty(self.num_tables, dt)
        elif out.shape != (self.num_tables,) or out.dtype != dt or not out.flags.c_contiguous:
            raise ValueError('out must be a C-contiguous array of packed_dtype(N) with one row per table')
        L.check(self._lib.pk_get_obs_packed(self._h, seat, L.ptr(out)), self._h)
        return out

    observations = property(lambda self: self.observations_of(None))

    def state_views(self, player=None):
        """One `StateView` (the reference's observation object, game.py:39-240) per table, for host-side policies."""
        from .state_view import StateView
        return [StateView(row, self.num_players) for row in self.observations_of(player)]

    def state_view(self, table=0, player=None):
        from .state_view import StateView
        return StateView(self.observations_of(player)[table], self.num_players)

    active_state = observations
