"""Shared comparison drivers (TEST INFRASTRUCTURE): every table-kernel family against the CPU oracle, for one configuration at a time.

One copy of each loop: tests/test_hip_seat_matrix.py runs them at every seat count 2 .. 16, tests/test_seat_matrix_host.py runs their
oracle halves without a GPU (caps, content, comparators), and tools/fuzz_*.py run them over seeded odd configurations.  The oracle
halves (`*_trace`, `*_want`, the comparators, `oracle_rows`) need numpy and oracle/ only; the device halves import pokerl_amd when called.
Every comparison is bit-exact: bytes of every f64, every state byte (golden_util.assert_snap), per-table delivered sequences."""
import numpy as np

import golden_util as GU
from oracle import loader as O
from oracle import rng_spec as R

SEATS = list(range(2, 17))
T_MATRIX = 165                 # 64 + 64 + 37 lanes ONLY at 64 tables per wave (shape "full"); pk_create's own choice at this size is one table per wave
T_BATCHES = 3 * 64 + 5         # B = 2 sub-batches: a range is whole 64-table blocks (batch_ranges)
CAPS = O.ERR_HAND_CAP | O.ERR_ENV_CAP
PS_BROKEN = 4
KINDS = ("default", "ladder", "top_seat")
RESUMED = "resumed"            # the fourth configuration: default, with the RNG streams resumed just below 2^32 (matrix_config)
DEEP = "deep"                  # the fifth configuration: the never-fold caller of rng_spec.py (POLICY_DEEP) on per-seat fractional stacks (matrix_config)
ALL_KINDS = KINDS + (RESUMED, DEEP)
DEEP_SHAPE_SEATS = (2, 6, 9, 13, 16)             # seat counts at which the deep game_step / env_step cases also run under `spread` and `part`
RESUMED_SEATS = (2, 6, 9, 13, 16)
RESUMED_SERIALS = (2 ** 32 - 2, 2 ** 35 - 5)     # (hand_serial, step_serial): the action-block index step_serial >> 3 is 2^32 - 1
# How pk_create lays the tables out over wavefronts (PK_TPB; None: its own rule, tpb_rule).  spread: what a caller gets -- one table per wave at
# the matrix's sizes.  full: waves of 64, 64 and 37 live lanes.  part: twenty waves of 8 live lanes and one of 5, lanes >= 8 dead inside the wave --
# the shape every caller between 1 025 and 32 768 tables gets.
WAVE_SHAPES = {"spread": None, "full": 64, "part": 8}
# steps per family in the matrix (a case is to take a few seconds); tests/test_seat_matrix_host.py checks the caps at the same budgets
K_GAME, K_ENV, K_MULTI, K_PLAYED = 40, 15, 15, 40
K_ROLLOUT = 48                 # the fused rollout family: launches of 16, 25 and 7 steps -- the first two long enough for k_rollout_tab / k_rollout_allin_tab
K_DEEP_GAME = 60               # lockstep steps of the deep configuration's game_step families
K_DEEP = 30                    # lockstep deep steps before the rollout_from_deep, snapshot and equity families take over
BUDGETS = (1, 3)               # hand ends / Game.steps per launch of the bounded forms


def k_call(N):
    """Steps of the call-agent rollout: a hand of calling stations lasts four rounds of N calls."""
    return max(40, 6 * N)


def k_of(family, kind, N):
    """Steps of `family` (a driver's name) in configuration `kind`.  The resumed configuration needs three tables in four to end two hands
    inside the run, so that hand_serial 2^32 is dealt; tests/test_seat_matrix_host.py holds the oracle half to that at these very K, and they
    suffice as they are (random agents end a hand within a few steps) -- a family that missed it would get a longer K for RESUMED here."""
    if kind == DEEP:
        # game_step: long enough for 40 river hand ends among three or more seats and 40 hands that pay three or more amounts at every seat
        # count (the pre-flight's floors).  env_step: PokerGameEnv.step never returns for a seat 0 that goes broke while an opponent's step
        # ends the hand with two or more call agents left (game_env.py:49-52; the product ends it with PK_TERR_ENV_CAP after 8 192 steps), and
        # from eight seats on the first such step comes after six env.steps of the deep configuration's tables.
        return {"game_step": K_DEEP_GAME, "game_step_async": K_DEEP_GAME, "env_step": K_ENV if N <= 7 else 6,
                "played": K_DEEP, "rollout": K_ROLLOUT}[family]
    return {"game_step": K_GAME, "game_step_async": K_GAME, "env_step": K_ENV, "rollout": K_ROLLOUT, "rollout_call": k_call(N)}[family]


# ------------------------------------------------------------------ wave shapes
def tpb_rule(T):
    """Tables per wavefront as pk_create picks them without a knob (include/pokerl_hip.h, pk_get_wave_shape), restated: 64 halved while the
    batch fits 1 024 waves of half as many -- 1 up to 1 024 tables, 64 only above 32 768."""
    tpb = 64
    while tpb > 1 and T <= 1024 * (tpb // 2):
        tpb //= 2
    return tpb


def use_shape(monkeypatch, shape):
    """Sets the environment a handle created from now on reads its wave shape from; PK_ENV_TPB goes, so that the env kernels follow PK_TPB."""
    if WAVE_SHAPES[shape] is None:
        monkeypatch.delenv("PK_TPB", raising=False)
    else:
        monkeypatch.setenv("PK_TPB", str(WAVE_SHAPES[shape]))
    monkeypatch.delenv("PK_ENV_TPB", raising=False)


def shape_demand(cfg):
    """(tables per wave, ... of the env kernels) that cfg's shape demands of every handle made for it."""
    tpb = WAVE_SHAPES[cfg["shape"]] or tpb_rule(cfg["T"])
    return tpb, tpb


def assert_shape(g, cfg):
    """Every handle a driver makes: the shape the case names is the shape that runs (a case must not silently run one table per wave).
    Configurations that name no shape (the fuzz tools') claim none."""
    if cfg.get("shape") is not None:
        assert g.wave_shape == shape_demand(cfg), (where_of(cfg), "wave shape", g.wave_shape, shape_demand(cfg))
    return g


def batch_ranges(T, B):
    """The contiguous table ranges pk_set_env_batches(h, B) cuts T tables into, by the rule its header states: ceil(T / B) tables rounded up
    to whole 64-table blocks per range, as many ranges as that takes (fewer than B for a small batch)."""
    size = -(-(-(-T // B)) // 64) * 64
    return [(b, min(b + size, T)) for b in range(0, T, size)]


# ------------------------------------------------------------------ configurations
def matrix_config(kind, N, T=T_MATRIX, shape="spread"):
    """The matrix's configurations at N seats.  default: stacks 100, blinds 2 / 1, random agents.  ladder: per-seat stacks 5 (p + 1),
    all-in agents, first dealer N - 1 -- every hand an N-way showdown with up to N - 1 side-pot levels.  top_seat: table ids that wrap
    inside the batch, and seat N - 1 wherever a family takes a seat.  resumed: default with the serials set to RESUMED_SERIALS before the
    first reset -- that reset deals hand_serial 2^32 - 2, the first hand end 2^32 - 1 (a lone table's stock of four decks then spans the
    carry into the high counter word), the second 2^32; the action-block index crosses 2^32 after five Game.steps.
    deep: per-seat stacks 7.5 (p + 1) + 0.25 (p % 3), the never-fold caller POLICY_DEEP (test infrastructure: the device is handed the
    oracle's actions wherever another configuration lets it pick), first dealer N - 1, table ids that wrap inside the batch -- raises on
    every street, short stacks all-in on different streets, multi-way river showdowns that pay several different amounts.
    `shape`: the wave shape the drivers demand of every handle (WAVE_SHAPES; the caller sets it with use_shape)."""
    cfg = dict(kind=kind, T=T, N=N, start=100, bb=2, sb=1, seed=0x5EA7 * 1000003 + 7919 * N + ALL_KINDS.index(kind), base=0, dealer=0, policy=0, top=None,
               shape=shape, serials=None)
    if kind == "ladder":
        cfg.update(start=[5.0 * (p + 1) for p in range(N)], policy=1, dealer=N - 1)
    elif kind == "top_seat":
        cfg.update(base=2 ** 32 - 100, top=N - 1)
    elif kind == RESUMED:
        cfg.update(serials=RESUMED_SERIALS)
    elif kind == DEEP:
        cfg.update(start=deep_stacks(N), policy=R.POLICY_DEEP, dealer=N - 1, base=2 ** 32 - 100)
    elif kind != "default":
        raise ValueError(kind)
    return cfg


def deep_stacks(N):
    return [7.5 * (p + 1) + 0.25 * (p % 3) for p in range(N)]


def env_config(kind, N, T=T_MATRIX, shape="spread"):
    """matrix_config for the env families.  deep: the same stacks dealt in REVERSE seat order, seat 0 the deepest -- with seat 0 the
    shortest stack against call agents it is broke within three env.steps at eight or more seats, which the env never returns from
    (k_of); the deepest seat lasts six."""
    cfg = matrix_config(kind, N, T, shape)
    if kind == DEEP:
        cfg["start"] = cfg["start"][::-1]
    return cfg


def is_deep(cfg):
    return cfg["policy"] == R.POLICY_DEEP


def device_picks(g, buf, cfg, a):
    """The actions of this step in a device buffer: the in-kernel agent's own pick, or -- the deep caller is no product policy -- the oracle's."""
    if is_deep(cfg):
        buf.upload(np.ascontiguousarray(a, np.int32))
    else:
        g.pick_actions_d(buf, cfg["policy"])


def multi_seats(cfg):
    """(policy per opponent seat, caller-played seats) of the multi-agent family.  top_seat: the top seat shoves and is played by the
    caller, seat 1 plays random -- a different policy in the top nibble (bits 60 .. 63 at 16 seats) than in nibble 1."""
    N = cfg["N"]
    if cfg["kind"] == "ladder":
        return [1] * (N - 1), list(range(1, N, 2))
    pols = [0] * (N - 1)
    if cfg["kind"] == "top_seat":
        pols[N - 2] = 1
        return pols, sorted({1, N - 1} if N > 2 else {1})
    return pols, list(range(2, N, 3)) or [1]


def deep_multi_seats(N, mixed):
    """(policy per opponent seat, caller-played seats) of the deep configuration's multi-agent cases: every seat the deep caller, played by
    the CALLER (the product knows no such policy; the oracle plays nibble 14) -- or, `mixed`, in-kernel call agents at the odd seats, from
    eight seats on at seat 1 alone: two call agents left over by the deep seats, with seat 0 broke, never end their game (k_of)."""
    pols = [2 if mixed and s % 2 and (N <= 7 or s == 1) else R.POLICY_DEEP for s in range(1, N)]
    return pols, [s for s in range(1, N) if pols[s - 1] == R.POLICY_DEEP]


def in_kernel_seats(cfg):
    """Per-seat IN-KERNEL policies (no caller-played seat): top nibble all-in, nibble 1 random, the call agent in between at seat 2."""
    N = cfg["N"]
    pols = [0] * (N - 1)
    pols[N - 2] = 1
    if N > 3:
        pols[1] = 2
    return pols


def where_of(cfg, what=""):
    return "%s N=%d T=%d %s%s" % (cfg["kind"] if "kind" in cfg else "cfg", cfg["N"], cfg["T"], "shape=%s " % cfg["shape"] if cfg.get("shape") else "", what)


def oracle_of(cfg):
    o = O.OracleGame(cfg["T"], cfg["N"], cfg["start"], cfg["bb"], cfg["sb"], seed=cfg["seed"], table_id_base=cfg["base"])
    if cfg.get("serials"):
        o.set_serials(*cfg["serials"])
    return o


def backend_of(HB, cfg):
    h = HB(cfg["T"], cfg["N"], cfg["start"], cfg["bb"], cfg["sb"], seed=cfg["seed"], table_id_base=cfg["base"])
    assert_shape(h.g, cfg)
    if cfg.get("serials"):
        h.set_serials(*cfg["serials"])
    return h


def env_of(agents, cfg):
    """A VecPokerGameEnv of cfg's tables (opponents: one policy or a list of agents), its shape asserted, its serials set before the first reset."""
    import pokerl_amd
    env = pokerl_amd.VecPokerGameEnv(agents, **env_kwargs(cfg))
    assert_shape(env.game, cfg)
    if cfg.get("serials"):
        env.game.set_serials(*cfg["serials"])
    return env


def crossed(snap0, snap1):
    """A resumed run between two oracle snapshots: (every table's action-block index step_serial >> 3 starts below 2^32 and ends at or above
    it, the number of tables whose hand_serial ends above 2^32 -- the deal of serial 2^32 itself has happened there)."""
    b0, b1 = np.asarray(snap0["step_serial"], np.uint64) >> np.uint64(3), np.asarray(snap1["step_serial"], np.uint64) >> np.uint64(3)
    return bool((b0 < 2 ** 32).all() and (b1 >= 2 ** 32).all() and (np.asarray(snap0["hand_serial"], np.uint64) < 2 ** 32).all()), \
        int((np.asarray(snap1["hand_serial"], np.uint64) > 2 ** 32).sum())


def env_kwargs(cfg):
    return dict(num_tables=cfg["T"], num_players=cfg["N"], start_credits=cfg["start"], big_blind=cfg["bb"], small_blind=cfg["sb"],
                seed=cfg["seed"], table_id_base=cfg["base"])


# ------------------------------------------------------------------ observation rows from the oracle's state, and the comparators
def oracle_rows(snap, N):
    """Game.StateView(player to act) (game.py:117-131) of every table of an oracle snapshot: the dense f64 rows [T, 17 + 3N] and the packed
    rows [T, 16 + 8 (3N + 1)] bytes (include/pokerl_hip.h PK_OBS_DIM / PK_OBS_PACKED_BYTES), restated here from the field lists."""
    T = len(snap["active"])
    a, turn, ar = snap["active"].astype(np.int64), snap["turn"].astype(np.int64), np.arange(T)
    cards = np.asarray(snap["cards"])
    dense = np.empty((T, 17 + 3 * N), np.float64)
    dense[:, 0], dense[:, 1], dense[:, 2] = a, turn, snap["min_raise"]
    dense[:, 3:10] = (snap["valid"].astype(np.int64)[:, None] >> np.arange(7)) & 1
    dense[:, 10], dense[:, 11] = cards[ar, 5 + 2 * a], cards[ar, 6 + 2 * a]
    vis = (turn[:, None] != 0) & (np.arange(5)[None, :] < turn[:, None] + 2)               # game.py:266-278
    dense[:, 12:17] = np.where(vis, cards[:, :5].astype(np.float64), -1.0)
    dense[:, 17:17 + N], dense[:, 17 + N:17 + 2 * N], dense[:, 17 + 2 * N:] = snap["credits"], snap["bets"], snap["pending"]
    packed = np.zeros((T, 16 + 8 * (3 * N + 1)), np.uint8)
    packed[:, 0], packed[:, 1], packed[:, 2] = a, turn, snap["valid"] & 0x7f
    packed[:, 3], packed[:, 4] = cards[ar, 5 + 2 * a], cards[ar, 6 + 2 * a]
    packed[:, 5:10] = np.where(vis, cards[:, :5], 0xFF)
    packed[:, 16:] = np.ascontiguousarray(np.concatenate([dense[:, 2:3], dense[:, 17:]], axis=1)).view(np.uint8)
    return dense, packed


def _first_bad(bad):
    return np.nonzero(bad)[0][:4].tolist(), int(bad.sum())


def assert_rows(dense, packed, want_dense, want_packed, mask, where):
    """The rows a kernel wrote (either may be None) against oracle_rows', bit for bit, for the tables in `mask`."""
    if dense is not None:
        bad = mask & (np.ascontiguousarray(dense).view(np.uint64) != np.ascontiguousarray(want_dense).view(np.uint64)).any(axis=1)
        if bad.any():
            t = int(np.argmax(bad))
            col = int(np.argmax(dense[t].view(np.uint64) != want_dense[t].view(np.uint64)))
            raise AssertionError("%s: dense row differs at tables %s (%d), first at element %d: oracle %r got %r"
                                 % ((where,) + _first_bad(bad) + (col, want_dense[t, col], dense[t, col])))
    if packed is not None:
        bad = mask & (packed != want_packed).any(axis=1)
        if bad.any():
            t = int(np.argmax(bad))
            col = int(np.argmax(packed[t] != want_packed[t]))
            raise AssertionError("%s: packed row differs at tables %s (%d), first at byte %d: oracle %d got %d"
                                 % ((where,) + _first_bad(bad) + (col, want_packed[t, col], packed[t, col])))
    return int(mask.sum()) * ((dense is not None) + (packed is not None))


DELIVERED = ("reward", "done", "hand", "terr", "obs")


def assert_delivered(got, want, where):
    """What an env call delivered for some tables -- (reward f64, done, hand, terr[, obs rows]) -- against what the oracle (or the synchronous
    call) returned for the same steps of the same tables, bit for bit."""
    assert len(got) == len(want), where
    for name, x, y in zip(DELIVERED, got, want):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape, (where, name, x.shape, y.shape)
        if x.dtype == np.float64 or y.dtype == np.float64:
            bad = np.ascontiguousarray(x, np.float64).view(np.uint64) != np.ascontiguousarray(y, np.float64).view(np.uint64)
        else:
            bad = x.astype(np.int64) != y.astype(np.int64)
        if bad.any():
            i = tuple(np.argwhere(bad)[0])
            raise AssertionError("%s: delivered %s differs at %d places, first at %s: want %r got %r" % (where, name, int(bad.sum()), list(i), y[i], x[i]))


def assert_flags(fl, te, fo, eo, auto, where):
    """Flags / terr of a Game.step call against the oracle's; with the reset inside the launch GAME_OVER also stands for a capped step."""
    over = ((fo & 1) | ((eo & 4) >> 2)).astype(np.uint8)
    exp = ((fo & 6) | over).astype(np.uint8) if auto else fo
    bad = (fl != exp) | (te != eo)
    if bad.any():
        t = int(np.argmax(bad))
        raise AssertionError("%s: flags / terr differ at tables %s (%d): oracle (%d, %d) got (%d, %d)" % ((where,) + _first_bad(bad) + (exp[t], eo[t], fl[t], te[t])))


def over_of(fo, eo):
    """Game over, or a step the reference would never leave (PK_TERR_HAND_CAP): what a reset inside the launch resets."""
    return ((fo & 1) | ((eo & 4) >> 2)).astype(np.uint8)


# ------------------------------------------------------------------ 1. lockstep Game.step
def game_step_trace(cfg, K, before=False):
    """The oracle's half of game_step: yields per step the actions, flags, terr, the reset mask, the rows before any reset (what
    pk_step_d leaves) and after the reset of finished games (what pk_step_auto_d leaves), both snapshots, and the oracle itself."""
    o = oracle_of(cfg)
    o.reset(dealer=cfg["dealer"])
    N = cfg["N"]
    for s in range(K):
        a = o.pick_actions(cfg["policy"])
        was = o.snapshot() if before else None
        fo, eo = o.step(a)
        over = over_of(fo, eo)
        pre = o.snapshot()
        if over.any():
            o.reset(mask=over)
        post = o.snapshot() if over.any() else pre
        if (eo & 2).any():                            # game.py:473: the table stays as it is; the caller resets it
            o.reset(mask=((eo & 2) != 0).astype(np.uint8))
        yield dict(s=s, a=a, fo=fo, eo=eo, over=over, was=was, pre=pre, post=post, rows=oracle_rows(pre, N), rows_auto=oracle_rows(post, N), o=o)


def oracle_views(snap):
    """VecGame.pot / high_bet / game_over (game.py:281-320) in numpy on an oracle snapshot: np.sum per table (numpy's own association
    order: pairwise blocks of eight from eight seats on, two of them at sixteen), the largest pending bet, one seat left that is not broke."""
    bets, pend = np.ascontiguousarray(snap["bets"], np.float64), np.ascontiguousarray(snap["pending"], np.float64)
    return np.array([np.sum(b) for b in bets]), np.max(pend, axis=1), (np.asarray(snap["states"]) != PS_BROKEN).sum(axis=1) == 1


def assert_views(g, snap, where):
    """The handle's pot / high_bet / game_over getters against oracle_views, bit for bit.  Returns the number of values compared."""
    pot, high, over = oracle_views(snap)
    for name, got, want in (("pot", g.pot, pot), ("high_bet", g.high_bet, high)):
        bad = np.ascontiguousarray(got, np.float64).view(np.uint64) != want.view(np.uint64)
        if bad.any():
            t = int(np.argmax(bad))
            raise AssertionError("%s: %s differs at tables %s (%d): oracle %r got %r" % ((where, name) + _first_bad(bad) + (want[t], got[t])))
    bad = np.asarray(g.game_over).astype(bool) != over
    if bad.any():
        raise AssertionError("%s: game_over differs at tables %s (%d)" % ((where,) + _first_bad(bad)))
    return 3 * len(pot)


def game_step(HB, cfg, K, snap_every=40, views_every=1):
    """Game.step with the caller's actions in its three complete forms, each on a handle of its own, against the oracle's step + reset: the
    host form (pk_step + pk_reset), pk_step_d + pk_reset_d(flags, GAME_OVER), and pk_step_auto_d (the reset inside the step's launch).  The
    step kernels write the StateView row of the player to act (pk_set_step_obs: dense + packed / packed only): every row against
    oracle_rows.  Every `views_every` steps pot / high_bet / game_over of the step_d handle BEFORE its reset (finished games stand) and of
    the step_auto_d handle against oracle_views.  Returns counts."""
    from pokerl_amd import _lib as L
    from pokerl_amd.hipmem import DeviceBuffer
    T, N, policy = cfg["T"], cfg["N"], cfg["policy"]
    D, P = 17 + 3 * N, 16 + 8 * (3 * N + 1)
    hd, ha, hb = (backend_of(HB, cfg) for _ in range(3))
    for x in (hd, ha, hb):
        x.reset(dealer=cfg["dealer"])
    act_a, fl_a, te_a, act_b, fl_b, te_b = bufs = [DeviceBuffer(n) for n in (T * 4, T, T) * 2]
    dense_a, packed_a, packed_b = obs = [DeviceBuffer(T * D * 8), DeviceBuffer(T * P), DeviceBuffer(T * P)]
    ha.g.set_step_obs(dense_a, packed_a); hb.g.set_step_obs(None, packed_b)
    all_t = np.ones(T, bool)
    st = dict(steps=2 * T * K, resets=0, rows=0, views=0, views_over=0)

    def rows_of(dense, packed):
        return (None if dense is None else dense.download(np.float64, T * D).reshape(T, D),
                None if packed is None else packed.download(np.uint8, T * P).reshape(T, P))

    for tr in game_step_trace(cfg, K):
        s, a, fo, eo, over, o = tr["s"], tr["a"], tr["fo"], tr["eo"], tr["over"], tr["o"]
        where = where_of(cfg, "step %d" % s)
        device_picks(ha.g, act_a, cfg, a); ha.g.step_d(act_a, fl_a, te_a, auto_reset=True)
        device_picks(hb.g, act_b, cfg, a); hb.g.step_d(act_b, fl_b, te_b)
        ha.g.sync(); hb.g.sync()
        assert np.array_equal(act_a.download(np.int32, T), a) and np.array_equal(act_b.download(np.int32, T), a), (where, "in-kernel agent picks")
        assert_flags(fl_b.download(np.uint8, T), te_b.download(np.uint8, T), fo, eo, False, where + " (step_d)")
        assert_flags(fl_a.download(np.uint8, T), te_a.download(np.uint8, T), fo, eo, True, where + " (step_auto_d)")
        st["rows"] += assert_rows(*rows_of(dense_a, packed_a), *tr["rows_auto"], all_t, where + " (step_auto_d)")
        st["rows"] += assert_rows(*rows_of(None, packed_b), *tr["rows"], all_t, where + " (step_d)")
        if views_every and s % views_every == views_every - 1:
            st["views"] += assert_views(hb.g, tr["pre"], where + " (step_d, before the reset)")
            st["views"] += assert_views(ha.g, tr["post"], where + " (step_auto_d)")
            st["views_over"] += int(oracle_views(tr["pre"])[2].sum())
        assert np.array_equal(hd.pick_actions(policy), a), (where, "pk_pick_actions")
        fh, eh = hd.step(a)
        assert_flags(fh, eh, fo, eo, False, where + " (host form)")
        hb.g.reset_d(fl_b, L.FLAG_GAME_OVER)              # HAND_OVER / TURN_OVER bits alone must not reset a table
        if (eo & 4).any():
            hb.g.reset_d(te_b, L.TERR_HAND_CAP)
        if over.any():
            hd.reset(mask=over)
            st["resets"] += int(over.sum())
        if (eo & 2).any():
            m = ((eo & 2) != 0).astype(np.uint8)
            ha.reset(mask=m); hb.reset(mask=m); hd.reset(mask=m)
        if s % snap_every == snap_every - 1 or s == K - 1:
            snap = o.snapshot()
            for h, form in ((hd, "host form"), (ha, "step_auto_d"), (hb, "step_d + reset_d")):
                GU.assert_snap(h.snapshot(), snap, where + " (%s)" % form)
    ha.g.set_step_obs(None, None); hb.g.set_step_obs(None, None)
    for b in bufs + obs:
        b.free()
    for h in (hd, ha, hb):
        h.g.close()
    return st


def game_step_async(HB, cfg, K, max_hands=1):
    """The bounded form of Game.step, pk_step_async_d (at most `max_hands` hand ends per launch, the reset inside), with a final drain: a
    step that rolls on stays in flight and is delivered by a later call; its flags / terr are those the oracle returned when the step
    started, its dense row (pk_set_step_obs) oracle_rows' at delivery, and after the drain every state byte is the oracle's.  The actions
    are the in-kernel agent's.  The twin stops at the first game.py:473 table of the lockstep trace (the caller would drain and reset
    it).  Returns counts."""
    from pokerl_amd.hipmem import DeviceBuffer
    T, N, policy = cfg["T"], cfg["N"], cfg["policy"]
    D = 17 + 3 * N
    hc, oc = backend_of(HB, cfg), oracle_of(cfg)
    hc.reset(dealer=cfg["dealer"]); oc.reset(dealer=cfg["dealer"])
    act_c, fl_c, te_c, rdy_c, dense_c = bufs = [DeviceBuffer(n) for n in (T * 4, T, T, T, T * D * 8)]
    hc.g.set_step_obs(dense_c, None)
    st = dict(async_steps=0, async_inflight=0, rows=0, drained=False)
    idle, want_f, want_e = np.ones(T, bool), np.zeros(T, np.uint8), np.zeros(T, np.uint8)
    off = False

    def call(actions_for_idle, budget, where):
        """One pk_step_async_d call against the oracle, which makes a step at the call that starts it.  Returns whether a delivered step
        ran into game.py:473."""
        nonlocal idle, want_f, want_e
        fo2, eo2 = oc.step(np.where(idle, actions_for_idle, -1).astype(np.int32))
        want_f, want_e = np.where(idle, fo2, want_f), np.where(idle, eo2, want_e)
        hc.g.step_async_d(act_c, fl_c, te_c, rdy_c, max_hands=budget, auto_reset=True); hc.g.sync()
        r = rdy_c.download(np.uint8, T) != 0
        fl, te = fl_c.download(np.uint8, T), te_c.download(np.uint8, T)
        assert_flags(np.where(r, fl, 0), np.where(r, te, 0), np.where(r, want_f, 0), np.where(r, want_e, 0), True, where + " (async)")
        m2 = (r & (over_of(want_f, want_e) != 0)).astype(np.uint8)
        if m2.any():
            oc.reset(mask=m2)
        st["rows"] += assert_rows(dense_c.download(np.float64, T * D).reshape(T, D), None, *oracle_rows(oc.snapshot(), N), r, where + " (async)")
        st["async_steps"] += int(r.sum()); st["async_inflight"] += int((~r).sum())
        idle = r.copy()
        return bool((r & ((want_e & 2) != 0)).any())

    for tr in game_step_trace(cfg, K):
        if off or (tr["eo"] & 2).any():
            off = True
            break
        device_picks(hc.g, act_c, cfg, oc.pick_actions(policy) if is_deep(cfg) else None); hc.g.sync()      # (deep: idle tables get the twin's next action)
        off = call(act_c.download(np.int32, T), max_hands, where_of(cfg, "step %d" % tr["s"]))
    act_c.upload(np.full(T, -1, np.int32))                # drain: idle tables get "no step"
    if not off:
        off = call(np.full(T, -1, np.int32), 0, where_of(cfg, "drain"))
        if not off:
            assert idle.all(), where_of(cfg, "drain left steps in flight")
            GU.assert_snap(hc.snapshot(), oc.snapshot(), where_of(cfg, "(async, drained)"))
            st["drained"] = True
    else:                                                 # (the twin stopped, perhaps with steps in flight: drain before the rows are unset)
        hc.g.step_async_d(act_c, fl_c, te_c, rdy_c, max_hands=0, auto_reset=True); hc.g.sync()
    hc.g.set_step_obs(None, None)
    for b in bufs:
        b.free()
    hc.g.close()
    return st


def seats_paid(tr):
    """Per table whose hand ended at this step of a game_step_trace(before=True): how many distinct non-zero amounts its seats RECEIVED
    from the pots (payoffs are net of the seat's own bets, game.py:531: received = payoff + what the seat had put in).  What a seat had put
    in is its bets + pending before the step, for the seat that acted its whole stack after ALL_IN.  Counted only where that is known and
    consistent: the step's action is FOLD, CHECK or ALL_IN, and every other seat's stack grew by exactly what it received (a step that rolls
    through several hands does not pass this); 0 elsewhere."""
    was, now, a = tr["was"], tr["pre"], np.asarray(tr["a"])
    T, N = was["credits"].shape
    ar, actor = np.arange(T), was["active"].astype(np.int64)
    put = was["bets"] + was["pending"]
    put[ar, actor] = np.where(a == 6, was["bets"][ar, actor] + was["credits"][ar, actor], put[ar, actor])
    got = now["payoffs"] + put
    others = np.arange(N)[None, :] != actor[:, None]
    known = ((tr["fo"] & 2) != 0) & (tr["eo"] == 0) & np.isin(a, (0, 1, 6))
    known &= (~others | (now["credits"] - was["credits"] + was["pending"] == got)).all(axis=1) & (got >= 0).all(axis=1)
    return np.array([len(set(g[g != 0].tolist())) if k else 0 for g, k in zip(got, known)])


# ------------------------------------------------------------------ 2. PokerGameEnv.step
def env_want(cfg, opp, K, seat0=None):
    """The oracle's half of the env families: per env.step with auto-reset what every table delivers -- (reward, done, hand, terr), where
    terr also holds an error raised by the reset that followed (the fused call reports it with the step's) -- the observation rows after
    it, and the actions seat 0 played.  `opp`: one policy or one per opponent seat.  Returns (want list, rows list, actions list, oracle, stats)."""
    o = oracle_of(cfg)
    o.env_reset(None, opp)
    seat0 = cfg["policy"] if seat0 is None else seat0
    want, rows, acts, step_terr = [], [], [], []
    capped = np.zeros(cfg["T"], bool)
    stats = dict(done=0, hands=0)
    for k in range(K):
        a = o.pick_actions(seat0)
        ro, do, ho, eo = o.env_step(a, opp)
        step_terr.append(eo)
        m = ((do != 0) | ((eo & CAPS) != 0)).astype(np.uint8)            # done, or PK_TERR_HAND_CAP / _ENV_CAP: auto-reset
        if m.any():
            o.env_reset(m, opp)
            eo = eo | (o.errs() * m)
        capped |= (eo & CAPS) != 0
        stats["done"] += int((do != 0).sum()); stats["hands"] += int((ho != 0).sum())
        want.append((ro, do, ho, eo)); acts.append(a); rows.append(oracle_rows(o.snapshot(), cfg["N"])[0])
    stats["capped"], stats["step_terr"] = int(capped.sum()), step_terr
    return want, rows, acts, o, stats


def env_step(cfg, opp, K, passes, B=1, exact_batches=True):
    """PokerGameEnv.step in its forms against env_want: the synchronous host call (pk_env_step + pk_env_reset of what ended), the fused
    call (pk_env_step_fused_d: seat 0 in-kernel, reset and observation row in the launch), and bounded launches (pk_env_step_async_d with
    `passes` Game.steps per launch; B > 1: in sub-batches, pk_set_env_batches) whose per-table delivered (reward, done, hand, terr, row)
    sequence must be the fused call's.  Returns counts."""
    from pokerl_amd import _lib as L
    from pokerl_amd.hipmem import DeviceBuffer
    lib = L.lib()
    T, N, seat0 = cfg["T"], cfg["N"], cfg["policy"]
    D = 17 + 3 * N
    where = where_of(cfg, "opp=%s K=%d passes=%d sub-batches=%d" % (opp, K, passes, B))
    want, rows, acts, o, wstats = env_want(cfg, opp, K)
    rew, done, hand, terr, obs, ready, act = bufs = [DeviceBuffer(n) for n in (T * 8, T, T, T, T * D * 8, T, T * 4)]
    deep = is_deep(cfg)                              # seat 0's actions are uploaded (actions_d non-NULL) instead of picked in the kernel
    A = np.stack(acts).astype(np.int32)
    out = lambda: (rew.download(np.float64, T), done.download(np.uint8, T), hand.download(np.uint8, T), terr.download(np.uint8, T),
                   obs.download(np.float64, T * D).reshape(T, D))
    st = dict(delivered=0, sub=0, launches=0)
    # ---- the host form: pk_env_step, then pk_env_reset of the episodes that ended (errors of that reset stay in the handle)
    env = env_of(opp, cfg)
    env.reset()
    for k in range(K):
        ob, r, d, h, e = env.step(acts[k], strict=False)
        assert_delivered((r, d, h, e), (want[k][0], want[k][1] != 0, want[k][2] != 0, wstats["step_terr"][k]), where + " pk_env_step %d" % k)
        m = (d | ((e & CAPS) != 0)).astype(np.uint8)
        if m.any():
            ob = env.reset(m)
        ok = want[k][3] == 0
        assert_rows(ob, None, rows[k], None, ok, where + " pk_env_step %d" % k)
    GU.assert_snap(_env_snapshot(env), o.snapshot(), where + " pk_env_step")
    env.close()
    # ---- fused
    env = env_of(opp, cfg)
    g = env.game
    env.reset()
    sync = []
    for k in range(K):
        if deep:
            act.upload(A[k])
        L.check(lib.pk_env_step_fused_d(g._h, act.ptr if deep else None, 0 if deep else seat0, env.opp_policy, 1, rew.ptr, done.ptr, hand.ptr, terr.ptr, obs.ptr), g._h)
        g.sync()
        w = out()
        assert_delivered(w[:4], want[k], where + " fused %d" % k)
        assert_rows(w[4], None, rows[k], None, want[k][3] == 0, where + " fused %d" % k)
        sync.append(w)
    GU.assert_snap(_env_snapshot(env), o.snapshot(), where + " fused")
    env.close()
    # ---- bounded launches of the same tables
    env = env_of(opp, cfg)
    g = env.game
    env.reset()
    nb = env.set_env_batches(B) if B > 1 else 1
    ranges = batch_ranges(T, B)                      # the split the header's rule gives, under any wave shape (not read back from the handle)
    if B > 1 and exact_batches:                      # (a small batch is cut into fewer ranges than asked for: a range is whole 64-table blocks)
        assert nb == B and env.last_range()[1] % 64 == 0, (where, nb, env.last_range())
        assert nb == len(ranges) and env.last_range() == ranges[0] + (True,), (where, nb, env.last_range(), ranges)
    st["sub"] = int(nb > 1)
    W = [np.stack([s[i] for s in sync]) for i in range(5)]
    count = np.zeros(T, np.int64)
    while count.min() < K:
        st["launches"] += 1
        # (a table whose seat 0 is broke with the game not over plays up to PK_ENV_STEP_CAP = 8 192 opponent steps per env.step: with a
        #  budget of `passes` Game.steps per launch that is ~8 192 / passes launches for ONE env.step -- slow, not stuck)
        assert st["launches"] < max(200, 2 * 8192 // passes + 50) * K * nb, (where, "no progress")
        if deep:                                     # action count[t] of the table's own sequence; -1 once it has delivered its K steps
            act.upload(np.where(count < K, A[np.minimum(count, K - 1), np.arange(T)], -1).astype(np.int32))
        env.step_async_d(act.ptr if deep else None, rew.ptr, done.ptr, hand.ptr, terr.ptr, obs.ptr, ready.ptr, max_passes=passes, seat0_policy=0 if deep else seat0)
        g.sync()
        r = ready.download(np.uint8, T) != 0
        if nb > 1:                                   # one range was launched; outputs are complete inside the DELIVERED range only
            db, de, fresh = env.last_range()
            assert not exact_batches or (db, de) in ranges, (where, (db, de), ranges)
            if fresh:
                continue
            inside = np.zeros(T, bool)
            inside[db:de] = True
            r &= inside
        idx = np.nonzero(r & (count < K))[0]
        w = out()
        assert_delivered(tuple(x[idx] for x in w), tuple(x[count[idx], idx] for x in W), where + " bounded launch %d" % st["launches"])
        st["delivered"] += len(idx)
        if deep:                                     # a table past its K steps was given -1: back at once, untouched, and not counted
            past = r & (count >= K)
            assert (w[3][past] == L.TERR_INVALID_ACTION).all(), (where, "a table given no action", np.nonzero(past)[0][:4].tolist())
        count[r] += 1
    if deep:
        act.upload(np.full(T, -1, np.int32))
    env.step_async_d(act.ptr if deep else None, rew.ptr, done.ptr, hand.ptr, terr.ptr, obs.ptr, ready.ptr, max_passes=0, seat0_policy=0 if deep else seat0)
    g.sync()
    assert (ready.download(np.uint8, T) != 0).all(), where
    if deep:                                         # every table has made exactly its K env.steps: the oracle's state
        GU.assert_snap(_env_snapshot(env), o.snapshot(), where + " bounded, drained")
    env.close()
    for b in bufs:
        b.free()
    return st


def _env_snapshot(env):
    from hip_backend import HipBackend
    hb = HipBackend.__new__(HipBackend)
    hb.env, hb.g, hb.T, hb.N = env, env.game, env.game.num_tables, env.game.num_players
    return hb.snapshot()


# ------------------------------------------------------------------ 3. one agent per seat, some seats played by the caller
def multi_want(cfg, pols, K):
    """env_want with one policy per opponent seat, stacked: ([K, T] reward, done, hand, terr), stats."""
    want, _, _, _, stats = env_want(cfg, list(pols), K, seat0=cfg["policy"] if is_deep(cfg) else 0)
    return [np.stack([w[i] for w in want]) for i in range(4)], stats


def multi_yields(cfg, pols, external, K):
    """The same K env.steps replayed through Game.step on a twin oracle (game_env.py:20-53 restated over all tables at once), counting how
    often a table stands at a caller-played seat: {seat: yields}.  The twin must end in the state orc_env_step_seats reaches."""
    T, N = cfg["T"], cfg["N"]
    o, ref = oracle_of(cfg), oracle_of(cfg)
    seatpol = np.array([0] + list(pols))
    yields = {s: 0 for s in external}

    def opponents_act(go):
        """One Game.step of the tables in `go` by the agent of the seat to act; the others are given no step."""
        snap_active = o.snapshot()["active"].astype(np.int64)
        for s in external:
            yields[s] += int((go & (snap_active == s)).sum())
        a = np.full(T, -1, np.int32)
        for pol in set(seatpol[1:].tolist()):
            pick = o.pick_actions(pol)
            sel = go & (seatpol[snap_active] == pol)
            a[sel] = pick[sel]
        fl, e = o.step(a)
        assert not e[go].any(), where_of(cfg, "twin replay: a cap or an error, replay undefined")
        return fl

    def reset(mask):
        o.reset(mask=mask.astype(np.uint8))
        go = mask & (o.snapshot()["active"] != 0)
        while go.any():
            fl = opponents_act(go)
            over = go & ((fl & 1) != 0)
            if over.any():
                o.reset(mask=over.astype(np.uint8))
            go = go & (o.snapshot()["active"] != 0)

    reset(np.ones(T, bool)); ref.env_reset(None, list(pols))
    for k in range(K):
        a = ref.pick_actions(0)
        ro, do, ho, eo = ref.env_step(a, list(pols))
        assert not eo.any(), where_of(cfg, "twin replay: caps")
        fl, e = o.step(a)
        done, hand = (fl & 1) != 0, (fl & 2) != 0
        fin = done | (o.snapshot()["states"][:, 0] == PS_BROKEN)
        while True:
            go = ~fin & ~hand & (o.snapshot()["active"] != 0)
            if not go.any():
                break
            fl = opponents_act(go)
            done, hand = np.where(go, (fl & 1) != 0, done), np.where(go, (fl & 2) != 0, hand)
        while True:
            go = ~fin & ~done & (o.snapshot()["active"] != 0)
            if not go.any():
                break
            fl = opponents_act(go)
            done = np.where(go, (fl & 1) != 0, done)
        assert np.array_equal(done | fin, do != 0), where_of(cfg, "twin replay: done, env.step %d" % k)
        if do.any():
            reset(do != 0); ref.env_reset(do, list(pols))
        GU.assert_snap(o.snapshot(), ref.snapshot(), where_of(cfg, "twin replay, env.step %d" % k))
    return yields


def env_multi(cfg, pols, external, K, passes, cap=6000):
    """pk_env_step_multi_d -- one agent per seat, the seats in `external` played by the caller by their policy's own rule (from the
    delivered row's valid mask and the table's step serial), bounded launches with auto-reset -- against multi_want: per table the
    delivered (reward, done, hand, terr) sequence is the oracle's.  At most cap * K launches.  Returns counts."""
    import pokerl_amd
    from pokerl_amd import _lib as L
    from pokerl_amd.hipmem import DeviceBuffer
    T, N, seed, base = cfg["T"], cfg["N"], cfg["seed"], cfg["base"]
    D = 17 + 3 * N
    where = where_of(cfg, "pols=%s external=%s K=%d passes=%d" % (pols, external, K, passes))
    W, _ = multi_want(cfg, pols, K)
    seat0 = cfg["policy"] if is_deep(cfg) else 0
    agents = [(lambda st: 0) if s in external else [pokerl_amd.RandomAgent(), pokerl_amd.AllInAgent(), pokerl_amd.CallAgent()][pols[s - 1]]
              for s in range(1, N)]
    env = env_of(agents, cfg)
    g = env.game
    rew, done, hand, terr, obs, who, ready, act, rst = bufs = [DeviceBuffer(n) for n in (T * 8, T, T, T, T * D * 8, T, T, T * 4, T)]
    count = np.full(T, -1, np.int64)                  # -1: the delivery of the initial reset is still to come
    rst.upload(np.ones(T, np.uint8))
    a = np.full(T, L.ACTION_SKIP, np.int32)
    st = dict(launches=0, delivered=0, yields=0, yields_by_seat={s: 0 for s in external})
    first = True
    while count.min() < K:
        st["launches"] += 1
        assert st["launches"] < cap * K, (where, "launch cap: no progress")
        act.upload(a)
        env.step_multi_d(act.ptr, rst.ptr if first else None, rew.ptr, done.ptr, hand.ptr, terr.ptr, obs.ptr, who.ptr, ready.ptr,
                         max_passes=passes, auto_reset=True)
        first = False
        g.sync()
        r, w = ready.download(np.uint8, T), who.download(np.uint8, T)
        rows = obs.download(np.float64, T * D).reshape(T, D)
        te = terr.download(np.uint8, T)
        ret = r == 1
        idx = np.nonzero(ret & (count >= 0) & (count < K))[0]
        if len(idx):
            got = (rew.download(np.float64, T)[idx], done.download(np.uint8, T)[idx], hand.download(np.uint8, T)[idx], te[idx])
            assert_delivered(got, tuple(x[count[idx], idx] for x in W), where + " launch %d" % st["launches"])
            st["delivered"] += len(idx)
        count[ret] += 1
        assert not te[r == 2].any() and np.isin(w[r == 2], external).all() and (w[ret] == 0).all(), where
        st["yields"] += int((r == 2).sum())
        for s in external:
            st["yields_by_seat"][s] += int(((r == 2) & (w == s)).sum())
        # the caller's moves: seat 0 by the random agent's rule, its opponent seats by their policy's rule, from the delivered
        # row's valid mask and the table's step serial (readable while env calls are in flight)
        a = np.full(T, -1, np.int32)
        serial = g.step_serial
        bits = (rows[:, 3:10] > 0).astype(np.uint32) @ (1 << np.arange(7, dtype=np.uint32))
        for t in np.nonzero((r == 1) | (r == 2))[0]:
            pol = seat0 if r[t] == 1 else pols[int(w[t]) - 1]
            a[t] = R.pick_action(seed, base + int(t), int(serial[t]), int(bits[t]), pol)
    env.end_multi()
    env.close()
    for b in bufs:
        b.free()
    return st


def env_in_kernel_seats(cfg, pols, K):
    """PokerGameEnv.step with one IN-KERNEL agent per seat (VecPokerGameEnv(agents=[...]).step over pk_env_step_multi_d, no caller-played
    seat), against the oracle with the same list; every state byte at the end."""
    import pokerl_amd
    where = where_of(cfg, "in-kernel pols=%s" % (pols,))
    agents = [[pokerl_amd.RandomAgent(), pokerl_amd.AllInAgent(), pokerl_amd.CallAgent()][p] for p in pols]
    env = env_of(agents, cfg)
    o = oracle_of(cfg)
    env.reset(); o.env_reset(None, list(pols))
    for k in range(K):
        a = o.pick_actions(0)
        ro, do, ho, eo = o.env_step(a, list(pols))
        ob, r, d, h, e = env.step(a, strict=False)
        assert_delivered((r, d, h, e), (ro, do != 0, ho != 0, eo), where + " env.step %d" % k)
        m = ((do != 0) | (eo != 0)).astype(np.uint8)
        if m.any():
            o.env_reset(m, list(pols)); env.reset(m)
    GU.assert_snap(_env_snapshot(env), o.snapshot(), where)
    env.close()


# ------------------------------------------------------------------ 4. rollouts
def rollout_call(HB, cfg, K):
    """PK_POLICY_CALL in the rollout kernels (k_rollout_call: fused, one step per launch, deferred launches) and pk_pick_actions against the
    oracle's call agent.  Returns the counters of the fused call."""
    o, h = oracle_of(cfg), backend_of(HB, cfg)
    o.reset(dealer=cfg["dealer"]); h.reset(dealer=cfg["dealer"])
    where = where_of(cfg, "call-agent rollout")
    a = o.pick_actions(2)
    assert np.array_equal(a, h.pick_actions(2)) and set(np.unique(a)) <= {1, 2, 6}, where
    co, _ = o.rollout(K, 2, True)
    ch = h.rollout(K, 2, True)
    assert ch.tolist() == co.tolist(), (where, "fused", co.tolist(), ch.tolist())
    GU.assert_snap(h.snapshot(), o.snapshot(), where + " fused")
    co2, _ = o.rollout(7, 2, True)
    ch2 = h.rollout(7, 2, True, fused=False)
    assert ch2.tolist() == co2.tolist(), (where, "one step per launch")
    for _ in range(5):                                   # asynchronous calls (deferred / merged) of the call agents
        h.g.rollout(9, 2, True, True, counters=False)
    o.rollout(45, 2, True)
    GU.assert_snap(h.snapshot(), o.snapshot(), where)
    h.g.close()
    return co


def rollout_then_lockstep(HB, cfg, K, lock=6, split=True, lock_policy=None):
    """Fused rollout (deferred launches of mixed lengths when `split`) and a few lockstep steps against the oracle.  lock_policy: the agent
    of the lockstep part where it is not the rollout's (R.POLICY_DEEP: the never-fold caller; the backend takes the oracle's actions)."""
    policy = cfg["policy"]
    o, h = oracle_of(cfg), backend_of(HB, cfg)
    o.reset(dealer=cfg["dealer"]); h.reset(dealer=cfg["dealer"])
    where = where_of(cfg, "start=%s bb=%s sb=%s policy=%d K=%d" % (cfg["start"], cfg["bb"], cfg["sb"], policy, K))
    GU.assert_snap(h.snapshot(), o.snapshot(), where + " reset")
    co, _ = o.rollout(K, policy, True)
    if split:
        k1 = K // 3                                                  # (K >= 48: both deferred launches are >= 16 steps, which k_rollout_tab / _allin_tab take up to 6 / 10 seats)
        h.g.rollout(k1, policy, True, True, counters=False)          # deferred launches of mixed lengths ...
        h.g.rollout(K - k1 - 7, policy, True, True, counters=False)
        ch = h.rollout(7, policy, True)                              # ... and a completing one
    else:
        ch = h.rollout(K, policy, True)
    assert co.tolist() == ch.tolist(), where
    GU.assert_snap(h.snapshot(), o.snapshot(), where + " rollout")
    for s in range(lock):
        a = o.pick_actions(policy if lock_policy is None else lock_policy)
        fo, eo = o.step(a)
        fh, eh = h.step(a)
        assert np.array_equal(fo, fh) and np.array_equal(eo, eh), where
        bad = ((fo & 1) | (eo != 0)).astype(np.uint8)
        if bad.any():
            o.reset(mask=bad); h.reset(mask=bad)
    GU.assert_snap(h.snapshot(), o.snapshot(), where + " lockstep")
    h.g.close()
    return cfg["T"] * (K + lock)


def deep_lockstep(h, o, cfg, K):
    """K lockstep steps of the deep caller on a backend (pk_step_d with the oracle's actions uploaded, pk_reset_d of finished games; None:
    the oracle alone) and the oracle, flags and terr compared at every step, every state byte at the end.  Returns the tables standing
    past the flop with three or more seats in the hand."""
    T = cfg["T"]
    if h is not None:
        from pokerl_amd import _lib as L
        from pokerl_amd.hipmem import DeviceBuffer
        act, fl, te = bufs = [DeviceBuffer(n) for n in (T * 4, T, T)]
    for s in range(K):
        a = o.pick_actions(cfg["policy"])
        fo, eo = o.step(a)
        assert not (eo & 2).any(), where_of(cfg, "deep lockstep step %d: game.py:473" % s)
        over = over_of(fo, eo)
        if over.any():
            o.reset(mask=over)
        if h is not None:
            act.upload(a)
            h.g.step_d(act, fl, te); h.g.sync()
            assert_flags(fl.download(np.uint8, T), te.download(np.uint8, T), fo, eo, False, where_of(cfg, "deep lockstep step %d" % s))
            h.g.reset_d(fl, L.FLAG_GAME_OVER)
            if (eo & 4).any():
                h.g.reset_d(te, L.TERR_HAND_CAP)
    snap = o.snapshot()
    if h is not None:
        for b in bufs:
            b.free()
        GU.assert_snap(h.snapshot(), snap, where_of(cfg, "after %d deep lockstep steps" % K))
    return int(((snap["turn"] >= 1) & (np.isin(snap["states"], (1, 2, 3)).sum(axis=1) >= 3)).sum())


def rollout_from_deep(HB, cfg, K, K_roll=K_ROLLOUT):
    """K lockstep deep steps, then the fused rollout of the CALL agents for K_roll steps in deferred launches (16 / 25 / 7 at 48): the rollout
    kernels (k_rollout_call, and the table-evaluator variants where the seat count selects them) finish hands whose pots were built over
    several streets, with all-in and broke seats.  Counters and every state byte against the oracle.  Returns (tables mid-hand past the
    flop among three or more seats when the rollout starts, the counters)."""
    o, h = oracle_of(cfg), backend_of(HB, cfg)
    o.reset(dealer=cfg["dealer"]); h.reset(dealer=cfg["dealer"])
    where = where_of(cfg, "rollout from deep tables")
    deep_tables = deep_lockstep(h, o, cfg, K)
    co, err = o.rollout(K_roll, 2, True)
    assert err == 0, where
    k1 = K_roll // 3
    h.g.rollout(k1, 2, True, True, counters=False)
    h.g.rollout(K_roll - k1 - 7, 2, True, True, counters=False)
    ch = h.rollout(7, 2, True)
    assert co.tolist() == ch.tolist(), (where, co.tolist(), ch.tolist())
    GU.assert_snap(h.snapshot(), o.snapshot(), where)
    h.g.close()
    return deep_tables, co


def played(HB, cfg, K, extra_call=0):
    """(backend, oracle) after reset, a K-step rollout of the configuration's agents and `extra_call` steps of the call agents (which
    bring tables past the flop where the configuration's own agents end every hand at once), state compared.  deep: K lockstep steps of
    the deep caller instead (deep_lockstep) -- tables mid-hand past the flop with all-in and broke seats."""
    o, h = oracle_of(cfg), backend_of(HB, cfg)
    o.reset(dealer=cfg["dealer"]); h.reset(dealer=cfg["dealer"])
    if is_deep(cfg):
        deep_lockstep(h, o, cfg, K)
        return h, o
    played_oracle(cfg, K, extra_call, o)
    h.rollout(K, cfg["policy"], True)
    if extra_call:
        h.rollout(extra_call, 2, True)
    GU.assert_snap(h.snapshot(), o.snapshot(), where_of(cfg, "played %d + %d" % (K, extra_call)))
    return h, o


def played_oracle(cfg, K, extra_call=0, o=None):
    if o is None:
        o = oracle_of(cfg)
        o.reset(dealer=cfg["dealer"])
    if is_deep(cfg):
        deep_lockstep(None, o, cfg, K)
        return o
    o.rollout(K, cfg["policy"], True)
    if extra_call:
        o.rollout(extra_call, 2, True)
    return o


# ------------------------------------------------------------------ 5. snapshots
def snapshots(HB, cfg, K, extra_call=0, observer="active", nonce=5):
    """Save / load (host and device blobs), a permuted clone inside the handle, and a clone with redeal into a second handle, on tables as
    `played` leaves them: the restored handle continues in lockstep with the oracle; the clone holds the oracle's state of its source and
    continues with it while the hand goes on; the redealt cards are tests/snapshot_spec.redeal's for the observer."""
    import pokerl_amd
    import snapshot_spec as SS
    from pokerl_amd.hipmem import DeviceBuffer
    T, N, policy = cfg["T"], cfg["N"], cfg["policy"]
    where = where_of(cfg, "snapshots")
    h, o = played(HB, cfg, K, extra_call)
    g = h.g
    blob = g.save()
    hd = SS.header(blob)
    assert (hd["magic"], hd["version"], hd["n"], hd["m"]) == (SS.MAGIC, SS.VERSION, N, T), where
    buf = DeviceBuffer(pokerl_amd.snapshot_nbytes(N, T))
    g.save_d(buf); g.sync()
    assert np.array_equal(buf.download(np.uint8, blob.size), blob), (where, "host and device blobs")
    # the redeal first (it reads the handle as it stands)
    seed2, base2 = 0xABCDEF12345, 2 ** 32 - 7
    d = pokerl_amd.VecGame(T, num_players=N, start_credits=cfg["start"], big_blind=cfg["bb"], small_blind=cfg["sb"], seed=seed2, table_id_base=base2)
    assert_shape(d, cfg)
    d.reset()
    rng = np.random.default_rng(N)
    perm = rng.permutation(T).astype(np.int32)
    d.clone_tables(perm, np.arange(T), src=g, observer=observer, nonce=nonce)
    src = o.snapshot()
    got = _game_snapshot(d)
    GU.assert_snap({k: (got[k][perm] if k != "cards" else src[k]) for k in GU.SNAP_FIELDS}, src, where + " redeal: non-card fields")
    for i in range(T):
        t = int(perm[i])
        p = int(src["active"][i]) if observer == "active" else int(observer)
        exp = SS.redeal(src["cards"][i], N, int(src["turn"][i]), p, seed2, base2 + t, nonce)
        assert np.array_equal(got["cards"][t], exp), (where, "redeal", observer, i)
    d.close()
    # off course, then restore: host blob into the handle, device blob into a twin
    g.step(g.pick_actions(2), strict=False)
    g.reset(mask=(np.arange(T) % 3 == 0).astype(np.uint8))
    g.rollout(7, policy=0, counters=False)
    g.load(blob)
    GU.assert_snap(h.snapshot(), o.snapshot(), where + " right after load")
    assert not g.owed.any(), where
    twin = backend_of(HB, cfg)
    twin.g.load_d(buf); twin.g.sync()
    buf.free()
    GU.assert_snap(twin.snapshot(), o.snapshot(), where + " right after load_d into a fresh handle")
    for s in range(8):
        a = o.pick_actions(policy)
        fo, eo = o.step(a)
        for x in (h, twin):
            fh, eh = x.step(a)
            assert_flags(fh, eh, fo, eo, False, where + " step %d after load" % s)
        m = over_of(fo, eo)
        if m.any():
            o.reset(mask=m); h.reset(mask=m); twin.reset(mask=m)
    GU.assert_snap(h.snapshot(), o.snapshot(), where + " after load")
    GU.assert_snap(twin.snapshot(), o.snapshot(), where + " after load_d")
    twin.g.close()
    # permuted clone: table t <- table perm[t], every table both a source and a destination
    src = o.snapshot()
    g.clone_tables(np.arange(T), perm)
    GU.assert_snap(h.snapshot(), {k: src[k][perm] for k in GU.SNAP_FIELDS}, where + " right after the clone")
    a = o.pick_actions(policy)
    fo, eo = o.step(a)
    fh, eh = h.step(a[perm])
    cont = (fo[perm] & 2) == 0                           # hand going on: no card of the destination's own decks is dealt
    assert_flags(np.where(cont, fh, fh & 2), eh, np.where(cont, fo[perm], fo[perm] & 2), eo[perm], False, where + " step after the clone")
    so, sh = o.snapshot(), h.snapshot()
    GU.assert_snap({k: sh[k][cont] for k in GU.SNAP_FIELDS}, {k: so[k][perm][cont] for k in GU.SNAP_FIELDS}, where + " step after the clone, hand going on")
    g.close()
    return dict(cont=int(cont.sum()))


def _game_snapshot(g):
    from hip_backend import HipBackend
    hb = HipBackend.__new__(HipBackend)
    hb.env, hb.g, hb.T, hb.N = None, g, g.num_tables, g.num_players
    return hb.snapshot()


# ------------------------------------------------------------------ 6. equity
EQUITY_KEYS = ("win", "tie", "share", "boards", "status")
EQUITY_FIRST = 24


def equity_tables(turn, first=EQUITY_FIRST):
    """The first `first` tables past the flop (pre-flop enumeration in numpy is too slow at 13+ seats)."""
    return np.nonzero(np.asarray(turn) >= 1)[0][:first].astype(np.int32)


def assert_counts(got, want, keys, where):
    for k in keys:
        a, b = np.asarray(got[k]).astype(np.uint64), np.asarray(want[k]).astype(np.uint64)
        assert a.shape == b.shape and (a == b).all(), (where, k, np.argwhere(a != b)[:4].tolist())


def equity(HB, cfg, K, extra_call=0, observer=-2, samples=65, nonce=11):
    """pk_table_equity against equity_spec, and pk_table_equity_sampled as `observer` (a seat, -2 = each table's active seat, -1 = nobody:
    all hole cards known) sees the tables against equity_sampled_spec, both fed from the getters of tables as `played` leaves them, through
    the index-array form restricted to equity_tables.  Exact counts."""
    import equity_sampled_spec as SS
    import equity_spec as ES
    where = where_of(cfg, "equity")
    h, o = played(HB, cfg, K, extra_call)
    g = h.g
    pick = equity_tables(g.turn)
    assert len(pick) == EQUITY_FIRST, (where, "tables past the flop", len(pick))
    holes, board, nboard, live = ES.table_spots(g.deck, g.player_states, g.turn)
    want = ES.batch_equity(holes[pick], board[pick], nboard[pick], live[pick])
    r = g.equity(pick)
    assert not want["status"].any(), where
    assert_counts({k: getattr(r, k) for k in EQUITY_KEYS}, want, EQUITY_KEYS, where + " pk_table_equity")
    holes, board, nboard, live = SS.table_spots(g.deck, g.player_states, g.turn, g.active_player, observer)
    ids = (cfg["base"] + pick.astype(np.int64)) % 2 ** 32
    want = SS.batch_equity(holes[pick], board[pick], nboard[pick], live[pick], samples, nonce=nonce, ids=ids, key=R.seed_key(cfg["seed"]))
    r = g.equity_sampled(pick, observer=observer, samples=samples, nonce=nonce)
    assert not want["status"].any() and (want["samples"] == samples).all(), where
    assert_counts({k: getattr(r, k) for k in SS.KEYS}, want, SS.KEYS, where + " pk_table_equity_sampled observer %d" % observer)
    g.close()
    return dict(tables=len(pick), samples=int(np.asarray(r.samples).sum()))


def extra_call(kind, N):
    """Call-agent steps after the configuration's own rollout in the snapshot and equity families: they bring most tables past the flop (the
    ladder's all-in agents end every hand at once, and random agents at many seats rarely see a flop)."""
    return 2 * N + 3
