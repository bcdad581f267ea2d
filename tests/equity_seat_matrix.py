"""Shared drivers (TEST INFRASTRUCTURE): every seat-templated equity kernel -- k_equity<N>, k_eqs<N>, k_eqw<N, RC>, k_ev<N> and k_evw<N> with
their prep kernels, and the table forms of the five -- against the numpy restatements of their definitions, for one seat count at a time.

One copy of each case: tests/test_hip_equity_seat_matrix.py runs them on the device at every seat count 2 .. 16, and
tests/test_equity_seat_matrix_host.py runs the spec halves without a GPU and holds the INPUTS to what they are there for (ties that reach
seat N - 1, every group of pot levels, bet sums that round differently in numpy's order, accepted attempts with every seat hidden), so
that a GPU case cannot pass by comparing nothing.  The oracle halves (`case`, `want`, `table_state`, `table_want`) need numpy, oracle/ and
the spec modules only; the device halves (`device_host`, `device_stream`, `table_device`) import pokerl_amd when called.  Every comparison
is exact: integers equal, every f64 byte for byte."""
import ctypes as C
import functools

import numpy as np

import equity_ranged_spec as WS
import equity_sampled_spec as SS
import equity_spec as ES
import ev_spec as EV
import ranged_ev_spec as XS
from oracle import rng_spec as R

SEATS = list(range(2, 17))
SPOT_FAMILIES = ("equity", "sampled", "ranged", "ev", "ranged_ev")
FAMILIES = SPOT_FAMILIES + ("table_forms",)
STREAM_SEATS = (4, 8, 12, 13, 15)    # the device forms on a caller's stream are written once for all N: the word edges of the range rows and both level groupings
SEED = 0x5EED0123456789AB
S_SAMPLED = 65                       # one full wavefront plus one lane
S_RANGED = 130                       # two full wavefronts plus two lanes
T_TABLES, S_TABLE = 8, 65
TABLE_BASE = 2 ** 32 - 3             # table ids that wrap inside the batch
U = WS.UNIFORM
ROYAL = [0x09, 0x0A, 0x0B, 0x0C, 0x00]                # TS JS QS KS AS: the board plays for everyone
KEYS = {"equity": ("win", "tie", "share", "boards", "status"), "sampled": SS.KEYS, "ranged": WS.KEYS,
        "ev": ("share", "level_seat", "amount", "ev", "boards", "status"), "ranged_ev": XS.KEYS}
COUNT_OF = {"equity": "boards", "sampled": "samples", "ranged": "accepted", "ev": "boards", "ranged_ev": "accepted"}
TABLE_PARTS = {"equity": "equity", "equity_ev": "ev", "equity_sampled": "sampled", "equity_ranged": "ranged", "ev_ranged": "ranged_ev"}
# (family, N) -> a salt of the case's generator, where the plain one misses a floor of tests/test_equity_seat_matrix_host.py (chosen there,
# with the spec on the CPU; nothing here comes from a kernel)
SALT = {("ranged", 3): 1, ("ranged", 9): 1, ("ranged", 14): 6, ("ranged", 15): 6, ("ranged_ev", 13): 1, ("ranged_ev", 14): 1, ("ranged_ev", 16): 1,
        ("table_forms", 15): 2}
TABLE_RANDOM_STEPS = 3               # table_state: steps of the random agents (they fold) before the never-fold caller takes over
TABLE_STEP_CAP = 400


def rng_of(family, N, part=0):
    return np.random.default_rng([0xE95EA7, FAMILIES.index(family), N, part, SALT.get((family, N), 0)])


def where_of(family, N, what=""):
    return "equity seat matrix %s N=%d%s" % (family, N, " " + what if what else "")


def ev_group(N):
    """Pot levels per task of k_ev / k_evw, restated: 3 up to eight seats, 2 from nine on."""
    return 3 if N <= 8 else 2


def ev_groups_max(N):
    return (N - 1 + ev_group(N) - 1) // ev_group(N)


def groups_with_work(level_seat, amount, N):
    """The groups of levels that have a level to compare, as a bit mask: level i (not the last stand) with amount > 0 sets bit i // ev_group(N)."""
    nlev = int((np.asarray(level_seat) != EV.NO_LEVEL).sum())
    mask = 0
    for i in range(nlev):
        last = i == nlev - 1 and nlev == N                            # (N level records on N live seats: the N-th is the last stand)
        if not last and amount[i] > 0:
            mask |= 1 << (i // ev_group(N))
    return mask


def disjoint_rows(rng=None):
    """Sixteen rows of three holdings each over cards 3 r .. 3 r + 2: sixteen drawn holdings never collide."""
    w = np.zeros((16, WS.HOLDINGS), np.uint16)
    for r in range(16):
        for a, b in ((3 * r, 3 * r + 1), (3 * r, 3 * r + 2), (3 * r + 1, 3 * r + 2)):
            w[r, b * (b - 1) // 2 + a] = 1 + 1000 * r + a if rng is None else int(rng.integers(1, 65536))
    return w


def full_ladder(N, descending=False):
    """No two bets equal: N - 1 compared levels and a last stand."""
    b = 10.0 * (np.arange(N) + 1)
    return b[::-1].copy() if descending else b


FRAC_PLAIN = (0.1, 33.33, 3)         # one level that rounds differently left to right at 8 .. 15 seats, seven at 16
FRAC_DENSE = (1.1, 11.11, 4)         # three or four such levels at 8 .. 15 seats, eight at 16 (found by a search over a few such patterns)


def frac_ladder(N, pattern=FRAC_DENSE):
    """a (p + 1) + b (p % k): no two bets equal, and from eight seats on the clipped bets of some levels add up to different bits in
    numpy's pairwise order than left to right (tests/test_equity_seat_matrix_host.py asserts it for both patterns)."""
    a, b, k = pattern
    p = np.arange(N)
    return a * (p + 1) + b * (p % k)


def sum_left_to_right(x):
    r = np.float64(x[0])
    for v in x[1:]:
        r = r + np.float64(v)
    return r


def order_sensitive_levels(bets, live):
    """The levels of ev_spec.levels whose amount differs between np.sum and a plain left-to-right loop over the same addends."""
    bets = np.asarray(bets, np.float64)
    work, out = bets.copy(), []
    for i, (s, amount, remain, last) in enumerate(EV.levels(bets, live)):
        addends = work if last else np.clip(work, 0, work[s])
        assert np.float64(amount).tobytes() == np.float64(np.sum(addends)).tobytes()
        if np.float64(np.sum(addends)).tobytes() != np.float64(sum_left_to_right(addends)).tobytes():
            out.append(i)
        if not last:
            work = work - addends
    return out


def deal(rng, N, skip=()):
    """Distinct hole cards [N, 2] and five more cards from a shuffled deck without `skip`."""
    cards = np.array([c for c in ES.CANON if c not in skip], np.uint8)
    cards = cards[rng.permutation(len(cards))]
    return cards[:2 * N].reshape(N, 2).copy(), cards[2 * N:2 * N + 5].copy()


def full(N):
    return (1 << N) - 1


def folded_mask(rng, N, top_folded=False):
    """A live mask with at least one folded seat (at two seats: one live seat); top_folded: seat N - 1 is among the folded."""
    while True:
        m = int(rng.integers(1, 1 << N))
        if top_folded:
            m &= ~(1 << (N - 1))
        if m and m != full(N) and (bin(m).count("1") >= 2 or N <= 2 + top_folded):
            return m


# ------------------------------------------------------------------ the cases: inputs per family and seat count
@functools.lru_cache(maxsize=None)
def case(family, N):
    """The inputs of `family`'s case at N seats: a list of calls, each a dict of the host form's arguments plus `parts` (name -> spot
    indices).  Cached: callers leave the arrays as they are."""
    return {"equity": equity_case, "sampled": sampled_case, "ranged": ranged_case, "ev": ev_case, "ranged_ev": ranged_case}[family](N, family)


def stack(spots):
    holes, board, nboard, live = zip(*spots)
    return dict(holes=np.array(holes, np.uint8), board=np.array(board, np.uint8), nboard=np.array(nboard, np.uint8), live=np.array(live, np.uint16))


def equity_case(N, family="equity"):
    """Three spots on each of nb = 5, 4, 3 -- every seat live; seat N - 1 alone; folded seats, some of them unknown -- one all-live spot at
    nb = 2 (C(50 - 2 N, 3) boards), and the royal flush on the board with every seat live."""
    rng = rng_of(family, N)
    spots, parts = [], {"all_live": [], "top_alone": [], "folded": [], "royal": []}
    for nb in (5, 4, 3, 2):
        for kind in ("all_live", "top_alone", "folded") if nb > 2 else ("all_live",):
            holes, board = deal(rng, N)
            live = {"all_live": full(N), "top_alone": 1 << (N - 1), "folded": folded_mask(rng, N)}[kind]
            if kind == "folded":
                for p in range(N):
                    if not (live >> p) & 1 and rng.integers(0, 2):
                        holes[p] = ES.UNKNOWN                          # a folded hand nobody saw: its cards are in the pool
            parts[kind].append(len(spots))
            spots.append((holes, board, nb, live))
    holes, _ = deal(rng, N, skip=[c for c in ES.CANON if c >> 4 == 0])   # no spade in a hand: nothing extends or shifts the board's run
    parts["royal"].append(len(spots))
    spots.append((holes, np.array(ROYAL, np.uint8), 5, full(N)))
    return [dict(stack(spots), parts=parts)]


def sampled_case(N, family="sampled"):
    """Twelve spots of equity_sampled_spec.random_spots (hidden masks: none, all, one byte, random) on nb = i % 6, and one spot with every
    seat live and hidden pre-flop: D = 2 N + 5 draws.  Ids that are not the identity; S = 65."""
    rng = rng_of(family, N)
    holes, board, nboard, live = SS.random_spots(rng, N, 12)
    nboard[:] = np.arange(12) % 6
    holes = np.concatenate([holes, np.full((1, N, 2), ES.UNKNOWN, np.uint8)])
    board = np.concatenate([board, board[:1]])
    nboard, live = np.append(nboard, np.uint8(0)), np.append(live, np.uint16(full(N)))
    ids = rng.integers(0, 2 ** 32, 13, dtype=np.uint64).astype(np.uint32)
    return [dict(holes=holes, board=board, nboard=nboard, live=live, ids=ids, samples=S_SAMPLED, nonce=N, parts={"random": list(range(12)), "all_hidden": [12]})]


def ranged_case(N, family):
    """Two calls.  The first on the sixteen disjoint three-holding rows: (a) every seat live and hidden, pre-flop with range_of = arange(N)
    and on the flop with its reverse -- H = N, so H + 1 words and every packed word of range rows in use; (b) seat N - 1 shown, the rest
    hidden, one of them uniform, pre-flop and on the turn; (d) two spots with nothing hidden.  The second on the mixed four rows of
    equity_ranged_spec.random_ranges: (c) six spots of its random_spots -- rejection, and spots that accept nothing.  S = 130; ids that are
    not the identity.  ranged_ev: the fractional ladder on (a) and (b), ranged_ev_spec.bet_patterns on (c) and (d)."""
    rng = rng_of(family, N)
    top = [ES.CANON[3 * (N - 1)], ES.CANON[3 * (N - 1) + 1]]                 # two cards of row N - 1, which no hidden seat of (b) draws from
    flop = [ES.CANON[48], ES.CANON[49], ES.CANON[50], ES.CANON[51], 0]        # the four cards no row holds
    hidden = np.full((N, 2), ES.UNKNOWN, np.uint8)
    shown = hidden.copy()
    shown[N - 1] = top
    spots = [(hidden, [0] * 5, 0, full(N)), (hidden, flop, 3, full(N)), (shown, [0] * 5, 0, full(N)), (shown, flop, 4, full(N))]
    ro = [np.arange(N), np.arange(N)[::-1], np.arange(N), np.arange(N)]
    ro[2], ro[3] = ro[2].copy(), ro[3].copy()
    ro[2][0], ro[3][max(N - 2, 0)] = U, U
    for nb in (3, 4):
        holes, board = deal(rng, N)
        spots.append((holes, board, nb, folded_mask(rng, N)))
        ro.append(np.arange(N))
    first = dict(stack(spots), weights=disjoint_rows(), range_of=np.array(ro, np.uint16), parts={"a": [0, 1], "b": [2, 3], "d": [4, 5]})
    holes, board, nboard, live = WS.random_spots(rng, N, 6)
    second = dict(holes=holes, board=board, nboard=nboard, live=live, weights=WS.random_ranges(rng_of(family, N, 1)),
                  range_of=rng.choice(np.array([0, 1, 2, 3, U], np.uint16), (6, N)), parts={"c": list(range(6))})
    for k, call in enumerate((first, second)):
        m = len(call["nboard"])
        call.update(ids=rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32), samples=S_RANGED, nonce=2 * N + k)
    if family == "ranged_ev":
        first["bets"] = np.array([frac_ladder(N)] * 4 + [XS.bet_patterns(N, first["live"][i], i - 1) for i in (4, 5)], np.float64)
        second["bets"] = np.array([XS.bet_patterns(N, live[i], i) for i in range(6)], np.float64)
    return [first, second]


def ev_case(N, family="ev"):
    """Every seat live on a turn spot and a flop spot: the full ladder (ascending on the turn, descending on the flop) and the fractional
    ladder (FRAC_PLAIN on the turn, FRAC_DENSE on the flop); the royal flush on the board under the ascending ladder; a turn spot with folded seats that hold dead money, the folded seat
    N - 1 above every live bet; a flop spot with one live seat."""
    rng = rng_of(family, N)
    spots, bets, parts = [], [], {}

    def add(name, holes, board, nb, live, b):
        parts.setdefault(name, []).append(len(spots))
        spots.append((holes, board, nb, live))
        bets.append(np.asarray(b, np.float64))

    for nb in (4, 3):
        add("ladder", *deal(rng, N), nb, full(N), full_ladder(N, descending=nb == 3))
        add("frac", *deal(rng, N), nb, full(N), frac_ladder(N, FRAC_PLAIN if nb == 4 else FRAC_DENSE))
    holes, _ = deal(rng, N, skip=[c for c in ES.CANON if c >> 4 == 0])
    add("royal", holes, np.array(ROYAL, np.uint8), 5, full(N), full_ladder(N))
    live = folded_mask(rng, N, top_folded=True)
    b = np.array([5.0 * (p + 1) if (live >> p) & 1 else 3.0 + p for p in range(N)])
    b[N - 1] = 5.0 * N + 50.0
    add("dead_money", *deal(rng, N), 4, live, b)
    add("one_live", *deal(rng, N), 3, 1 << (N // 2), full_ladder(N))
    return [dict(stack(spots), bets=np.array(bets, np.float64), parts=parts)]


# ------------------------------------------------------------------ what the specs say
@functools.lru_cache(maxsize=None)
def want(family, N):
    """The spec's outputs for case(family, N): one dict per call.  Cached: callers leave the arrays as they are."""
    return [spec_call(family, c) for c in case(family, N)]


def spec_call(family, c):
    if family == "equity":
        return ES.batch_equity(c["holes"], c["board"], c["nboard"], c["live"])
    if family == "ev":
        return EV.batch_ev(c["holes"], c["board"], c["nboard"], c["live"], c["bets"])
    if family == "sampled":
        return SS.batch_equity(c["holes"], c["board"], c["nboard"], c["live"], c["samples"], SEED, c["nonce"], c["ids"])
    if family == "ranged":
        return WS.batch_equity(c["holes"], c["board"], c["nboard"], c["live"], c["samples"], c["weights"], c["range_of"], per_spot=True, seed=SEED,
                               nonce=c["nonce"], ids=c["ids"])
    assert family == "ranged_ev"
    return XS.batch_ev(c["holes"], c["board"], c["nboard"], c["live"], c["bets"], c["samples"], c["weights"], c["range_of"], per_spot=True, seed=SEED,
                       nonce=c["nonce"], ids=c["ids"])


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def invariants(family, out, where):
    """On every call of every case: a refused spot is all zero (level_seat 0xFF), and the shares of a spot -- of each of its levels that
    pays -- add up to 720720 * (boards | samples | accepted) exactly."""
    out = {k: np.asarray(v) for k, v in out.items()}
    count = out[COUNT_OF[family]].astype(object)
    bad = out["status"] != 0
    for k in KEYS[family]:
        if k == "level_seat":
            assert (out[k][bad] == EV.NO_LEVEL).all(), (where, k)
        elif k != "status":
            assert not (bits(out[k][bad]) if out[k].dtype == np.float64 else out[k][bad]).any(), (where, k)
    sums = out["share"].astype(object).sum(axis=-1)
    if family in ("ev", "ranged_ev"):
        paid = (out["level_seat"] != EV.NO_LEVEL) & (out["amount"] > 0)
        assert np.where(paid, sums == count[:, None] * ES.SHARE_UNIT, sums == 0).all(), (where, "share sums")
    else:
        assert (sums == count * ES.SHARE_UNIT).all(), (where, "share sums")
        assert ((out["win"].astype(np.int64) + out["tie"]) <= out[COUNT_OF[family]].astype(np.int64)[:, None]).all(), (where, "win + tie")


def assert_same(family, got, want_, where):
    """Every output of one call against the spec (or another form of the call): integers equal, f64 bit for bit."""
    if family == "ev":
        EV.assert_same(got, want_, where)
    elif family == "ranged_ev":
        XS.assert_same(got, want_, where)
    else:
        for k in KEYS[family]:
            a, b = np.asarray(got[k]).astype(np.uint64), np.asarray(want_[k]).astype(np.uint64)
            assert a.shape == b.shape and (a == b).all(), (where, k, np.argwhere(a != b)[:4].tolist())


def royal_shares(N):
    """What the royal flush on the board gives without any spec: equity -- win 0, tie 1, share 720720 / N at every seat; under the
    ascending ladder level i splits 720720 / (N - i) among the seats >= i and the last stand pays seat N - 1."""
    ev = np.zeros((N, N), np.uint64)
    for i in range(N):
        ev[i, i:] = ES.SHARE_UNIT // (N - i)
    return ES.SHARE_UNIT // N, ev


def assert_royal(family, N, out, where):
    i = case(family, N)[0]["parts"]["royal"][0]
    eq, ev = royal_shares(N)
    assert out["status"][i] == 0 and out["boards"][i] == 1, where
    if family == "equity":
        assert not out["win"][i].any() and (out["tie"][i] == 1).all() and (out["share"][i] == eq).all(), (where, "royal")
    else:
        assert np.array_equal(np.asarray(out["share"][i], np.uint64), ev) and out["level_seat"][i].tolist() == list(range(N)), (where, "royal")


# ------------------------------------------------------------------ the device halves of the spot families
def device_call(family, N, c):
    """The host form of one call through pokerl_amd.judger -> dict of its outputs."""
    from pokerl_amd import judger as J
    spots = (c["holes"], c["board"], c["nboard"], c["live"])
    if family == "equity":
        r = J.showdown_equity_batch(*spots)
    elif family == "ev":
        r = J.showdown_ev_batch(*spots, c["bets"])
    elif family == "sampled":
        r = J.sampled_equity_batch(*spots, c["samples"], SEED, c["nonce"], c["ids"])
    elif family == "ranged":
        r = J.ranged_equity_batch(*spots, c["weights"], c["range_of"], c["samples"], SEED, c["nonce"], c["ids"])
    else:
        r = J.ranged_ev_batch(*spots, c["bets"], c["weights"], c["range_of"], c["samples"], SEED, c["nonce"], c["ids"])
    return {k: np.asarray(getattr(r, k)) for k in KEYS[family]}


def device_host(family, N):
    """case(family, N) through the host forms: one dict per call, the invariants checked."""
    outs = []
    for k, c in enumerate(case(family, N)):
        out = device_call(family, N, c)
        invariants(family, out, where_of(family, N, "host form, call %d" % k))
        outs.append(out)
    return outs


def out_layout(family, m, N):
    """name -> (dtype, shape) of a call's outputs on m spots."""
    if family in ("ev", "ranged_ev"):
        lay = dict(share=(np.uint64, (m, N, N)), level_seat=(np.uint8, (m, N)), amount=(np.float64, (m, N)), ev=(np.float64, (m, N)))
    else:
        lay = dict(win=(np.uint32, (m, N)), tie=(np.uint32, (m, N)), share=(np.uint64, (m, N)))
    lay[COUNT_OF[family]] = (np.uint32, (m,))
    lay["status"] = (np.uint8, (m,))
    return lay


class DeviceOuts:
    """Device buffers for a call's outputs, pre-filled with 0x5A (the call writes every output it is given itself)."""

    def __init__(self, family, m, N):
        from pokerl_amd import hipmem
        self.lay = out_layout(family, m, N)
        self.buf = {}
        for k, (dt, shape) in self.lay.items():
            nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
            self.buf[k] = hipmem.DeviceBuffer(nbytes).upload(np.full(nbytes, 0x5A, np.uint8))

    def ptr(self, k):
        return self.buf[k].ptr

    def fetch(self):
        return {k: self.buf[k].download(dt, int(np.prod(shape))).reshape(shape) for k, (dt, shape) in self.lay.items()}

    def free(self):
        for b in self.buf.values():
            b.free()


def device_stream(family, N):
    """case(family, N) through the device forms (pk_X_d) on a caller's non-blocking stream: one dict per call."""
    from pokerl_amd import hipmem
    from pokerl_amd import judger as J
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0             # hipStreamNonBlocking: a caller's own stream
    outs = []
    for c in case(family, N):
        m = len(c["nboard"])
        up = {k: hipmem.DeviceBuffer(np.ascontiguousarray(c[k]).nbytes).upload(np.ascontiguousarray(c[k]))
              for k in ("holes", "board", "nboard", "live", "bets", "ids", "weights", "range_of") if k in c}
        spots = [up[k].ptr for k in ("holes", "board", "nboard", "live")]
        o = DeviceOuts(family, m, N)
        if family == "equity":
            J.showdown_equity_d(N, m, *spots, o.ptr("win"), o.ptr("tie"), o.ptr("share"), o.ptr("boards"), o.ptr("status"), stream=stream)
        elif family == "ev":
            J.showdown_ev_d(N, m, *spots, up["bets"].ptr, o.ptr("status"), o.ptr("share"), o.ptr("level_seat"), o.ptr("amount"), o.ptr("ev"),
                            o.ptr("boards"), stream=stream)
        elif family == "sampled":
            J.sampled_equity_d(N, m, *spots, c["samples"], ids_d=up["ids"].ptr, seed=SEED, nonce=c["nonce"], win_d=o.ptr("win"), tie_d=o.ptr("tie"),
                               share_d=o.ptr("share"), samples_d=o.ptr("samples"), status_d=o.ptr("status"), stream=stream)
        elif family == "ranged":
            J.ranged_equity_d(N, m, *spots, c["samples"], up["weights"].ptr, len(c["weights"]), up["range_of"].ptr, ids_d=up["ids"].ptr, seed=SEED,
                              nonce=c["nonce"], win_d=o.ptr("win"), tie_d=o.ptr("tie"), share_d=o.ptr("share"), accepted_d=o.ptr("accepted"),
                              status_d=o.ptr("status"), stream=stream)
        else:
            J.ranged_ev_d(N, m, *spots, up["bets"].ptr, c["samples"], o.ptr("status"), weights_d=up["weights"].ptr, num_ranges=len(c["weights"]),
                          range_of_d=up["range_of"].ptr, ids_d=up["ids"].ptr, seed=SEED, nonce=c["nonce"], share_d=o.ptr("share"),
                          level_seat_d=o.ptr("level_seat"), amount_d=o.ptr("amount"), ev_d=o.ptr("ev"), accepted_d=o.ptr("accepted"), stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        outs.append(o.fetch())
        o.free()
        for b in up.values():
            b.free()
    assert hip.hipStreamDestroy(stream) == 0
    return outs


def assert_same_bytes(family, got, other, where):
    """Two forms of one call: every output byte for byte."""
    for k in KEYS[family]:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(other[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (where, k)


# ------------------------------------------------------------------ the table forms
def table_config(N):
    """Eight tables on per-seat stacks 20 + frac_ladder(N) -- side pots, and from eight seats on level amounts that round differently left
    to right (the all-in bets are the stacks) --, table ids that wrap inside the batch."""
    return dict(tables=T_TABLES, n=N, start_credits=(20.0 + frac_ladder(N)).tolist(), seed=0x7AB1E5 * 1000003 + 7919 * N + SALT.get(("table_forms", N), 0),
                table_id_base=TABLE_BASE)


def table_targets():
    """The street every table is driven to: turn 1 (flop), 2 (turn), 3 (river) by turns -- at least two streets, and no pre-flop table,
    whose enumeration the numpy spec cannot afford at few seats."""
    return 1 + np.arange(T_TABLES) % 3


def table_state(b):
    """Drives a backend of golden_util's interface (the C oracle, tests/hip_backend.HipBackend) to the matrix's table state: a few steps of
    the random agents, who fold, then the never-fold caller of oracle/rng_spec.py, who raises on every street; a table that has reached its
    target street is given no further step (action -1: refused, the table stays as it is), a finished game is reset.  Returns the snapshot."""
    b.reset()
    target = table_targets()
    for s in range(TABLE_STEP_CAP):
        snap = b.snapshot()
        there = snap["turn"] >= target
        if there.all():
            return snap
        a = np.where(there, -1, b.pick_actions(0 if s < TABLE_RANDOM_STEPS else R.POLICY_DEEP)).astype(np.int32)
        flags, _ = b.step(a)
        over = ((flags & 1) != 0) & ~there
        if over.any():
            b.reset(mask=over.astype(np.uint8))
    raise AssertionError("table_state: %d steps did not bring every table to its street" % TABLE_STEP_CAP)


def table_rows(N):
    """N range rows over disjoint runs of 52 // N cards each, every holding inside a run with a weight of its own: hidden seats on rows of
    their own never collide with each other, only with the board and the observer."""
    k = 52 // N
    w = np.zeros((N, WS.HOLDINGS), np.uint16)
    for r in range(N):
        for b in range(k * r, k * r + k):
            for a in range(k * r, b):
                w[r, b * (b - 1) // 2 + a] = 1 + (7 * a + 13 * b + r) % 50
    return w


def table_range_of(N):
    """Seat p draws from row p; at five seats and more seat 1 is uniform."""
    ro = np.arange(N).astype(np.uint16)
    if N >= 5:
        ro[1] = U
    return ro


def table_want(N, deck, player_states, turn, active, bets, pending_bets):
    """What the five specs say for the tables the getters describe, the spots taken through each spec module's table_spots; observer
    N - 1 where a family takes one -> {method name: outputs}."""
    cfg = table_config(N)
    ids = (cfg["table_id_base"] + np.arange(T_TABLES)) % 2 ** 32
    key = R.seed_key(cfg["seed"])
    o = N - 1
    out = {}
    out["equity"] = ES.batch_equity(*ES.table_spots(deck, player_states, turn))
    out["equity_ev"] = EV.batch_ev(*ES.table_spots(deck, player_states, turn), np.asarray(bets, np.float64) + np.asarray(pending_bets, np.float64))
    out["equity_sampled"] = SS.batch_equity(*SS.table_spots(deck, player_states, turn, active, o), S_TABLE, nonce=N, ids=ids, key=key)
    out["equity_ranged"] = WS.batch_equity(*WS.table_spots(deck, player_states, turn, active, o), S_TABLE, table_rows(N), table_range_of(N), nonce=N, ids=ids, key=key)
    holes, board, nboard, live, b = XS.table_spots(deck, player_states, turn, active, o, bets, pending_bets)
    out["ev_ranged"] = XS.batch_ev(holes, board, nboard, live, b, S_TABLE, table_rows(N), table_range_of(N), nonce=N, ids=ids, key=key)
    return out


def table_want_of_snapshot(N, snap):
    return table_want(N, snap["cards"][:, :5 + 2 * N], snap["states"], snap["turn"], snap["active"], snap["bets"], snap["pending"])


def table_backend(N):
    from hip_backend import HipBackend
    cfg = table_config(N)
    return HipBackend(cfg["tables"], N, start_credits=cfg["start_credits"], seed=cfg["seed"], table_id_base=cfg["table_id_base"])


def table_device(g, N):
    """The five host table forms of a handle -> {method name: outputs}, the invariants checked."""
    o = N - 1
    res = dict(equity=g.equity(), equity_ev=g.equity_ev(), equity_sampled=g.equity_sampled(observer=o, samples=S_TABLE, nonce=N),
               equity_ranged=g.equity_ranged(observer=o, ranges=table_rows(N), range_of=table_range_of(N), samples=S_TABLE, nonce=N),
               ev_ranged=g.ev_ranged(observer=o, ranges=table_rows(N), range_of=table_range_of(N), samples=S_TABLE, nonce=N))
    out = {}
    for name, r in res.items():
        fam = TABLE_PARTS[name]
        out[name] = {k: np.asarray(getattr(r, k)) for k in KEYS[fam]}
        invariants(fam, out[name], where_of("table_forms", N, name))
    return out


def table_device_stream(g, N):
    """The five device table forms (pk_table_X_d) with the handle on a caller's non-blocking stream -> {method name: outputs}."""
    from pokerl_amd import hipmem
    hip = hipmem._lib()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    g.set_stream(stream)
    w, ro = table_rows(N), table_range_of(N)
    wd, rd = hipmem.DeviceBuffer(w.nbytes).upload(w), hipmem.DeviceBuffer(ro.nbytes).upload(ro)
    o, m = N - 1, T_TABLES
    outs = {name: DeviceOuts(fam, m, N) for name, fam in TABLE_PARTS.items()}
    d = outs["equity"]
    g.equity_d(win_d=d.ptr("win"), tie_d=d.ptr("tie"), share_d=d.ptr("share"), boards_d=d.ptr("boards"), status_d=d.ptr("status"))
    d = outs["equity_ev"]
    g.equity_ev_d(d.ptr("status"), share_d=d.ptr("share"), level_seat_d=d.ptr("level_seat"), amount_d=d.ptr("amount"), ev_d=d.ptr("ev"), boards_d=d.ptr("boards"))
    d = outs["equity_sampled"]
    g.equity_sampled_d(observer=o, samples=S_TABLE, nonce=N, win_d=d.ptr("win"), tie_d=d.ptr("tie"), share_d=d.ptr("share"), samples_d=d.ptr("samples"),
                       status_d=d.ptr("status"))
    d = outs["equity_ranged"]
    g.equity_ranged_d(observer=o, weights_d=wd, num_ranges=N, range_of_d=rd, samples=S_TABLE, nonce=N, win_d=d.ptr("win"), tie_d=d.ptr("tie"),
                      share_d=d.ptr("share"), accepted_d=d.ptr("accepted"), status_d=d.ptr("status"))
    d = outs["ev_ranged"]
    g.ev_ranged_d(d.ptr("status"), observer=o, weights_d=wd, num_ranges=N, range_of_d=rd, samples=S_TABLE, nonce=N, share_d=d.ptr("share"),
                  level_seat_d=d.ptr("level_seat"), amount_d=d.ptr("amount"), ev_d=d.ptr("ev"), accepted_d=d.ptr("accepted"))
    assert hip.hipStreamSynchronize(stream) == 0
    got = {name: d.fetch() for name, d in outs.items()}
    g.use_own_stream()
    for x in list(outs.values()) + [wd, rd]:
        x.free()
    assert hip.hipStreamDestroy(stream) == 0
    return got
